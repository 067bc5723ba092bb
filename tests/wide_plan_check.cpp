// wide_plan_check.cpp — the launch plan's decisions about the wide work-groups of the persistent-wave traversal
// (ray_tracer_amd/csrc/launch_plan.h: KernelKey::threads, Tuning::wideMinSlots, DispatchFacts::groupThreads), as worked cases on
// the CPU: when trace_kernel_key returns the wide key, that every other key is what it was, the knob, the grid of a wide launch
// and the LDS sum. Driven by tests/test_wide_plan.py; tests/launch_plan_check.cpp pins everything else.
#include "launch_plan.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <string>

#include "scene_layout.h"   // RT_MAP_*, RT_HOT_PAIRS
#include "check.h"

static DispatchFacts slots(uint32_t nPixels, uint32_t nFrames = 1) { DispatchFacts d; d.nPixels = nPixels; d.nFrames = nFrames; d.samples = 1; return d; }
static Tuning tuned(const char* key, int value) {
    Tuning t;
    const TuningChange ch = set_tuning(t, key, value);
    CHECK(ch.error.empty(), "%s %d: %s", key, value, ch.error.c_str());
    return t;
}
static SceneFacts scene(uint32_t depth, uint32_t hotNodes = 192, bool cull = false) { SceneFacts s; s.maxLeafDepth = depth; s.hotNodes = hotNodes; s.cull = cull; return s; }
static bool same(const KernelKey& k, KernelFamily family, int stack, bool ovf, bool pix, bool stats, bool cull, int hot, int blocks, int threads) {
    return k.family == family && k.stack == stack && k.ovf == ovf && k.pix == pix && k.stats == stats && k.cull == cull && k.hot == hot && k.blocks == blocks && k.threads == threads;
}
static bool wide(const KernelKey& k) { return k.threads != RT_BLOCK; }
static std::string show(const KernelKey& k) {
    char m[160];
    snprintf(m, sizeof m, "family %d <%d, ovf %d, pix %d, stats %d, cull %d, hot %d, blocks %d, threads %d>", (int)k.family, k.stack, (int)k.ovf, (int)k.pix, (int)k.stats, (int)k.cull, k.hot, k.blocks, k.threads);
    return m;
}

// the shipped shape: two groups of 768 threads are six waves per SIMD, with the whole table of the scene layout
static_assert(RT_WIDE_THREADS == 768 && RT_WIDE_GROUPS == 2 && RT_WIDE_HOT == 192, "the shipped wide work-group");
static_assert(RT_WIDE_HOT <= (int)RT_HOT_PAIRS, "no more pairs than the scene layout puts first");
static_assert(wide_group_lds(20, 192, 768) == 64512 + 1024 + 12288, "stacks, object metadata, table");
static_assert(RT_WIDE_GROUPS * wide_group_lds(20, RT_WIDE_HOT, RT_WIDE_THREADS) <= 160 * 1024, "the LDS sum of the shipped shape");
static_assert(wide_group_lds(20, RT_WIDE_HOT, RT_WIDE_THREADS) <= 81920, "half a CU's LDS per group");

static void check_wide_key() {
    const KernelFamily PW = KernelFamily::trace_pw;
    const Tuning t;
    const uint32_t big = 2u << 20, small = 3072;
    CHECK(t.wideMinSlots == t.lanesMinSlots && t.wideMinSlots == 1u << 20, "the default is the size at which a dispatch goes into parts: %llu", (unsigned long long)t.wideMinSlots);
    for (uint32_t depth : {17u, 20u}) {
        KernelKey k = trace_kernel_key(t, scene(depth), slots(big));
        CHECK(same(k, PW, 20, false, false, false, false, RT_WIDE_HOT, RT_WIDE_GROUPS, RT_WIDE_THREADS), "depth %u, 2 M pixels: %s", depth, show(k).c_str());
        k = trace_kernel_key(t, scene(depth), slots(small));
        CHECK(same(k, PW, 20, false, false, false, false, 144, 5, RT_BLOCK), "depth %u, 3 072 pixels: %s", depth, show(k).c_str());
        // the threshold itself, and the frames of a dispatch count together
        CHECK(wide(trace_kernel_key(t, scene(depth), slots(1u << 20))) && !wide(trace_kernel_key(t, scene(depth), slots((1u << 20) - 1))), "2^20 paths");
        CHECK(wide(trace_kernel_key(t, scene(depth), slots(131072, 8))) && !wide(trace_kernel_key(t, scene(depth), slots(131072, 7))), "eight frames of 2^17 pixels");
    }
    CHECK(!wide(trace_kernel_key(t, scene(20), DispatchFacts{})), "a default DispatchFacts has no paths");

    // ---- everything else keeps the parent's key at any size, and is never wide
    struct Case { const char* what; Tuning t; SceneFacts sc; DispatchFacts d; KernelFamily family; int stack; bool ovf, pix, stats, cull; int hot, blocks; };
    DispatchFacts heat = slots(big); heat.pixStats = true;
    DispatchFacts perRay = slots(big); perRay.perRay = true;
    DispatchFacts phases = slots(big); phases.phaseStats = 1;
    SceneFacts alpha = scene(18); alpha.mapFlags = RT_MAP_ALPHA;
    const Case cases[] = {
        {"cull", t, scene(18, 192, true), slots(big), PW, 20, false, false, false, true, 144, 5},
        {"depth 16", t, scene(16), slots(big), PW, 16, false, false, false, false, 192, 5},
        {"depth 21", t, scene(21), slots(big), PW, 24, false, false, false, false, 80, 5},
        {"hot_pairs 0", tuned("hot_pairs", 0), scene(18), slots(big), PW, 20, false, false, false, false, 0, 6},
        {"hot_pairs 1", tuned("hot_pairs", 1), scene(18), slots(big), PW, 20, false, false, false, false, 72, 6},
        {"lds_stack 16", tuned("lds_stack", 16), scene(18), slots(big), PW, 16, true, false, false, false, 120, 6},
        {"no top levels", t, scene(18, 0), slots(big), PW, 20, false, false, false, false, 0, 6},
        {"heat map", t, scene(18), heat, PW, 20, false, true, false, false, 0, 6},
        {"per-ray counters", t, scene(18), perRay, PW, 20, false, true, false, false, 0, 6},
        {"phase statistics", t, scene(18), phases, PW, 20, false, true, true, false, 0, 6},
        {"alpha map", t, alpha, slots(big), KernelFamily::trace_pw_alpha, 24, true, false, false, false, 0, 0},
        {"trace_variant 0", tuned("trace_variant", 0), scene(18), slots(big), KernelFamily::trace, 24, false, false, false, false, 0, 0},
    };
    for (const Case& c : cases)
        for (int always : {0, 1}) {   // ... also with the knob at "always"
            Tuning tt = c.t;
            if (always) CHECK(set_tuning(tt, "wide_min_kslots", 0).error.empty(), "wide_min_kslots 0");
            const KernelKey k = trace_kernel_key(tt, c.sc, c.d);
            CHECK(same(k, c.family, c.stack, c.ovf, c.pix, c.stats, c.cull, c.hot, c.blocks, RT_BLOCK), "%s%s: %s", c.what, always ? ", wide_min_kslots 0" : "", show(k).c_str());
        }
    // the fused pipeline has no wide kernel
    CHECK(fused_kernel_key(t, scene(18), slots(big)).threads == RT_BLOCK, "fused");
}

static void check_knob() {
    KernelKey k = trace_kernel_key(tuned("wide_min_kslots", 0), scene(18), slots(3072));
    CHECK(wide(k) && k.hot == RT_WIDE_HOT && k.blocks == RT_WIDE_GROUPS, "wide_min_kslots 0, 3 072 pixels: %s", show(k).c_str());
    CHECK(wide(trace_kernel_key(tuned("wide_min_kslots", 0), scene(18), DispatchFacts{})), "wide_min_kslots 0, no pixels: always");
    k = trace_kernel_key(tuned("wide_min_kslots", INT_MAX), scene(18), slots(2u << 20));
    CHECK(same(k, KernelFamily::trace_pw, 20, false, false, false, false, 144, 5, RT_BLOCK), "wide_min_kslots INT_MAX, 2 M pixels: %s", show(k).c_str());
    CHECK(!wide(trace_kernel_key(tuned("wide_min_kslots", INT_MAX), scene(18), slots(UINT_MAX))), "no dispatch reaches INT_MAX * 1024 paths");
    CHECK(tuned("wide_min_kslots", 5).wideMinSlots == 5120, "wide_min_kslots counts 1024 paths");
    CHECK(tuned("wide_min_kslots", INT_MAX).wideMinSlots == (uint64_t)INT_MAX << 10, "... in 64 bits");
    Tuning t;
    CHECK(set_tuning(t, "wide_min_kslots", -1).error == "wide_min_kslots >= 0", "\"%s\"", set_tuning(t, "wide_min_kslots", -1).error.c_str());
    CHECK(set_tuning(t, "wide_min_kslots", INT_MIN).error == "wide_min_kslots >= 0", "INT_MIN");
    CHECK(t.wideMinSlots == 1u << 20, "a refused value leaves the knob as it was");
    CHECK(!set_tuning(t, "wide_min_kslots", 7).rebuildEmitters, "the emitter list does not follow it");
    // the other knobs of the parts leave it alone
    CHECK(tuned("lanes_min_kslots", 1).wideMinSlots == 1u << 20, "lanes_min_kslots does not move it");
}

static void check_wide_shape() {
    const SceneFacts sc;
    Measured m;
    // blocks: a work-group per `threads` rays, at most the part's share of the resident work-groups, at least one. The share of a
    // launch of wide groups beside other parts (gridPct < 100) is wide_grid_pct, 40 by default; lane_grid_pct given by hand wins
    struct Grid { const char* key; int value; uint32_t maxRays, resident; int gridPct; uint32_t threads; int pct; uint32_t blocks; };
    const Grid grids[] = {
        {"", 0, 1u << 20, 512, 100, 768, 100, 512}, {"", 0, 1u << 20, 512, 50, 768, 40, 204}, {"", 0, 1u << 20, 512, 40, 768, 40, 204},
        {"", 0, 1, 512, 100, 768, 100, 1}, {"", 0, 1, 512, 50, 768, 40, 1},
        {"", 0, 768, 512, 100, 768, 100, 1}, {"", 0, 769, 512, 100, 768, 100, 2}, {"", 0, 800, 512, 100, 768, 100, 2}, {"", 0, 64, 512, 100, 768, 100, 1},
        {"", 0, 100000, 512, 100, 768, 100, 131}, {"", 0, 100000, 512, 50, 768, 40, 131},
        {"", 0, 1u << 20, 2, 50, 768, 40, 1}, {"", 0, UINT_MAX, 512, 100, 768, 100, 512}, {"", 0, 3u << 30, 768, 50, 512, 40, 307},
        {"wide_grid_pct", 0, 1u << 20, 512, 50, 768, 50, 256}, {"wide_grid_pct", 60, 1u << 20, 512, 50, 768, 60, 307}, {"wide_grid_pct", 60, 1u << 20, 512, 100, 768, 100, 512},
        {"lane_grid_pct", 50, 1u << 20, 512, 50, 768, 50, 256}, {"lane_grid_pct", 30, 1u << 20, 512, 30, 768, 30, 153},
        // the 256-thread groups as they were, whatever wide_grid_pct says
        {"", 0, 1000, 1280, 100, 256, 100, 4}, {"", 0, 1u << 20, 1280, 50, 256, 50, 640}, {"wide_grid_pct", 20, 1u << 20, 1280, 50, 256, 50, 640},
    };
    for (const Grid& g : grids) {
        Tuning t;
        if (g.key[0]) t = tuned(g.key, g.value);
        DispatchFacts d; d.gridPct = g.gridPct; d.groupThreads = g.threads;
        const TraceShape s = trace_shape(t, m, sc, d, g.maxRays, g.resident);
        const uint64_t need = ((uint64_t)g.maxRays + g.threads - 1) / g.threads, cap = std::max<uint64_t>(1, (uint64_t)g.resident * g.pct / 100);
        CHECK(s.blocks == g.blocks, "%s %d: %u rays in groups of %u, %u resident, %d %%: %u blocks, want %u", g.key, g.value, g.maxRays, g.threads, g.resident, g.gridPct, s.blocks, g.blocks);
        CHECK(s.blocks == (uint32_t)std::min(need, cap), "ceil(rays / threads) capped by resident x share");
    }
    CHECK(DispatchFacts{}.groupThreads == RT_BLOCK, "256 threads unless the key says otherwise");
    // the knob
    Tuning t;
    CHECK(t.wideGridPct == 40, "default share of the wide groups in parts: %d", t.wideGridPct);
    for (int bad : {-1, 1, 9, 101}) CHECK(set_tuning(t, "wide_grid_pct", bad).error == "wide_grid_pct: 0 (the parts' share) or 10..100", "wide_grid_pct %d", bad);
    CHECK(t.wideGridPct == 40, "a refused value leaves the knob as it was");
    CHECK(tuned("wide_grid_pct", 10).wideGridPct == 10 && tuned("wide_grid_pct", 100).wideGridPct == 100 && tuned("wide_grid_pct", 0).wideGridPct == 0, "accepted at both ends and at 0");
    // the parts' own share is not touched (tests/launch_plan_check.cpp pins it)
    CHECK(part_grid_pct(t, 3, 6912000) == 50 && part_grid_pct(t, 3, 691200) == 40 && part_grid_pct(t, 1, 6912000) == 100, "part_grid_pct");
}

int main() {
    check_wide_key();
    check_knob();
    check_wide_shape();
    return check_finish("wide plan ok");
}
