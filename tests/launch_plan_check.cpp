// launch_plan_check.cpp — the launch policy (ray_tracer_amd/csrc/launch_plan.h) restated as worked cases and checked on the CPU:
// the pipeline, the probe, the parts, their slices and grid share, the frames per dispatch, the kernel key with its depth buckets
// and top-level tables, the launch shapes, the measured statistics and every tuning key. The expected values follow DESIGN.md §4
// and the comment blocks beside each decision. Driven by tests/test_launch_plan.py.
// (Not pinned on purpose: what a new scene keeps of the previous scene's measurements — that is rt_device.hip's measured_new_scene.)
#include "launch_plan.h"

#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "scene_layout.h"   // RT_MAP_*
#include "check.h"

static Measured measured(double boxPerRay, double segPerPath = -1.0) { Measured m; m.boxPerRay = boxPerRay; m.segPerPath = segPerPath; return m; }
static DispatchFacts slots(uint32_t nPixels, uint32_t nFrames = 1, uint32_t samples = 1) { DispatchFacts d; d.nPixels = nPixels; d.nFrames = nFrames; d.samples = samples; return d; }
static Tuning tuned(const char* key, int value) {
    Tuning t;
    const TuningChange ch = set_tuning(t, key, value);
    CHECK(ch.error.empty(), "%s %d: %s", key, value, ch.error.c_str());
    return t;
}

// ---------------------------------------------------------------- pipeline
static void check_pipeline() {
    const Tuning t;
    const SceneFacts small;
    SceneFacts big;   // 3.2 MB of child pairs + 2.4 MB of triangle positions: more than one XCD's 4 MiB of L2
    big.nodeCount = 100000; big.triCount = 50000;
    struct Case { double boxPerRay; uint32_t nPixels, nFrames; const SceneFacts* sc; int want; };
    const Case cases[] = {
        {-1.0, 65536, 1, &small, 1},
        {-1.0, 8294400, 1, &small, 0},
        {10.0, 3686400, 1, &small, 1},
        {10.0, 2073600, 10, &small, 1},     // 20 736 000 slots
        {153.0, 2073600, 1, &small, 0},
        {153.0, 921600, 1, &small, 1},
        {33.0, 2073600, 10, &big, 0},
        {33.0, 8294400, 1, &big, 1},
        {20.0, 2073600, 10, &big, 1},
        {33.0, 2073600, 10, &small, 1},
        // the size limit: 4 M paths up to 90 tests per ray, 2.75 M at 120, 1.5 M from 150 on
        {70.0, 3999999, 1, &small, 1}, {70.0, 4000000, 1, &small, 0},
        {90.0, 3999999, 1, &small, 1}, {90.0, 4000000, 1, &small, 0},
        {120.0, 2740000, 1, &small, 1}, {120.0, 2760000, 1, &small, 0},
        {150.0, 1499999, 1, &small, 1}, {150.0, 1500001, 1, &small, 0},
        {153.0, 1499999, 1, &small, 1}, {153.0, 1500000, 1, &small, 0},
        {400.0, 1499999, 1, &small, 1}, {400.0, 1500000, 1, &small, 0},
        // short rays end just below 70 tests, very short ones just below 25, the big dispatch begins at 10 * 2^20 paths
        {69.9, 2073600, 10, &small, 1}, {70.0, 2073600, 10, &small, 0},
        {24.9, 2073600, 10, &big, 1}, {25.0, 2073600, 10, &big, 0},
        {33.0, (10u << 20) - 1, 1, &big, 1}, {33.0, 10u << 20, 1, &big, 0},
    };
    for (const Case& c : cases) {
        const int got = choose_pipeline(t, measured(c.boxPerRay), *c.sc, slots(c.nPixels, c.nFrames));
        CHECK(got == c.want, "%.1f tests per ray, %u pixels x %u frames, %s scene: pipeline %d, want %d", c.boxPerRay, c.nPixels, c.nFrames, c.sc == &big ? "big" : "small", got, c.want);
    }
    // the scene's size is child pairs and triangle positions together, and 4 MiB itself is still small
    SceneFacts edge; edge.nodeCount = 131072; edge.triCount = 0;
    CHECK(choose_pipeline(t, measured(33.0), edge, slots(2073600, 10)) == 1, "4 MiB of nodes");
    edge.triCount = 1;
    CHECK(choose_pipeline(t, measured(33.0), edge, slots(2073600, 10)) == 0, "4 MiB of nodes and a triangle");
    // "pipeline" wins over the size and the ray cost; a scene that binds a map takes the multi-kernel pipeline unless fused_maps
    DispatchFacts forced = slots(8294400); forced.pipeline = 1;
    CHECK(choose_pipeline(t, measured(153.0), small, forced) == 1, "pipeline 1");
    forced = slots(65536); forced.pipeline = 0;
    CHECK(choose_pipeline(t, measured(10.0), small, forced) == 0, "pipeline 0");
    for (uint32_t flags : {RT_MAP_METALNESS, RT_MAP_ALPHA, RT_MAP_BUMP}) {
        SceneFacts maps; maps.mapFlags = flags;
        forced = slots(65536); forced.pipeline = 1;
        CHECK(choose_pipeline(t, measured(10.0), maps, forced) == 0, "map %u, pipeline 1, fused_maps 0", flags);
        CHECK(choose_pipeline(tuned("fused_maps", 1), measured(10.0), maps, forced) == 1, "map %u, pipeline 1, fused_maps 1", flags);
        CHECK(choose_pipeline(tuned("fused_maps", 1), measured(-1.0), maps, slots(8294400)) == 0, "map %u, fused_maps 1 chooses as usual", flags);
    }
    // the two knobs of the automatic choice
    CHECK(choose_pipeline(tuned("fused_below_pixels", 1000000), measured(-1.0), small, slots(1000000)) == 0, "fused_below_pixels");
    CHECK(choose_pipeline(tuned("fused_below_box_tests", 160), measured(153.0), small, slots(2073600, 10)) == 1, "fused_below_box_tests");
}

// ---------------------------------------------------------------- the probe
static void check_probe() {
    const Tuning t;
    const SceneFacts sc;
    const DispatchFacts big = slots(2073600, 1, 4);   // 8.3 M pixel samples
    CHECK(probe_first(t, measured(-1.0), sc, big), "an unmeasured scene's first big dispatch");
    CHECK(probe_first(t, measured(-1.0), sc, slots(1000000, 1, 8)), "8 M pixel samples exactly");
    CHECK(!probe_first(t, measured(-1.0), sc, slots(999999, 1, 8)), "just below 8 M pixel samples");
    CHECK(!probe_first(t, measured(33.0), sc, big), "measured");
    CHECK(!probe_first(tuned("probe", 0), measured(-1.0), sc, big), "probe 0");
    DispatchFacts d = big; d.probe = true;
    CHECK(!probe_first(t, measured(-1.0), sc, d), "the probe itself");
    d = big; d.debug = 0;
    CHECK(!probe_first(t, measured(-1.0), sc, d), "heat map");
    SceneFacts maps; maps.mapFlags = RT_MAP_BUMP;
    CHECK(!probe_first(t, measured(-1.0), maps, big), "a scene that binds a map");

    struct Case { TileRows tile, want; };
    const Case cases[] = {
        {{0, 1, 1080}, {67, 135, 8}},   // a whole 1080p frame: eight rows spread over it
        {{3, 8, 135}, {67, 128, 8}},    // rank 3 of 8, interleaved rows
        {{0, 1, 5}, {0, 1, 5}},         // fewer than eight rows: all of them
        {{10, 2, 8}, {10, 2, 8}},
        {{0, 1, 15}, {0, 1, 8}},
    };
    for (const Case& c : cases) {
        const TileRows r = probe_rows(c.tile);
        CHECK(r.row0 == c.want.row0 && r.rowStride == c.want.rowStride && r.nRows == c.want.nRows, "rows %u + k*%u, k < %u: probe %u + k*%u, k < %u",
              c.tile.row0, c.tile.rowStride, c.tile.nRows, r.row0, r.rowStride, r.nRows);
        CHECK(r.row0 + (r.nRows - 1) * r.rowStride <= c.tile.row0 + (c.tile.nRows - 1) * c.tile.rowStride, "the probe's rows are the tile's");
    }
}

// ---------------------------------------------------------------- parts
static void check_parts() {
    const Tuning t;
    const SceneFacts sc;
    SceneFacts placed; placed.cull = true;
    CHECK(choose_parts(t, measured(-1.0), sc, slots(1u << 20)) == 3, "2^20 slots");
    CHECK(choose_parts(t, measured(-1.0), sc, slots((1u << 20) - 1)) == 1, "2^20 - 1 slots");
    CHECK(choose_parts(t, measured(-1.0), sc, slots(1u << 20, 1, 0)) == 1, "samples 0");
    DispatchFacts d = slots(1u << 20); d.phaseStats = 1;
    CHECK(choose_parts(t, measured(-1.0), sc, d) == 1, "phase_stats");
    CHECK(choose_parts(t, measured(150.0), placed, slots(8u << 20)) == 1, "placed objects, 150 tests per ray, 8 * 2^20 slots");
    CHECK(choose_parts(t, measured(150.0), placed, slots((8u << 20) - 1)) == 3, "the same, one slot fewer");
    CHECK(choose_parts(t, measured(149.9), placed, slots(8u << 20)) == 3, "the same, 149.9 tests per ray");
    CHECK(choose_parts(tuned("lanes", 2), measured(150.0), placed, slots(8u << 20)) == 2, "the same with lanes 2");
    CHECK(choose_parts(tuned("lanes", 3), measured(150.0), placed, slots(8u << 20)) == 3, "the same with lanes 3 given");
    CHECK(choose_parts(t, measured(153.3), sc, slots(2073600, 10)) == 3, "no placed objects, 153.3 tests per ray, 20 736 000 slots");
    CHECK(choose_parts(tuned("lanes", 4), measured(-1.0), sc, slots(1u << 20)) == 4, "lanes 4");
    CHECK(choose_parts(tuned("lanes", 1), measured(-1.0), sc, slots(1u << 20)) == 1, "lanes 1");
    CHECK(choose_parts(tuned("lanes_min_kslots", 64), measured(-1.0), sc, slots(65536)) == 3, "lanes_min_kslots 64");

    CHECK(part_grid_pct(t, 1, 2073600) == 100, "one part");
    CHECK(part_grid_pct(t, 3, 691200) == 40, "three parts of 691 200");
    CHECK(part_grid_pct(t, 3, 6912000) == 50, "three parts of 6 912 000");
    CHECK(part_grid_pct(t, 2, 1199999) == 40 && part_grid_pct(t, 2, 1200000) == 50, "1.2 M paths per part");
    CHECK(part_grid_pct(tuned("lane_grid_pct", 30), 3, 6912000) == 30, "lane_grid_pct 30");
    CHECK(part_grid_pct(tuned("lane_grid_pct", 30), 1, 6912000) == 100, "lane_grid_pct 30, one part");

    struct Case { uint32_t nSlots, nFrames; int nParts; uint32_t n[RT_MAX_LANES]; int gridPct; };
    const Case cases[] = {
        {2073600, 1, 3, {691200, 691200, 691200}, 40},
        {20736000, 10, 3, {6912000, 6912000, 6912000}, 50},
        {1000, 1, 3, {512, 256, 232}, 40},
        {300, 1, 3, {256, 44, 0}, 40},
        {2073600, 1, 1, {2073600}, 100},
        {2073600, 1, 4, {518400, 518400, 518400, 518400}, 40},
        {1u << 20, 1, 3, {349696, 349440, 349440}, 40},   // 4096 blocks of 256: 1366, 1365 and 1365
        {64 * 7 * 3, 3, 2, {768, 576}, 40},               // three frames: whole 256-slot blocks of all three
    };
    for (const Case& c : cases) {
        const PartSlices p = slice_parts(t, c.nSlots, c.nFrames, c.nParts);
        uint32_t at = 0;
        for (int l = 0; l < c.nParts; l++) {
            CHECK(p.n[l] == c.n[l], "%u slots x %u frames in %d: part %d has %u, want %u", c.nSlots, c.nFrames, c.nParts, l, p.n[l], c.n[l]);
            CHECK(p.begin[l] == at, "%u slots in %d: part %d begins at %u, not at %u", c.nSlots, c.nParts, l, p.begin[l], at);
            if (l + 1 < c.nParts && p.n[l + 1]) CHECK(p.n[l] % (256u * c.nFrames) == 0, "part %d of %u slots ends inside a block", l, c.nSlots);
            at += p.n[l];
        }
        CHECK(at == c.nSlots, "%u slots in %d: the parts cover %u", c.nSlots, c.nParts, at);
        CHECK(p.gridPct == c.gridPct, "%u slots in %d: grid share %d, want %d", c.nSlots, c.nParts, p.gridPct, c.gridPct);
    }
    for (uint32_t nSlots : {1u, 255u, 256u, 257u, 1023u, 65536u, 1000003u, 24u << 20})   // contiguous and complete whatever the size
        for (uint32_t nFrames : {1u, 3u, 10u})
            for (int nParts = 1; nParts <= RT_MAX_LANES; nParts++) {
                const PartSlices p = slice_parts(t, nSlots, nFrames, nParts);
                uint32_t at = 0;
                bool ok = true;
                for (int l = 0; l < nParts; l++) { ok = ok && p.begin[l] == at; at += p.n[l]; }
                CHECK(ok && at == nSlots, "%u slots x %u frames in %d parts", nSlots, nFrames, nParts);
            }
}

// ---------------------------------------------------------------- frames per dispatch
static void check_frames() {
    const Tuning t;
    const uint64_t hd = 1920 * 1080, uhd = 3840 * 2160;
    CHECK(frames_per_dispatch(t, hd, 100, -1) == 12, "1080p: twelve frames fit");
    CHECK(frames_per_dispatch(t, hd, 10, -1) == 10, "1080p: ten asked");
    CHECK(frames_per_dispatch(t, uhd, 10, -1) == 3, "4K");
    CHECK(frames_per_dispatch(tuned("frames_per_launch", 2), hd, 10, -1) == 2, "frames_per_launch 2");
    CHECK(frames_per_dispatch(t, hd, 10, 0) == 1, "heat map");
    CHECK(frames_per_dispatch(t, hd, 1, -1) == 1, "one frame");
    CHECK(frames_per_dispatch(t, 0, 10, -1) == 1, "no pixels");
    CHECK(frames_per_dispatch(t, 30u << 20, 10, -1) == 1, "a frame of more paths than the limit goes alone");
    CHECK(frames_per_dispatch(tuned("frames_max_mslots", 8), hd, 10, -1) == 4, "frames_max_mslots 8");
    CHECK(frames_per_dispatch(tuned("frames_max_mslots", 1000), 100, 100000000u, -1) == 8192000, "the limit counts whole 64-slot blocks per frame");
    CHECK(frames_per_dispatch(tuned("frames_max_mslots", 1000), 1u << 20, 5000, -1) == 1000, "1000 M paths are below the 30-bit slot ids");
    CHECK(frame_slots(1) == 64 && frame_slots(64) == 64 && frame_slots(65) == 128, "frame_slots");
    CHECK(dispatch_slots(100, 1) == 100 && dispatch_slots(100, 3) == 384, "dispatch_slots");
}

// ---------------------------------------------------------------- the kernel key
static bool same(const KernelKey& k, KernelFamily family, int stack, bool ovf, bool pix, bool stats, bool cull, int hot, int blocks) {
    return k.family == family && k.stack == stack && k.ovf == ovf && k.pix == pix && k.stats == stats && k.cull == cull && k.hot == hot && k.blocks == blocks;
}
static std::string show(const KernelKey& k) {
    char m[128];
    snprintf(m, sizeof m, "family %d <%d, ovf %d, pix %d, stats %d, cull %d, hot %d, blocks %d>", (int)k.family, k.stack, (int)k.ovf, (int)k.pix, (int)k.stats, (int)k.cull, k.hot, k.blocks);
    return m;
}
static SceneFacts scene(uint32_t depth, uint32_t hotNodes = 0, bool cull = false) { SceneFacts s; s.maxLeafDepth = depth; s.hotNodes = hotNodes; s.cull = cull; return s; }

// the tables themselves: HOT by (STACK, OVF) at six and at five work-groups per CU
static_assert(hot6(8, false) == 192 && hot6(16, false) == 136 && hot6(20, false) == 72 && hot6(24, false) == 0, "six work-groups per CU");
static_assert(hot6(8, true) == 0 && hot6(16, true) == 120 && hot6(24, true) == 0, "six work-groups per CU, overflow stacks");
static_assert(hot5(8, false) == 192 && hot5(16, false) == 192 && hot5(20, false) == 144 && hot5(24, false) == 80, "five work-groups per CU");
static_assert(hot5(8, true) == 0 && hot5(16, true) == 0 && hot5(24, true) == 0, "five work-groups per CU, overflow stacks");

static void check_kernel_key() {
    const KernelFamily PW = KernelFamily::trace_pw, FUSED = KernelFamily::render_fused;
    const DispatchFacts plain;
    // ---- stack buckets, no top-level table (hotNodes 0)
    struct Bucket { int cap; uint32_t depth; int stack; bool ovf; int fusedStack; bool fusedOvf; };
    const Bucket buckets[] = {
        {24, 1, 8, false, 8, false}, {24, 8, 8, false, 8, false}, {24, 9, 16, false, 16, false}, {24, 16, 16, false, 16, false},
        {24, 17, 20, false, 24, false}, {24, 20, 20, false, 24, false}, {24, 21, 24, false, 24, false}, {24, 24, 24, false, 24, false},
        {24, 25, 24, true, 24, true}, {24, 64, 24, true, 24, true},
        {16, 8, 8, false, 8, false}, {16, 16, 16, false, 16, false}, {16, 17, 16, true, 16, true}, {16, 40, 16, true, 16, true},
        {8, 8, 8, false, 8, false}, {8, 9, 8, true, 8, true}, {8, 30, 8, true, 8, true},
    };
    for (const Bucket& b : buckets)
        for (bool cull : {false, true}) {
            const Tuning t = tuned("lds_stack", b.cap);
            const KernelKey k = trace_kernel_key(t, scene(b.depth, 0, cull), plain);
            CHECK(same(k, PW, b.stack, b.ovf, false, false, cull, 0, 6), "multi-kernel, cap %d, depth %u: %s", b.cap, b.depth, show(k).c_str());
            const KernelKey f = fused_kernel_key(t, scene(b.depth, 192, cull), plain);
            CHECK(same(f, FUSED, b.fusedStack, b.fusedOvf, false, false, cull, 0, 0), "fused, cap %d, depth %u: %s", b.cap, b.depth, show(f).c_str());
        }
    // ---- the top-level table by hot_pairs
    struct Table { int hotPairs, cap; uint32_t depth; int stack; bool ovf; int hot, blocks; };
    const Table tables[] = {
        {2, 24, 8, 8, false, 192, 5}, {2, 24, 16, 16, false, 192, 5}, {2, 24, 20, 20, false, 144, 5}, {2, 24, 24, 24, false, 80, 5},
        {2, 16, 17, 16, true, 120, 6}, {2, 8, 9, 8, true, 0, 6},
        {1, 24, 8, 8, false, 192, 6}, {1, 24, 16, 16, false, 136, 6}, {1, 24, 20, 20, false, 72, 6}, {1, 24, 24, 24, false, 80, 5},
        {1, 16, 17, 16, true, 120, 6}, {1, 8, 9, 8, true, 0, 6},
        {0, 24, 8, 8, false, 0, 6}, {0, 24, 16, 16, false, 0, 6}, {0, 24, 20, 20, false, 0, 6}, {0, 24, 24, 24, false, 0, 6}, {0, 16, 17, 16, true, 0, 6},
        // deeper than 24 with a table wanted: 16 entries in LDS and the table beside six work-groups; without one, 24 and the overflow buffer
        {2, 24, 28, 16, true, 120, 6}, {1, 24, 28, 16, true, 120, 6}, {2, 24, 25, 16, true, 120, 6}, {0, 24, 28, 24, true, 0, 6},
    };
    for (const Table& c : tables) {
        Tuning t = tuned("hot_pairs", c.hotPairs);
        CHECK(set_tuning(t, "lds_stack", c.cap).error.empty(), "lds_stack %d", c.cap);
        const KernelKey k = trace_kernel_key(t, scene(c.depth, 192, true), plain);
        CHECK(same(k, PW, c.stack, c.ovf, false, false, true, c.hot, c.blocks), "hot_pairs %d, cap %d, depth %u: %s", c.hotPairs, c.cap, c.depth, show(k).c_str());
    }
    // ---- heat maps, per-ray counters, phase statistics or a scene without top levels: no table
    const Tuning t;
    DispatchFacts heat; heat.pixStats = true;
    DispatchFacts perRay; perRay.perRay = true;
    DispatchFacts phases; phases.phaseStats = 1;
    DispatchFacts both = heat; both.phaseStats = 2;
    for (uint32_t depth : {8u, 16u, 20u, 24u}) {
        const int stack = (int)depth;
        KernelKey k = trace_kernel_key(t, scene(depth, 192), heat);
        CHECK(same(k, PW, stack, false, true, false, false, 0, 6), "heat map, depth %u: %s", depth, show(k).c_str());
        k = trace_kernel_key(t, scene(depth, 192), perRay);
        CHECK(same(k, PW, stack, false, true, false, false, 0, 6), "per-ray counters, depth %u: %s", depth, show(k).c_str());
        k = trace_kernel_key(t, scene(depth, 192), phases);
        CHECK(same(k, PW, stack, false, true, true, false, 0, 6), "phase statistics, depth %u: %s", depth, show(k).c_str());
        k = trace_kernel_key(t, scene(depth, 192), both);
        CHECK(same(k, PW, stack, false, true, true, false, 0, 6), "phase statistics and a heat map, depth %u: %s", depth, show(k).c_str());
        k = trace_kernel_key(t, scene(depth, 0), plain);
        CHECK(same(k, PW, stack, false, false, false, false, 0, 6), "no top levels, depth %u: %s", depth, show(k).c_str());
    }
    KernelKey k = trace_kernel_key(t, scene(28, 192), heat);   // (and without a table a deep BVH keeps its 24 entries)
    CHECK(same(k, PW, 24, true, true, false, false, 0, 6), "heat map, depth 28: %s", show(k).c_str());
    k = trace_kernel_key(t, scene(28, 192), phases);
    CHECK(same(k, PW, 24, true, true, true, false, 0, 6), "phase statistics, depth 28: %s", show(k).c_str());
    k = trace_kernel_key(tuned("lds_stack", 16), scene(28, 192), plain);
    CHECK(same(k, PW, 16, true, false, false, false, 120, 6), "cap 16, depth 28: %s", show(k).c_str());
    // ---- an alpha map: the one traversal kernel that reads it, whatever trace_variant says
    SceneFacts alpha = scene(13, 192, true); alpha.mapFlags = RT_MAP_ALPHA | RT_MAP_BUMP;
    for (int variant : {0, 1}) {
        k = trace_kernel_key(tuned("trace_variant", variant), alpha, plain);
        CHECK(same(k, KernelFamily::trace_pw_alpha, 24, true, false, false, false, 0, 0), "alpha map, trace_variant %d: %s", variant, show(k).c_str());
        k = trace_kernel_key(tuned("trace_variant", variant), alpha, heat);
        CHECK(same(k, KernelFamily::trace_pw_alpha, 24, true, true, false, false, 0, 0), "alpha map, heat map, trace_variant %d: %s", variant, show(k).c_str());
    }
    SceneFacts bump = scene(13, 192); bump.mapFlags = RT_MAP_BUMP | RT_MAP_METALNESS;   // (the other maps are the shading kernel's business)
    k = trace_kernel_key(t, bump, plain);
    CHECK(same(k, PW, 16, false, false, false, false, 192, 5), "bump map: %s", show(k).c_str());
    // ---- trace_variant 0: one ray per lane, the whole stack in LDS
    const uint32_t v0[][2] = {{1, 8}, {8, 8}, {9, 16}, {16, 16}, {17, 24}, {24, 24}, {25, 32}, {32, 32}, {33, 48}, {48, 48}, {49, 64}, {64, 64}};
    for (const auto& c : v0) {
        k = trace_kernel_key(tuned("trace_variant", 0), scene(c[0], 192, true), heat);
        CHECK(same(k, KernelFamily::trace, (int)c[1], false, false, false, false, 0, 0), "trace_variant 0, depth %u: %s", c[0], show(k).c_str());
    }
    // ---- the fused pipeline: heat maps, and the one kernel of the scenes that bind a map
    k = fused_kernel_key(t, scene(17, 192, true), heat);
    CHECK(same(k, FUSED, 24, false, true, false, true, 0, 0), "fused heat map: %s", show(k).c_str());
    for (bool pix : {false, true}) {
        k = fused_kernel_key(tuned("lds_stack", 8), bump, pix ? heat : plain);
        CHECK(same(k, KernelFamily::render_fused_maps, 24, true, pix, false, true, 0, 0), "fused, maps: %s", show(k).c_str());
    }
}

// ---------------------------------------------------------------- launch shapes
static void check_trace_shape() {
    const Tuning t;
    const SceneFacts sc;
    const DispatchFacts d;
    TraceShape s = trace_shape(t, measured(70.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 12 && s.wSetup == 32, "long rays: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(t, measured(69.9), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 16 && s.wSetup == 16, "short rays: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(t, measured(-1.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 16 && s.wSetup == 16, "not measured: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(tuned("mk_refill", 20), measured(153.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 20 && s.wSetup == 32, "mk_refill 20: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(tuned("refill", 16), measured(153.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 16 && s.wSetup == 32, "refill 16: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(tuned("mk_w_setup", 16), measured(153.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 12 && s.wSetup == 16, "mk_w_setup 16: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(tuned("w_setup", 40), measured(10.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 16 && s.wSetup == 40, "w_setup 40: %u / %u", s.refillMk, s.wSetup);
    s = trace_shape(tuned("fused_below_box_tests", 100), measured(90.0), sc, d, 1u << 20, 1280);
    CHECK(s.refillMk == 16 && s.wSetup == 16, "long rays begin at fused_below_box_tests: %u / %u", s.refillMk, s.wSetup);
    // blocks: a block per 256 rays, at most the part's share of the resident work-groups, at least one
    struct Grid { uint32_t maxRays, resident; int gridPct; uint32_t blocks; };
    const Grid grids[] = {{1u << 20, 1280, 100, 1280}, {1u << 20, 1280, 40, 512}, {1u << 20, 1280, 50, 640}, {1000, 1280, 100, 4}, {1, 1280, 40, 1},
                          {1u << 20, 1536, 30, 460}, {1u << 20, 2, 40, 1}, {3u << 30, 1280, 100, 1280}};
    for (const Grid& g : grids) {
        DispatchFacts part; part.gridPct = g.gridPct;
        s = trace_shape(t, measured(-1.0), sc, part, g.maxRays, g.resident);
        CHECK(s.blocks == g.blocks, "%u rays, %u resident, %d %%: %u blocks, want %u", g.maxRays, g.resident, g.gridPct, s.blocks, g.blocks);
    }
    // wave times: phase_stats 1 every launch, 2 + k the k-th counted launch; never with the alpha kernel
    struct Times { int phaseStats; bool counted; uint64_t launches; bool want; };
    const Times times[] = {{0, true, 0, false}, {1, true, 5, true}, {1, false, 0, true}, {2, true, 0, true}, {2, true, 1, false}, {5, true, 3, true}, {5, true, 2, false}, {2, false, 0, false}};
    for (const Times& c : times) {
        DispatchFacts p; p.phaseStats = c.phaseStats; p.counted = c.counted; p.launches = c.launches;
        CHECK(trace_shape(t, measured(-1.0), sc, p, 1000, 1280).waveTimes == c.want, "phase_stats %d, launch %llu%s", c.phaseStats, (unsigned long long)c.launches, c.counted ? "" : " (not counted)");
        SceneFacts alpha; alpha.mapFlags = RT_MAP_ALPHA;
        CHECK(!trace_shape(t, measured(-1.0), alpha, p, 1000, 1280).waveTimes, "alpha map, phase_stats %d", c.phaseStats);
    }
}

static void check_fused_shape() {
    const Tuning t;
    const uint32_t resident = 1280;   // 5 120 resident waves
    FusedShape s = fused_shape(t, measured(70.0), slots(2073600), resident);
    CHECK(s.fastLanes == 40 && s.pixelRefill == 8, "long rays: fast lanes %u, pixel refill %u", s.fastLanes, s.pixelRefill);
    s = fused_shape(t, measured(69.9), slots(2073600), resident);
    CHECK(s.fastLanes == 24 && s.pixelRefill == 64, "short rays: fast lanes %u, pixel refill %u", s.fastLanes, s.pixelRefill);
    s = fused_shape(t, measured(-1.0), slots(2073600), resident);
    CHECK(s.fastLanes == 24 && s.pixelRefill == 64, "not measured: fast lanes %u, pixel refill %u", s.fastLanes, s.pixelRefill);
    s = fused_shape(tuned("fast_lanes", 50), measured(10.0), slots(2073600), resident);
    CHECK(s.fastLanes == 50, "fast_lanes 50: %u", s.fastLanes);
    s = fused_shape(tuned("fast_lanes", 0), measured(153.0), slots(2073600), resident);
    CHECK(s.fastLanes == 40, "fast_lanes 0: %u", s.fastLanes);
    CHECK(s.wSetup == 16 && s.wLeaf == 24 && !s.waveTimes, "weights %u / %u", s.wSetup, s.wLeaf);
    s = fused_shape(tuned("w_leaf", 40), measured(10.0), slots(2073600), resident);
    CHECK(s.wSetup == 16 && s.wLeaf == 40, "w_leaf 40: %u / %u", s.wSetup, s.wLeaf);
    s = fused_shape(tuned("mk_w_leaf", 40), measured(10.0), slots(2073600), resident);
    CHECK(s.wLeaf == 24, "mk_w_leaf 40 is the multi-kernel pipeline's: %u", s.wLeaf);
    DispatchFacts phases = slots(2073600); phases.phaseStats = 1;
    CHECK(fused_shape(t, measured(10.0), phases, resident).waveTimes, "phase_stats");
    // few blocks per wave: below 5, or below 8 when fewer than 2.5 segments per path were measured
    const uint32_t five = 5 * 5120 * 64, eight = 8 * 5120 * 64;
    CHECK(fused_shape(t, measured(10.0), slots(five), resident).pixelRefill == 64, "five blocks per wave");
    CHECK(fused_shape(t, measured(10.0), slots(five - 64), resident).pixelRefill == 8, "just below five blocks per wave");
    CHECK(fused_shape(t, measured(10.0, 2.5), slots(five), resident).pixelRefill == 64, "2.5 segments per path");
    CHECK(fused_shape(t, measured(10.0, 2.4), slots(five), resident).pixelRefill == 8, "2.4 segments per path, five blocks per wave");
    CHECK(fused_shape(t, measured(10.0, 2.4), slots(eight - 64), resident).pixelRefill == 8, "2.4 segments per path, just below eight");
    CHECK(fused_shape(t, measured(10.0, 2.4), slots(eight), resident).pixelRefill == 64, "2.4 segments per path, eight blocks per wave");
    CHECK(fused_shape(tuned("pixel_refill", 16), measured(153.0), slots(five), resident).pixelRefill == 16, "pixel_refill 16");
    // the 1/8-height 1080p tile: 4050 blocks of 64 for 5120 waves; 51 pixels give every wave one block
    s = fused_shape(t, measured(-1.0), slots(259200), resident);
    CHECK(s.pixelRefill == 8 && s.evenBelow == 1, "1/8 tile: pixel refill %u, even below %u", s.pixelRefill, s.evenBelow);
    CHECK(s.batchPixelsEven == 51 && s.g == 4 && s.batchPixels == 52, "1/8 tile: %u pixels, chunks of %u, %u pixels", s.batchPixelsEven, s.g, s.batchPixels);
    CHECK(s.nBatches == 4985 && s.blocks == 1247, "1/8 tile: %u blocks for the waves, %u work-groups", s.nBatches, s.blocks);
    // a block at a time (pixel refill 64): even blocks and scattered chunks up to two blocks per wave, whole blocks beyond
    s = fused_shape(tuned("pixel_refill", 64), measured(10.0), slots(2 * 5120 * 64), resident);
    CHECK(s.evenBelow == 2 && s.batchPixelsEven == 64 && s.g == 4 && s.nBatches == 10240 && s.blocks == 1280, "two blocks per wave: %u %u %u %u %u", s.evenBelow, s.batchPixelsEven, s.g, s.nBatches, s.blocks);
    s = fused_shape(tuned("pixel_refill", 64), measured(10.0), slots(2 * 5120 * 64 + 1), resident);
    CHECK(s.batchPixels == 64 && s.g == 0 && s.nBatches == 10241 && s.blocks == 1280, "beyond two blocks per wave: %u %u %u %u", s.batchPixels, s.g, s.nBatches, s.blocks);
    s = fused_shape(t, measured(10.0), slots(2073600), resident);
    CHECK(s.batchPixels == 64 && s.g == 0 && s.nBatches == 32400 && s.blocks == 1280, "a 1080p frame: %u %u %u %u", s.batchPixels, s.g, s.nBatches, s.blocks);
    // several frames: no scattered chunks; knobs by hand
    s = fused_shape(t, measured(-1.0), slots(25920, 10), resident);
    CHECK(s.g == 0, "ten frames: chunks of %u", s.g);
    s = fused_shape(tuned("scatter", 8), measured(10.0), slots(2073600), resident);
    CHECK(s.g == 8 && s.batchPixels == 64, "scatter 8: %u %u", s.g, s.batchPixels);
    s = fused_shape(tuned("scatter", 0), measured(-1.0), slots(259200), resident);
    CHECK(s.g == 0 && s.batchPixels == 51 && s.nBatches == 5083 && s.blocks == 1271, "scatter 0: %u %u %u %u", s.g, s.batchPixels, s.nBatches, s.blocks);
    s = fused_shape(tuned("batch_pixels", 32), measured(-1.0), slots(2073600), resident);
    CHECK(s.batchPixelsEven == 32 && s.batchPixels == 32, "batch_pixels 32: %u %u", s.batchPixelsEven, s.batchPixels);
    s = fused_shape(tuned("batch_fixed", 0), measured(-1.0), slots(259200), resident);
    CHECK(s.batchPixelsEven == 51, "batch_fixed 0: %u", s.batchPixelsEven);
    s = fused_shape(t, measured(-1.0), slots(1), resident);
    CHECK(s.nBatches == 1 && s.blocks == 1, "one pixel: %u %u", s.nBatches, s.blocks);
}

// ---------------------------------------------------------------- measured
static void check_measured() {
    Measured m;
    CHECK(m.boxPerRay < 0.0 && m.segPerPath < 0.0 && !m.snapPending, "nothing measured at first");
    fold_snapshot(m, RayCounters{20000000, 2000000, 200000, 800000, 200001});   // executed tests: boxTests - skippedBoxTests
    CHECK(m.boxPerRay == 90.0, "%.3f tests per ray", m.boxPerRay);
    CHECK(m.segPerPath == 800000.0 / 200001.0, "%.3f segments per path", m.segPerPath);
    CHECK(m.snapBox == 18000000 && m.snapRays == 200000 && m.snapSeg == 800000 && m.snapPaths == 200001, "the snapshot is kept");
    fold_snapshot(m, RayCounters{21000000, 2000000, 300000, 900000, 300001});   // 100 000 more rays and paths: too few to count
    CHECK(m.boxPerRay == 90.0 && m.segPerPath == 800000.0 / 200001.0, "a small difference changes nothing: %.3f", m.boxPerRay);
    CHECK(m.snapBox == 19000000 && m.snapRays == 300000 && m.snapSeg == 900000 && m.snapPaths == 300001, "... but the snapshot moves on");
    fold_snapshot(m, RayCounters{51000000, 2000000, 500000, 1200000, 500001});  // differences since the previous snapshot
    CHECK(m.boxPerRay == 150.0 && m.segPerPath == 1.5, "%.3f tests per ray, %.3f segments per path", m.boxPerRay, m.segPerPath);
    fold_snapshot(m, RayCounters{1000, 0, 400000, 100, 400000});                // counters that went back (reset): nothing measured from them
    CHECK(m.boxPerRay == 150.0 && m.segPerPath == 1.5 && m.snapRays == 400000, "after a reset");

    Measured p;
    fold_probe(p, RayCounters{1000, 100, 5000, 0, 0}, RayCounters{34000, 100, 6000, 0, 0});
    CHECK(p.boxPerRay < 0.0, "a probe of 1000 rays says nothing");
    fold_probe(p, RayCounters{1000, 100, 5000, 0, 0}, RayCounters{40038, 1100, 6001, 0, 0});
    CHECK(p.boxPerRay == 38.0, "the probe: %.3f tests per ray", p.boxPerRay);
    CHECK(p.snapRays == 0 && p.segPerPath < 0.0, "the probe leaves the snapshots alone");
}

// ---------------------------------------------------------------- tuning
static void check_tuning() {
    // every key with a range: accepted at both ends, refused just outside with its message
    struct Range { const char* key; int lo, hi; const char* message; };
    const Range ranges[] = {
        {"pipeline", -1, 1, "pipeline: -1 (auto), 0 or 1"},
        {"frames_max_mslots", 1, 1000, "frames_max_mslots: 1..1000 (millions of paths per multi-frame dispatch)"},
        {"frames_per_launch", 0, INT_MAX, "frames_per_launch >= 0"},
        {"fused_below_box_tests", 0, INT_MAX, "fused_below_box_tests >= 0"},
        {"fused_below_pixels", 0, INT_MAX, "fused_below_pixels >= 0"},
        {"trace_variant", 0, 1, "trace_variant: 0 or 1"},
        {"refill", 1, 64, "refill: 1..64"},
        {"hot_pairs", 0, 2, "hot_pairs: 0, 1 (six work-groups per CU) or 2 (five)"},
        {"mk_refill", 1, 64, "mk_refill: 1..64"},
        {"lds_stack", 8, 24, "lds_stack: 8, 16 or 24"},
        {"fast_lanes", 0, 65, "fast_lanes: 1..65 (0: back to the defaults)"},
        {"chunk", 1, 4096, "chunk: 1..4096"},
        {"w_setup", 1, 512, "w_setup: 1..512"},
        {"w_leaf", 1, 512, "w_leaf: 1..512"},
        {"mk_w_setup", 1, 512, "mk_w_setup: 1..512"},
        {"mk_w_leaf", 1, 512, "mk_w_leaf: 1..512"},
        {"fast_share", 0, 16, "fast_share: 0..16"},
        {"scatter", -1, 16, "scatter: -1 (auto), 0, 1, 2, 4, 8 or 16"},
        {"fused_maps", 0, 1, "fused_maps: 0 (map scenes take the multi-kernel pipeline) or 1 (they choose as usual)"},
        {"pixel_refill", 0, 64, "pixel_refill must be 0 (by ray length) .. 64"},
        {"batch_pixels", 0, 64, "batch_pixels must be 0 (auto) .. 64"},
        {"batch_fixed", 0, 4096, "batch_fixed out of range"},
        {"phase_stats", 0, INT_MAX, "phase_stats >= 0"},
        {"object_tree_min", 0, INT_MAX, "object_tree_min >= 0"},
        {"lanes", 0, 4, "lanes: 1..4 (parts of a multi-kernel dispatch, each on its own stream), 0 = automatic"},
        {"lane_grid_pct", 10, 100, "lane_grid_pct: 0 (by size) or 10..100"},
        {"lanes_min_kslots", 0, INT_MAX, "lanes_min_kslots >= 0"},
        {"blocks_per_cu", 0, 8, "blocks_per_cu: 0..8"},
    };
    for (const Range& r : ranges) {
        Tuning t;
        CHECK(set_tuning(t, r.key, r.lo).error.empty(), "%s %d", r.key, r.lo);
        CHECK(set_tuning(t, r.key, r.hi).error.empty(), "%s %d", r.key, r.hi);
        CHECK(set_tuning(t, r.key, r.lo - 1).error == r.message, "%s %d: \"%s\"", r.key, r.lo - 1, set_tuning(t, r.key, r.lo - 1).error.c_str());
        if (r.hi != INT_MAX) CHECK(set_tuning(t, r.key, r.hi + 1).error == r.message, "%s %d: \"%s\"", r.key, r.hi + 1, set_tuning(t, r.key, r.hi + 1).error.c_str());
        CHECK(!set_tuning(t, r.key, r.lo).rebuildEmitters, "%s does not touch the emitter list", r.key);
    }
    // the keys whose values are a list, between the ends
    struct Hole { const char* key; int value; bool ok; };
    const Hole holes[] = {{"lds_stack", 16, true}, {"lds_stack", 12, false}, {"lds_stack", 20, false}, {"scatter", 0, true}, {"scatter", 1, true}, {"scatter", 2, true},
                          {"scatter", 4, true}, {"scatter", 8, true}, {"scatter", 3, false}, {"scatter", 12, false}, {"lane_grid_pct", 0, true}, {"lane_grid_pct", 5, false},
                          {"lane_grid_pct", -1, false}};
    for (const Hole& h : holes) {
        Tuning t;
        CHECK(set_tuning(t, h.key, h.value).error.empty() == h.ok, "%s %d", h.key, h.value);
    }
    // the switches take any value
    for (const char* key : {"probe", "camera_reuse", "light_queries", "tile_slots", "mask_identity"})
        for (int value : {INT_MIN, -1, 0, 1, INT_MAX}) {
            Tuning t;
            const TuningChange ch = set_tuning(t, key, value);
            CHECK(ch.error.empty(), "%s %d", key, value);
            CHECK(ch.rebuildEmitters == (std::string(key) == "light_queries"), "%s: the emitter list follows light_queries only", key);
        }
    for (const char* key : {"", "lanes ", "Pipeline", "fused_below", "hot"}) {
        Tuning t;
        CHECK(set_tuning(t, key, 1).error == std::string("unknown tuning key ") + key, "\"%s\"", key);
    }
    // a refused value leaves the knob as it was
    Tuning t;
    CHECK(!set_tuning(t, "lanes", 5).error.empty() && t.lanes == 3 && !t.lanesSet, "lanes 5");
    CHECK(!set_tuning(t, "refill", 0).error.empty() && t.refill == 8 && t.refillMk == 16 && !t.refillMkSet, "refill 0");

    // what each key writes, the coupled writes among them
    const Tuning d;
    CHECK(d.pipeline == -1 && d.lanes == 3 && !d.lanesSet && d.lanesMinSlots == 1u << 20 && d.laneGridPct == 0 && d.fusedBelowPixels == 4000000 && d.fusedBelowBoxTests == 70, "defaults of the pipeline and the parts");
    CHECK(d.refill == 8 && d.refillMk == 16 && !d.refillMkSet && d.chunk == 256 && d.ldsStackCap == 24 && d.fastLanes == 32 && !d.fastLanesSet && d.fastShare == 10, "defaults of the traversal");
    CHECK(d.wSetup == 16 && d.wLeaf == 16 && !d.wSetupSet && !d.wLeafSet && d.wSetupFused == 16 && d.wLeafFused == 24, "default weights");
    CHECK(d.hotPairs == 2 && d.traceVariant == 1 && d.scatter == -1 && d.pixelRefill == 0 && d.batchPixels == 0 && d.batchFixed == 80 && d.fusedMaps == 0 && d.probe == 1, "defaults of the kernels and the fused pipeline");
    CHECK(d.framesPerLaunch == 0 && d.framesMaxSlots == 24ull << 20 && d.cameraReuse == 1 && d.lightQueries == 1 && d.objTreeMin == 48 && d.blocksPerCU == 0 && d.phaseStats == 0 && d.tileSlots == 1 && d.maskIdentity == 0, "the other defaults");
    t = tuned("refill", 5);
    CHECK(t.refill == 5 && t.refillMk == 5 && t.refillMkSet, "refill also sets the multi-kernel pipeline's");
    t = tuned("mk_refill", 5);
    CHECK(t.refill == 8 && t.refillMk == 5 && t.refillMkSet, "mk_refill");
    t = tuned("w_setup", 40);
    CHECK(t.wSetup == 40 && t.wSetupFused == 40 && t.wSetupSet && t.wLeaf == 16 && t.wLeafFused == 24 && !t.wLeafSet, "w_setup also writes the fused weight");
    t = tuned("w_leaf", 40);
    CHECK(t.wLeaf == 40 && t.wLeafFused == 40 && t.wLeafSet && t.wSetup == 16 && t.wSetupFused == 16 && !t.wSetupSet, "w_leaf also writes the fused weight");
    t = tuned("mk_w_setup", 40);
    CHECK(t.wSetup == 40 && t.wSetupFused == 16 && t.wSetupSet, "mk_w_setup");
    t = tuned("mk_w_leaf", 40);
    CHECK(t.wLeaf == 40 && t.wLeafFused == 24 && !t.wLeafSet, "mk_w_leaf");
    t = tuned("fast_lanes", 50);
    CHECK(t.fastLanes == 50 && t.fastLanesSet, "fast_lanes 50");
    CHECK(set_tuning(t, "fast_lanes", 0).error.empty() && t.fastLanes == 32 && !t.fastLanesSet, "fast_lanes 0 goes back to automatic");
    t = tuned("lanes", 2);
    CHECK(t.lanes == 2 && t.lanesSet, "lanes 2");
    CHECK(set_tuning(t, "lanes", 0).error.empty() && t.lanes == 3 && !t.lanesSet, "lanes 0 goes back to automatic");
    CHECK(tuned("frames_max_mslots", 2).framesMaxSlots == 2ull << 20, "frames_max_mslots counts millions of paths");
    CHECK(tuned("lanes_min_kslots", 5).lanesMinSlots == 5120, "lanes_min_kslots counts 1024 paths");
    CHECK(tuned("probe", 7).probe == 1 && tuned("probe", 0).probe == 0 && tuned("camera_reuse", 0).cameraReuse == 0 && tuned("light_queries", 0).lightQueries == 0, "switches");
    CHECK(tuned("tile_slots", 0).tileSlots == 0 && tuned("tile_slots", 5).tileSlots == 1 && tuned("mask_identity", 5).maskIdentity == 1, "switches");
    CHECK(tuned("pipeline", 0).pipeline == 0 && tuned("frames_per_launch", 4).framesPerLaunch == 4 && tuned("fused_below_box_tests", 50).fusedBelowBoxTests == 50 && tuned("fused_below_pixels", 9).fusedBelowPixels == 9, "plain knobs");
    CHECK(tuned("trace_variant", 0).traceVariant == 0 && tuned("hot_pairs", 1).hotPairs == 1 && tuned("lds_stack", 16).ldsStackCap == 16 && tuned("chunk", 64).chunk == 64 && tuned("fast_share", 3).fastShare == 3, "plain knobs");
    CHECK(tuned("scatter", 8).scatter == 8 && tuned("fused_maps", 1).fusedMaps == 1 && tuned("pixel_refill", 9).pixelRefill == 9 && tuned("batch_pixels", 33).batchPixels == 33 && tuned("batch_fixed", 7).batchFixed == 7, "plain knobs");
    CHECK(tuned("phase_stats", 3).phaseStats == 3 && tuned("object_tree_min", 0).objTreeMin == 0 && tuned("lane_grid_pct", 30).laneGridPct == 30 && tuned("blocks_per_cu", 2).blocksPerCU == 2, "plain knobs");
}

int main() {
    check_pipeline();
    check_probe();
    check_parts();
    check_frames();
    check_kernel_key();
    check_trace_shape();
    check_fused_shape();
    check_measured();
    check_tuning();
    return check_finish("launch plan ok");
}
