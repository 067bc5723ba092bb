// host_staging_check.cpp — the one rule for how the parts of a _host call lie in the ctx staging buffer
// (ray_tracer_amd/csrc/host_staging.h: stage_layout), on the CPU, built with plain g++ by tests/test_host_staging_host.py. The part
// lists are the ones rt_device.hip passes for each _host entry point, with and without the optional part; the byte counts
// themselves (12 n, sizeof(RtHit) n, ...) are pinned by the shape checks of ray_queries_check.cpp, radiance_queries_check.cpp and
// point_queries_check.cpp. Prints "host staging ok".
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "host_staging.h"
#include "rt_amd.h"
#include "check.h"

namespace {

static_assert(sizeof(size_t) >= 8, "the layout of 2^30 - 1 records is past 32 bits");

// the rule, for any list: the first offset 0; every offset and the total a multiple of 256; no part reaches into the next, and the
// next starts less than 256 bytes behind it; an absent part's offset is the next one's; the total ends less than 256 bytes behind
// the last part
StageLayout checked_layout(const size_t* bytes, int n) {
    const StageLayout g = stage_layout(bytes, n);
    CHECK(g.ok);
    if (!g.ok) return g;
    CHECK(n == 0 || g.offset[0] == 0);
    CHECK(g.bytes % 256 == 0);
    for (int k = 0; k < n; k++) {
        const size_t next = k + 1 < n ? g.offset[k + 1] : g.bytes;
        CHECK(g.offset[k] % 256 == 0);
        if (bytes[k]) CHECK(next >= g.offset[k] + bytes[k] && next < g.offset[k] + bytes[k] + 256);
        else CHECK(next == g.offset[k]);
    }
    if (n > 0) CHECK(g.bytes >= g.offset[n - 1] + bytes[n - 1] && g.bytes < g.offset[n - 1] + bytes[n - 1] + 256);
    return g;
}

const uint32_t NS[] = {0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, 1024u, 2299u, (1u << 30) - 1u};

// the same sums by division, not by masks
uint64_t up256(uint64_t b) { return (b + 255) / 256 * 256; }

void the_queries() {
    CHECK(sizeof(RtHit) == 60 && sizeof(RtNearest) == 48);
    for (const uint32_t n32 : NS) {
        const size_t n = n32;
        for (int opt = 0; opt < 2; opt++) {
            // rt_query_closest_host / rt_query_occluded_host: origins, dirs, the optional tmax, the hits or the flags
            for (const size_t rec : {sizeof(RtHit), (size_t)1}) {
                const size_t parts[4] = {12 * n, 12 * n, opt ? 4 * n : 0, rec * n};
                const StageLayout g = checked_layout(parts, 4);
                CHECK(g.offset[1] >= 12 * n && g.offset[2] >= g.offset[1] + 12 * n);
                CHECK(opt ? g.offset[3] >= g.offset[2] + 4 * n : g.offset[3] == g.offset[2]);
                CHECK(g.bytes >= g.offset[3] + rec * n && g.bytes < g.offset[3] + rec * n + 256);
                CHECK(g.bytes == 2 * up256(12 * (uint64_t)n) + (opt ? up256(4 * (uint64_t)n) : 0) + up256(rec * (uint64_t)n));
            }
            // rt_query_nearest_host: points, the optional limits, the records
            {
                const size_t parts[3] = {12 * n, opt ? 4 * n : 0, sizeof(RtNearest) * n};
                const StageLayout g = checked_layout(parts, 3);
                CHECK(g.offset[1] >= 12 * n && g.offset[1] < 12 * n + 256);
                CHECK(opt ? g.offset[2] >= g.offset[1] + 4 * n : g.offset[2] == g.offset[1]);
                CHECK(g.bytes >= g.offset[2] + 48 * n && g.bytes < g.offset[2] + 48 * n + 256);
                if (n == 0) CHECK(g.bytes == 0);
            }
            // rt_query_radiance_host: origins, dirs, the optional ids, the result (in/out when progressive: the same part)
            {
                const size_t parts[4] = {12 * n, 12 * n, opt ? 4 * n : 0, 16 * n};
                const StageLayout g = checked_layout(parts, 4);
                CHECK(g.offset[1] >= 12 * n && g.offset[2] >= g.offset[1] + 12 * n);
                CHECK(opt ? g.offset[3] >= g.offset[2] + 4 * n : g.offset[3] == g.offset[2]);
                CHECK(g.bytes >= g.offset[3] + 16 * n && g.bytes < g.offset[3] + 16 * n + 256);
            }
        }
    }
    // the pinned numbers: n = 65
    {
        const size_t ray[4] = {780, 780, 260, 65 * sizeof(RtHit)};   // limits, RtHit
        const StageLayout g = checked_layout(ray, 4);
        CHECK(ray[3] == 3900);
        CHECK(g.offset[0] == 0 && g.offset[1] == 1024 && g.offset[2] == 2048 && g.offset[3] == 2560 && g.bytes == 2560 + 4096);
        const size_t rad[4] = {780, 780, 260, 65 * 16};              // ids
        const StageLayout r = checked_layout(rad, 4);
        CHECK(r.offset[0] == 0 && r.offset[1] == 1024 && r.offset[2] == 2048 && r.offset[3] == 2560 && r.bytes == 2560 + 1280);
    }
    // n = 2^30 - 1: past 32 bits, exact
    {
        const size_t n = (1u << 30) - 1u;
        const size_t ray[4] = {12 * n, 12 * n, 4 * n, 60 * n};
        const StageLayout g = checked_layout(ray, 4);
        CHECK(g.offset[1] == 12884901888ull && g.offset[2] == 25769803776ull && g.offset[3] == 30064771072ull && g.bytes == 94489280512ull);
        const size_t rad[4] = {12 * n, 12 * n, 4 * n, 16 * n};
        CHECK(checked_layout(rad, 4).bytes == 47244640256ull);
        const size_t pts[3] = {12 * n, 4 * n, 48 * n};
        const StageLayout p = checked_layout(pts, 3);
        CHECK(p.bytes > 0xffffffffull && p.bytes == 68719476736ull);
    }
}

void the_planes() {
    // rt_temporal_accumulate_host: rgba, four AOV planes, the frame and the moments, 64 x 48 pixels of 16 bytes. A plane of a
    // multiple of 256 bytes packs as k * bytes.
    const size_t plane = 64 * 48 * 16;
    const size_t seven[7] = {plane, plane, plane, plane, plane, plane, plane};
    const StageLayout t = checked_layout(seven, 7);
    for (int k = 0; k < 7; k++) CHECK(t.offset[k] == (size_t)k * plane);
    CHECK(t.bytes == 7 * plane);
    // rt_denoise_host: five of them; an odd frame's planes are padded
    CHECK(checked_layout(seven, 5).bytes == 5 * plane);
    const size_t odd = 63 * 47 * 16;
    const size_t five[5] = {odd, odd, odd, odd, odd};
    const StageLayout d = checked_layout(five, 5);
    for (int k = 0; k < 5; k++) CHECK(d.offset[k] == (size_t)k * 47616);
    CHECK(d.bytes == 5 * 47616);
    // rt_build_sample_map_host: {n x 16, n x 4}
    for (const size_t n : {(size_t)64 * 48, (size_t)63 * 47, (size_t)1, (size_t)16384 * 16384}) {
        const size_t sm[2] = {n * 16, n * 4};
        const StageLayout s = checked_layout(sm, 2);
        CHECK(s.offset[1] == up256(n * 16) && s.bytes == up256(n * 16) + up256(n * 4));
    }
    const size_t sm[2] = {63 * 47 * 16, 63 * 47 * 4};
    const StageLayout s = checked_layout(sm, 2);
    CHECK(s.offset[1] == 47616 && s.bytes == 47616 + 12032);
    // rt_deinterleave_strips_host and rt_device_math_probe: an input and an output
    const size_t two[2] = {1920 * 1080 * 16, 1920 * 1080 * 16};
    CHECK(checked_layout(two, 2).offset[1] == 1920 * 1080 * 16);
    const size_t probe[2] = {3 * 32 * 4, 3 * 64 * 4};
    CHECK(checked_layout(probe, 2).offset[1] == 512 && checked_layout(probe, 2).bytes == 512 + 768);
}

void the_edges() {
    // all-absent lists and the empty list need nothing
    const size_t none[RT_STAGE_MAX_PARTS] = {};
    for (int n = 0; n <= (int)RT_STAGE_MAX_PARTS; n++) {
        const StageLayout g = checked_layout(none, n);
        CHECK(g.bytes == 0);
        for (int k = 0; k < n; k++) CHECK(g.offset[k] == 0);
    }
    CHECK(stage_layout(nullptr, 0).ok && stage_layout(nullptr, 0).bytes == 0);
    // an absent part in front, in the middle and at the end
    const size_t mixed[5] = {0, 1, 0, 257, 0};
    const StageLayout m = checked_layout(mixed, 5);
    CHECK(m.offset[0] == 0 && m.offset[1] == 0 && m.offset[2] == 256 && m.offset[3] == 256 && m.offset[4] == 768 && m.bytes == 768);
    // more parts than the rule holds are refused, not laid out
    CHECK(RT_STAGE_MAX_PARTS >= 7);
    const size_t many[RT_STAGE_MAX_PARTS + 1] = {1};
    CHECK(!stage_layout(many, RT_STAGE_MAX_PARTS + 1).ok && stage_layout(many, RT_STAGE_MAX_PARTS + 1).bytes == 0);
    CHECK(!stage_layout(many, -1).ok);
    CHECK(stage_layout(many, RT_STAGE_MAX_PARTS).ok);
}

}  // namespace

int main() {
    the_queries();
    the_planes();
    the_edges();
    return check_finish("host staging ok");
}
