// sample_map_check.cpp — the host logic of rt_build_sample_map and rt_render_sampled on the CPU (ray_tracer_amd/csrc/post_passes.h),
// built with plain g++ by tests/test_sample_map_host.py: every parameter refusal, the rule for the ctx-owned moments plane (none yet;
// of another size), and the refusal of a map with the debug heat maps. No plane is ever dereferenced: the addresses are made up.
// Prints "sample map ok".
#include <cstdio>
#include <limits>
#include <string>

#include "post_passes.h"
#include "check.h"

namespace {

bool has(const std::string& m, const char* part) { return m.find(part) != std::string::npos; }
const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();
const char* const FN = "rt_build_sample_map";

void parameter_checks() {
    const RtSampleMapParams ok{4u, 1u, 16u, 0.05f, 0.01f};
    const OwnedRows none{};
    const auto with = [&](uint32_t base, uint32_t mn, uint32_t mx, float tau, float floor) {
        return check_sample_map(8, 8, RtSampleMapParams{base, mn, mx, tau, floor}, true, none, FN);
    };
    CHECK(check_sample_map(8, 8, ok, true, none, FN).empty());
    CHECK(check_sample_map(0, 8, ok, true, none, FN) == "rt_build_sample_map: bad image geometry");
    CHECK(check_sample_map(8, 0, ok, true, none, "rt_build_sample_map_host") == "rt_build_sample_map_host: bad image geometry");
    CHECK(check_sample_map(1u << 15, 1u << 15, ok, true, none, FN) == "rt_build_sample_map: image too large");
    CHECK(with(4, 5, 16, 0.05f, 0.01f) == "rt_build_sample_map: minSamples must be <= baseSamples");
    CHECK(with(17, 1, 16, 0.05f, 0.01f) == "rt_build_sample_map: baseSamples must be <= maxSamples");
    CHECK(with(4, 4, 4, 0.05f, 0.01f).empty() && with(0, 0, 0, 0.05f, 0.01f).empty() && with(0, 0, 9, 0.05f, 0.01f).empty());
    for (float bad : {0.f, -0.05f, NaN, Inf, -Inf}) {
        CHECK(with(4, 1, 16, bad, 0.01f) == "rt_build_sample_map: targetRelError must be finite and > 0");
        CHECK(with(4, 1, 16, 0.05f, bad) == "rt_build_sample_map: luminanceFloor must be finite and > 0");
    }
    // the order: geometry, min <= base, base <= max, tau, the floor, then the moments plane
    const OwnedRows never{nullptr, false, RowsOf{}};
    CHECK(has(check_sample_map(0, 8, RtSampleMapParams{17u, 18u, 16u, 0.f, 0.f}, false, never, FN), "bad image geometry"));
    CHECK(has(check_sample_map(8, 8, RtSampleMapParams{17u, 18u, 16u, 0.f, 0.f}, false, never, FN), "minSamples"));
    CHECK(has(check_sample_map(8, 8, RtSampleMapParams{17u, 1u, 16u, 0.f, 0.f}, false, never, FN), "baseSamples"));
    CHECK(has(check_sample_map(8, 8, RtSampleMapParams{4u, 1u, 16u, 0.f, 0.f}, false, never, FN), "targetRelError"));
    CHECK(has(check_sample_map(8, 8, RtSampleMapParams{4u, 1u, 16u, 0.05f, 0.f}, false, never, FN), "luminanceFloor"));
    CHECK(has(check_sample_map(8, 8, ok, false, never, FN), "no ctx-owned moments"));
}

void owned_moments() {
    const RtSampleMapParams ok{4u, 1u, 16u, 0.05f, 0.01f};
    const void* const plane = (const void*)0x10000;
    // none yet: rt_temporal_accumulate never wrote a plane of the ctx's own
    CHECK(check_sample_map(8, 6, ok, false, OwnedRows{nullptr, false, RowsOf{}}, FN) ==
          "rt_build_sample_map: no ctx-owned moments: rt_temporal_accumulate was never called with d_moments = NULL");
    // the plane of the last call, of this very frame
    CHECK(check_sample_map(8, 6, ok, false, OwnedRows{plane, true, RowsOf{8, 6, 0, 1, 6}}, FN).empty());
    // of another size: another shape with the same pixel count, a larger and a smaller frame
    for (const RowsOf& r : {RowsOf{6, 8, 0, 1, 8}, RowsOf{16, 6, 0, 1, 6}, RowsOf{8, 5, 0, 1, 5}, RowsOf{4, 12, 0, 1, 12}}) {
        const std::string m = check_sample_map(8, 6, ok, false, OwnedRows{plane, true, r}, FN);
        CHECK(has(m, "rt_build_sample_map: the ctx moments") && has(m, "not the whole 8 x 6 frame"));
    }
    // a caller's plane is taken as it is: what the ctx owns does not matter
    CHECK(check_sample_map(8, 6, ok, true, OwnedRows{plane, true, RowsOf{6, 8, 0, 1, 8}}, FN).empty());
    CHECK(check_sample_map(8, 6, ok, true, OwnedRows{nullptr, false, RowsOf{}}, FN).empty());
}

void sampled_render() {
    RayTracerData td{};
    td.debug = -1;
    CHECK(check_sampled(td, true).empty() && check_sampled(td, false).empty());
    for (int dbg : {0, 1, 2}) {
        td.debug = dbg;
        CHECK(check_sampled(td, true) == "rt_render_sampled: the debug heat maps take no sample map");
        CHECK(check_sampled(td, false).empty());   // without a map it is rt_render_frames, heat maps included
    }
}

}  // namespace

int main() {
    parameter_checks();
    owned_moments();
    sampled_render();
    return check_finish("sample map ok");
}
