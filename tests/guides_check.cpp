// guides_check.cpp — what rt_render_guides refuses before anything is allocated (ray_tracer_amd/csrc/post_passes.h: check_guides, with
// check_tile and check_tile_slots, which rt_render and rt_render_aovs share), on the CPU, built with plain g++ by
// tests/test_guides_host.py: every message tests/test_guides.py asserts through the C ABI on the GPU, from the input that provokes
// it there, and their order. No plane is ever dereferenced: the addresses are made up. Prints "guides ok".
#include <cstdio>
#include <string>

#include "post_passes.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

const UploadedScene NONE{false, 0, 0}, SCENE{true, 3, 9};
RayTracerData counts(uint32_t spheres, uint32_t objects) {
    RayTracerData td{};
    td.sphereCount = spheres; td.objectCount = objects;
    return td;
}

// ---------------------------------------------------------------- the tile checks rt_render and rt_render_aovs share
void tile_checks() {
    const RayTracerData td = counts(3, 9);
    for (const char* fn : {"rt_render", "rt_render_aovs", "rt_render_guides"}) {
        const std::string f(fn);
        CHECK(check_tile(fn, td, 8, 8, 0, 1, 8, SCENE).empty());
        CHECK(check_tile(fn, td, 8, 8, 1, 3, 3, SCENE).empty());        // rows 1, 4, 7
        CHECK(check_tile(fn, td, 8, 8, 5, 1, 0, SCENE).empty());        // no rows: nothing to exceed
        CHECK(check_tile(fn, td, 0, 8, 0, 1, 1, SCENE) == f + ": bad image geometry");
        CHECK(check_tile(fn, td, 8, 0, 0, 1, 1, SCENE) == f + ": bad image geometry");
        CHECK(check_tile(fn, td, 8, 8, 0, 0, 1, SCENE) == f + ": bad image geometry");
        CHECK(check_tile(fn, td, 8, 8, 8, 1, 1, SCENE) == f + ": rows exceed the image");
        CHECK(check_tile(fn, td, 8, 8, 1, 4, 3, SCENE) == f + ": rows exceed the image");   // rows 1, 5, 9
        CHECK(check_tile(fn, td, 8, 8, 0xffffffffu, 0xffffffffu, 2, SCENE) == f + ": rows exceed the image");   // no 32-bit wrap
        CHECK(check_tile(fn, td, 8, 8, 0, 1, 8, NONE) == f + " before rt_upload_scene");
        CHECK(check_tile(fn, counts(4, 9), 8, 8, 0, 1, 8, SCENE) == "rayTraceParams.sphereCount exceeds the uploaded spheres");
        CHECK(check_tile(fn, counts(3, 10), 8, 8, 0, 1, 8, SCENE) == "rayTraceParams.objectCount exceeds the uploaded objects");
        CHECK(check_tile(fn, counts(0, 0), 8, 8, 0, 1, 8, SCENE).empty());   // fewer than uploaded is a dispatch with fewer
        // the order: geometry, rows, the scene, spheres, objects
        CHECK(check_tile(fn, counts(4, 10), 0, 8, 8, 1, 1, NONE) == f + ": bad image geometry");
        CHECK(check_tile(fn, counts(4, 10), 8, 8, 8, 1, 1, NONE) == f + ": rows exceed the image");
        CHECK(check_tile(fn, counts(4, 10), 8, 8, 0, 1, 8, NONE) == f + " before rt_upload_scene");
        CHECK(check_tile(fn, counts(4, 10), 8, 8, 0, 1, 8, SCENE) == "rayTraceParams.sphereCount exceeds the uploaded spheres");
        CHECK(check_tile_slots(fn, 1u << 15, 1u << 15) == f + ": tile too large (slot ids are 30 bits)");
        CHECK(check_tile_slots(fn, 1u << 15, (1u << 15) - 1u).empty());
        CHECK(check_tile_slots(fn, 8, 0).empty());
    }
}

// ---------------------------------------------------------------- rt_render_guides
void guide_checks() {
    const RayTracerData td = counts(3, 9);
    const auto with = [&](uint32_t maxBounces, const RtAovBuffers* g = nullptr, const RtAovBuffers* f = nullptr) {
        return check_guides(td, 8, 8, 0, 1, 8, maxBounces, g, f, SCENE);
    };
    for (uint32_t mb = 0; mb <= RT_GUIDE_MAX_BOUNCES; mb++) CHECK(with(mb).empty());
    CHECK(RT_GUIDE_MAX_BOUNCES == 8);
    CHECK(with(9) == "rt_render_guides: maxBounces must be 0..8");
    CHECK(with(0xffffffffu) == "rt_render_guides: maxBounces must be 0..8");
    // maxBounces first, then check_tile's refusals under this entry point's name, then the slot ids
    CHECK(check_guides(td, 0, 8, 0, 1, 8, 9, nullptr, nullptr, NONE) == "rt_render_guides: maxBounces must be 0..8");
    CHECK(check_guides(td, 0, 8, 0, 1, 8, 4, nullptr, nullptr, NONE) == "rt_render_guides: bad image geometry");
    CHECK(check_guides(td, 8, 8, 1, 4, 3, 4, nullptr, nullptr, NONE) == "rt_render_guides: rows exceed the image");
    CHECK(check_guides(td, 8, 8, 0, 1, 8, 4, nullptr, nullptr, NONE) == "rt_render_guides before rt_upload_scene");
    CHECK(check_guides(counts(4, 9), 8, 8, 0, 1, 8, 4, nullptr, nullptr, SCENE) == "rayTraceParams.sphereCount exceeds the uploaded spheres");
    CHECK(check_guides(counts(3, 10), 8, 8, 0, 1, 8, 4, nullptr, nullptr, SCENE) == "rayTraceParams.objectCount exceeds the uploaded objects");
    CHECK(check_guides(td, 1u << 15, 1u << 15, 0, 1, 1u << 15, 4, nullptr, nullptr, SCENE) == "rt_render_guides: tile too large (slot ids are 30 bits)");
    CHECK(check_guides(td, 1u << 15, 1u << 15, 0, 1, 1u << 15, 4, nullptr, nullptr, NONE) == "rt_render_guides before rt_upload_scene");

    // overlap: a plane is nRows * width records of 16 bytes; 8 x 8: 1024 bytes
    const uintptr_t G = 0x10000000u, F = 0x20000000u, B = 1024;
    const RtAovBuffers g{at<float>(G), at<float>(G + B), at<float>(G + 2 * B), at<float>(G + 3 * B), at<uint32_t>(G + 4 * B)};
    const RtAovBuffers f{at<float>(F), at<float>(F + B), at<float>(F + 2 * B), at<float>(F + 3 * B), at<uint32_t>(F + 4 * B)};
    CHECK(with(4, &g, &f).empty());
    CHECK(with(4, &g, nullptr).empty() && with(4, nullptr, &f).empty());
    CHECK(with(4, &g, &g) == "rt_render_guides: d_guides.normalDepth overlaps d_firstHit.normalDepth");
    const RtAovBuffers empty{};
    CHECK(with(4, &empty, &empty).empty() && with(4, &g, &empty).empty() && with(4, &empty, &g).empty());   // NULL fields are no planes
    const char* const names[5] = {"normalDepth", "position", "albedo", "rayDir", "ids"};
    for (int a = 0; a < 5; a++)
        for (int b = 0; b < 5; b++) {
            // first-hit plane b one record before the end of guide plane a, every other first-hit plane NULL
            void* planes[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            planes[b] = at<void>(G + (uintptr_t)a * B + B - 16);
            const RtAovBuffers one{(float*)planes[0], (float*)planes[1], (float*)planes[2], (float*)planes[3], (uint32_t*)planes[4]};
            const std::string m = with(4, &g, &one);
            if (a < 4) CHECK(m == std::string("rt_render_guides: d_guides.") + names[a] + " overlaps d_firstHit." + names[b]);
            else CHECK(m == std::string("rt_render_guides: d_guides.ids overlaps d_firstHit.") + names[b]);
            // ... and just past its end: the next guide plane's, or nobody's
            planes[b] = at<void>(G + 5 * B);
            const RtAovBuffers past{(float*)planes[0], (float*)planes[1], (float*)planes[2], (float*)planes[3], (uint32_t*)planes[4]};
            CHECK(with(4, &g, &past).empty());
        }
    // the planes of a tile are smaller: 2 rows of 8 pixels, 256 bytes
    const RtAovBuffers near{at<float>(G + 256), nullptr, nullptr, nullptr, nullptr};
    CHECK(check_guides(td, 8, 8, 0, 1, 8, 4, &g, &near, SCENE) == "rt_render_guides: d_guides.normalDepth overlaps d_firstHit.normalDepth");
    CHECK(check_guides(td, 8, 8, 0, 4, 2, 4, &g, &near, SCENE).empty());
    CHECK(check_guides(td, 8, 8, 0, 1, 0, 4, &g, &g, SCENE).empty());   // no rows: no byte to share
    // the overlap comes last
    CHECK(check_guides(td, 8, 8, 0, 1, 8, 9, &g, &g, SCENE) == "rt_render_guides: maxBounces must be 0..8");
    CHECK(check_guides(td, 8, 8, 0, 1, 8, 4, &g, &g, NONE) == "rt_render_guides before rt_upload_scene");
}

}  // namespace

int main() {
    tile_checks();
    guide_checks();
    return check_finish("guides ok");
}
