// ray_queries_check.cpp — what the ray queries and the ambient-occlusion pass refuse (ray_tracer_amd/csrc/ray_queries.h: check_ray_query,
// check_ao), in their order and with their messages, and the slot and byte arithmetic of a batch (query_shape), on
// the CPU, built with plain g++ by tests/test_ray_queries_host.py. No array is ever dereferenced by the checks: the addresses are
// made up (where the arrays lie in the staging buffer of the _host forms: tests/host_staging_check.cpp). rt_ao_rays_host, which lives in the same host-only unit, runs on two real records. Prints "ray queries ok".
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "ray_queries.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

const char* const FNS[4] = {"rt_query_closest", "rt_query_occluded", "rt_query_closest_host", "rt_query_occluded_host"};

void query_checks() {
    float* const O = at<float>(0x10000000u);
    float* const D = at<float>(0x20000000u);
    float* const T = at<float>(0x30000000u);
    void* const OUT = at<void>(0x40000000u);
    for (const char* fn : FNS) {
        const std::string f(fn);
        const RtRayBatch ok{O, D, T, 1000}, noLimit{O, D, nullptr, 1000};
        CHECK(check_ray_query(fn, true, &ok, OUT).empty());
        CHECK(check_ray_query(fn, true, &noLimit, OUT).empty());
        // every refusal
        CHECK(check_ray_query(fn, false, &ok, OUT) == f + " before rt_upload_scene");
        CHECK(check_ray_query(fn, true, nullptr, OUT) == f + ": the batch is NULL");
        const RtRayBatch noO{nullptr, D, T, 5}, noD{O, nullptr, T, 5};
        CHECK(check_ray_query(fn, true, &noO, OUT) == f + ": origins, dirs and the output are required");
        CHECK(check_ray_query(fn, true, &noD, OUT) == f + ": origins, dirs and the output are required");
        CHECK(check_ray_query(fn, true, &ok, nullptr) == f + ": origins, dirs and the output are required");
        const RtRayBatch big{O, D, T, 1u << 30}, most{O, D, T, (1u << 30) - 1u}, huge{O, D, T, 0xffffffffu};
        CHECK(check_ray_query(fn, true, &big, OUT) == f + ": a batch of 1073741824 rays does not fit the 30 bits of a slot id");
        CHECK(check_ray_query(fn, true, &huge, OUT) == f + ": a batch of 4294967295 rays does not fit the 30 bits of a slot id");
        CHECK(check_ray_query(fn, true, &most, OUT).empty());
        // n == 0 succeeds whatever the pointers are, but not without a scene or a batch
        const RtRayBatch none{nullptr, nullptr, nullptr, 0};
        CHECK(check_ray_query(fn, true, &none, nullptr).empty());
        CHECK(check_ray_query(fn, false, &none, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, the pointers, the size
        const RtRayBatch bigNoO{nullptr, D, T, 1u << 30};
        CHECK(check_ray_query(fn, false, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_ray_query(fn, false, &bigNoO, nullptr) == f + " before rt_upload_scene");
        CHECK(check_ray_query(fn, true, &bigNoO, OUT) == f + ": origins, dirs and the output are required");
        CHECK(check_ray_query(fn, true, &big, nullptr) == f + ": origins, dirs and the output are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtHit) == 60);
    struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {255, 1}, {256, 1}, {257, 2}, {(1u << 30) - 1u, 1u << 22}};
    for (const Row& r : rows) {
        const QueryShape s = query_shape(r.n, 256);
        CHECK(s.slots == r.n && s.blocks == r.blocks);
        CHECK((uint64_t)s.blocks * 256 >= r.n && (uint64_t)(s.blocks - 1) * 256 < r.n);
        CHECK(s.vecBytes == (size_t)12 * r.n && s.tmaxBytes == (size_t)4 * r.n && s.queueBytes == (size_t)4 * r.n);
        CHECK(s.hitBytes == (size_t)60 * r.n && s.occludedBytes == (size_t)r.n);
        // every slot id fits a queue entry: slot * 4 + kind in 32 bits
        CHECK(((uint64_t)(r.n - 1) << 2 | 3u) <= 0xffffffffull);
    }
    CHECK(query_shape(64, 64).blocks == 1 && query_shape(65, 64).blocks == 2 && query_shape(63, 64).blocks == 1);
    const QueryShape top = query_shape((1u << 30) - 1u, 256);
    CHECK(top.hitBytes == 64424509380ull);   // past 32 bits: size_t arithmetic
}

void ao_checks() {
    const uintptr_t B = 0x10000000u;
    const RtAovBuffers planes{at<float>(B), at<float>(B + 0x1000), nullptr, nullptr, at<uint32_t>(B + 0x2000)};
    const RtAoParams ok{4, 0.3f, 1};
    const char* fn = "rt_render_ao";
    const std::string f(fn);
    CHECK(check_ao(fn, true, 64 * 48, ok, &planes, false, 0).empty());
    CHECK(check_ao(fn, true, 64 * 48, ok, nullptr, true, 64 * 48).empty());
    CHECK(check_ao(fn, true, 64 * 48, RtAoParams{1, 1e-30f, 0xffffffffu}, &planes, false, 0).empty());
    CHECK(check_ao(fn, true, 64 * 48, RtAoParams{64, 1e30f, 0}, &planes, false, 0).empty());
    CHECK(check_ao(fn, true, (1u << 30) - 1u, ok, &planes, false, 0).empty());
    // every refusal
    CHECK(check_ao(fn, false, 64, ok, &planes, false, 0) == f + " before rt_upload_scene");
    CHECK(check_ao(fn, true, 64, RtAoParams{0, 0.3f, 0}, &planes, false, 0) == f + ": samples must be 1..64");
    CHECK(check_ao(fn, true, 64, RtAoParams{65, 0.3f, 0}, &planes, false, 0) == f + ": samples must be 1..64");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float r : {0.f, -0.f, -1.f, inf, -inf, nan}) CHECK(check_ao(fn, true, 64, RtAoParams{4, r, 0}, &planes, false, 0) == f + ": radius must be finite and > 0");
    CHECK(check_ao(fn, true, 0, ok, &planes, false, 0) == f + ": no pixels");
    CHECK(check_ao(fn, true, 1u << 30, ok, &planes, false, 0) == f + ": 1073741824 pixels do not fit the 30 bits of a slot id");
    for (int k = 0; k < 3; k++) {
        RtAovBuffers p = planes;
        if (k == 0) p.position = nullptr; else if (k == 1) p.normalDepth = nullptr; else p.ids = nullptr;
        CHECK(check_ao(fn, true, 64, ok, &p, true, 64) == f + ": the planes need position, normalDepth and ids");
    }
    CHECK(check_ao(fn, true, 64, ok, nullptr, false, 64) == f + ": no ctx-owned AOV planes: rt_render_aovs was never called with d_out = NULL");
    CHECK(check_ao(fn, true, 64, ok, nullptr, true, 63) == f + ": the ctx-owned AOV planes hold 63 pixels, not 64");
    // the order: the scene, the parameters, the pixels, the planes
    CHECK(check_ao(fn, false, 0, RtAoParams{0, nan, 0}, nullptr, false, 0) == f + " before rt_upload_scene");
    CHECK(check_ao(fn, true, 0, RtAoParams{0, nan, 0}, nullptr, false, 0) == f + ": samples must be 1..64");
    CHECK(check_ao(fn, true, 0, RtAoParams{4, nan, 0}, nullptr, false, 0) == f + ": radius must be finite and > 0");
    CHECK(check_ao(fn, true, 0, ok, nullptr, false, 0) == f + ": no pixels");
    CHECK(check_ao(fn, true, 1u << 30, ok, nullptr, false, 0) == f + ": 1073741824 pixels do not fit the 30 bits of a slot id");
    RtAoParams d{};
    rt_ao_params_default(&d);
    CHECK(d.samples == 4 && d.radius == 0.5f && d.seed == 0);
}

// rt_ao_rays_host on two records: a hit on a floor facing -y (the Cornell floor's normal) and a miss
void ao_rays() {
    float position[8] = {0.25f, 0.5f, -0.125f, 1.f, 0.f, 0.f, 0.f, 0.f};
    float normalDepth[8] = {0.f, -1.f, 0.f, 2.f, 0.f, 0.f, 0.f, 99999999.f};
    uint32_t ids[8] = {3, 7, 1, 5, ~0u, ~0u, ~0u, 0};
    const RtAovBuffers planes{normalDepth, position, nullptr, nullptr, ids};
    const RtAoParams p{4, 0.3f, 9};
    float o[6], d[6], o2[6], d2[6];
    uint8_t v[2], v2[2];
    CHECK(rt_ao_rays_host(2, &planes, &p, 0, o, d, v) == 0);
    CHECK(v[0] == 1 && v[1] == 0);
    CHECK(o[0] == 0.25f && o[1] == 0.5f + -1.f * 0.00001f && o[2] == -0.125f);
    CHECK(std::fabs(std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - 1.f) < 1e-6f && d[1] <= 0.f);
    for (int k = 3; k < 6; k++) CHECK(o[k] == 0.f && d[k] == 0.f);
    CHECK(rt_ao_rays_host(2, &planes, &p, 1, o2, d2, v2) == 0);
    CHECK(o2[0] == o[0] && o2[1] == o[1] && o2[2] == o[2] && !(d2[0] == d[0] && d2[1] == d[1] && d2[2] == d[2]));
    const RtAoParams other{4, 0.3f, 10};
    CHECK(rt_ao_rays_host(2, &planes, &other, 0, o2, d2, v2) == 0);
    CHECK(!(d2[0] == d[0] && d2[1] == d[1] && d2[2] == d[2]));
    // refused: a sample the parameters do not have, bad parameters, no pixels, a missing plane or argument
    CHECK(rt_ao_rays_host(2, &planes, &p, 4, o, d, v) == -1);
    const RtAoParams bad{0, 0.3f, 0};
    CHECK(rt_ao_rays_host(2, &planes, &bad, 0, o, d, v) == -1);
    CHECK(rt_ao_rays_host(0, &planes, &p, 0, o, d, v) == -1);
    const RtAovBuffers noIds{normalDepth, position, nullptr, nullptr, nullptr};
    CHECK(rt_ao_rays_host(2, &noIds, &p, 0, o, d, v) == -1);
    CHECK(rt_ao_rays_host(2, nullptr, &p, 0, o, d, v) == -1 && rt_ao_rays_host(2, &planes, nullptr, 0, o, d, v) == -1);
    CHECK(rt_ao_rays_host(2, &planes, &p, 0, nullptr, d, v) == -1 && rt_ao_rays_host(2, &planes, &p, 0, o, d, nullptr) == -1);
}

}  // namespace

int main() {
    query_checks();
    arithmetic();
    ao_checks();
    ao_rays();
    return check_finish("ray queries ok");
}
