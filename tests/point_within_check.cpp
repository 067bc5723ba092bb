// point_within_check.cpp — what the radius point queries refuse (ray_tracer_amd/csrc/point_within.h: check_within_query), in their
// order and with their messages, the block and byte arithmetic of a batch (within_shape) at n = 0, 1, ... 2^30 - 1 and k = 0, 1, 8,
// the stack choice (within_stack) at depths 24, 25, 64 and 65, the part layout of the _host form for 65 points (stage_layout),
// the units of the rule (include/rt_point_within.h) and rt_within_exhaustive_host on a hand-made scene, on the CPU, built with
// plain g++ by tests/test_point_within_host.py. No array of a batch is ever dereferenced by the checks: the addresses are made
// up. Prints "point within ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "host_staging.h"
#include "point_within.h"
#include "rt_point_within.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const P = at<float>(0x10000000u);
    float* const T = at<float>(0x30000000u);
    void* const O = at<void>(0x40000000u);
    void* const C = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_within", "rt_query_within_host"}) {
        const std::string f(fn);
        const RtPointBatch ok{P, T, 1000}, noLimit{P, nullptr, 1000};
        for (uint32_t k : {0u, 1u, 8u}) {
            CHECK(check_within_query(fn, true, &ok, k, O, C).empty());
            CHECK(check_within_query(fn, true, &noLimit, k, O, C).empty());
        }
        CHECK(check_within_query(fn, true, &ok, 0, nullptr, C).empty());   // counts only
        CHECK(check_within_query(fn, false, &ok, 8, O, C) == f + " before rt_upload_scene");
        CHECK(check_within_query(fn, true, nullptr, 8, O, C) == f + ": the batch is NULL");
        const RtPointBatch noP{nullptr, T, 5};
        CHECK(check_within_query(fn, true, &noP, 8, O, C) == f + ": points and the output are required");
        CHECK(check_within_query(fn, true, &ok, 9, O, C) == f + ": k = 9 is above RT_WITHIN_MAX_K = 8");
        CHECK(check_within_query(fn, true, &ok, 0xffffffffu, O, C) == f + ": k = 4294967295 is above RT_WITHIN_MAX_K = 8");
        CHECK(check_within_query(fn, true, &ok, 8, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_within_query(fn, true, &ok, 0, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_within_query(fn, true, &ok, 1, nullptr, C) == f + ": counts and, with k > 0, the output are required");
        const RtPointBatch big{P, T, 1u << 30}, most{P, T, (1u << 30) - 1u}, huge{P, T, 0xffffffffu};
        CHECK(check_within_query(fn, true, &big, 8, O, C) == f + ": a batch of 1073741824 points does not fit the 30 bits of a slot id");
        CHECK(check_within_query(fn, true, &huge, 0, nullptr, C) == f + ": a batch of 4294967295 points does not fit the 30 bits of a slot id");
        CHECK(check_within_query(fn, true, &most, 8, O, C).empty());
        // n == 0 succeeds whatever the pointers and k are, but not without a scene or a batch
        const RtPointBatch none{nullptr, nullptr, 0};
        CHECK(check_within_query(fn, true, &none, 99, nullptr, nullptr).empty());
        CHECK(check_within_query(fn, false, &none, 99, nullptr, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, points, k, the outputs, the size
        const RtPointBatch bigNoP{nullptr, T, 1u << 30};
        CHECK(check_within_query(fn, false, nullptr, 9, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_within_query(fn, true, nullptr, 9, nullptr, nullptr) == f + ": the batch is NULL");
        CHECK(check_within_query(fn, true, &bigNoP, 9, nullptr, nullptr) == f + ": points and the output are required");
        CHECK(check_within_query(fn, true, &big, 9, nullptr, nullptr) == f + ": k = 9 is above RT_WITHIN_MAX_K = 8");
        CHECK(check_within_query(fn, true, &big, 8, nullptr, C) == f + ": counts and, with k > 0, the output are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtNearest) == 48 && RT_WITHIN_MAX_K == 8 && RT_HITS_WORDS == 3);
    for (uint32_t k : {0u, 1u, 8u}) {
        const WithinShape zero = within_shape(0, k, 256);
        CHECK(zero.searchBlocks == 0 && zero.resolveBlocks == 0 && zero.pointBytes == 0 && zero.limitBytes == 0 && zero.outBytes == 0 && zero.countBytes == 0 && zero.listBytes == 0);
        struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
        for (const Row& r : rows) {
            const WithinShape s = within_shape(r.n, k, 256);
            CHECK(s.searchBlocks == r.blocks);
            const uint64_t slots = (uint64_t)r.n * k;
            CHECK((uint64_t)s.resolveBlocks * 256 >= slots && (k == 0 ? s.resolveBlocks == 0 : (uint64_t)(s.resolveBlocks - 1) * 256 < slots));
            CHECK(s.pointBytes == (size_t)12 * r.n && s.limitBytes == (size_t)4 * r.n && s.countBytes == (size_t)4 * r.n);
            CHECK(s.outBytes == (size_t)48 * r.n * k);
            CHECK(s.listBytes == (size_t)r.blocks * 256 * 96);   // 8 entries of 3 words for every lane of the grid
        }
    }
    CHECK(within_shape((1u << 30) - 1u, 8, 256).outBytes == 412316860032ull);   // past 32 bits: size_t arithmetic
    CHECK(within_shape((1u << 30) - 1u, 8, 256).resolveBlocks == (1u << 25));
    CHECK(within_shape((1u << 30) - 1u, 8, 256).searchBlocks == (1u << 22));
    CHECK(within_shape((1u << 30) - 1u, 1, 256).outBytes == 51539607504ull);

    std::string e;
    CHECK(within_stack("f", 0, &e) == 24 && within_stack("f", 24, &e) == 24 && within_stack("f", 25, &e) == 64 && within_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(within_stack("rt_query_within", 65, &e) == 0);
    CHECK(e == "rt_query_within: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_points_within");
}

// points, maxDist, out, counts of the _host form for 65 points, by the one rule of host_staging.h
void staging() {
    struct Case { uint32_t k; bool limits; size_t offset[4], total; } const cases[] = {
        {8, true, {0, 1024, 1536, 26624}, 27136},    // 780, 260, 24960, 260 bytes, each from a multiple of 256
        {8, false, {0, 1024, 1024, 26112}, 26624},   // no maxDist: the part is absent, its offset the next one's
        {0, true, {0, 1024, 1536, 1536}, 2048},      // counts only: no records
        {1, true, {0, 1024, 1536, 4864}, 5376}};
    for (const Case& c : cases) {
        const WithinShape s = within_shape(65, c.k, 256);
        const size_t bytes[4] = {s.pointBytes, c.limits ? s.limitBytes : 0, s.outBytes, s.countBytes};
        CHECK(bytes[0] == 780 && bytes[3] == 260 && bytes[2] == (size_t)3120 * c.k);
        const StageLayout g = stage_layout(bytes, 4);
        CHECK(g.ok && g.bytes == c.total, "k %u: %zu", c.k, g.bytes);
        for (int p = 0; p < 4; p++) CHECK(g.offset[p] == c.offset[p], "k %u part %d: %zu", c.k, p, g.offset[p]);
    }
}

void rule_units() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(rt_within_member(0.f, 1.f) && rt_within_member(0.5f, inf) && !rt_within_member(1.f, 1.f) && !rt_within_member(2.f, 1.f));
    CHECK(!rt_within_member(nan, inf) && !rt_within_member(inf, inf) && !rt_within_member(0.f, 0.f));
    CHECK(rt_within_sphere_word(3) == rt_hits_sphere_word(3, false) && rt_hits_is_sphere(rt_within_sphere_word(3)) && rt_hits_sphere_index(rt_within_sphere_word(3)) == 3);
    CHECK(rt_within_triangle_word(7) == 7 && !rt_hits_is_sphere(rt_within_triangle_word(7)));
    // the key on {d2, primitive word, triangle}: spheres first, then the object, then the triangle
    CHECK(rt_hits_before(1.f, rt_within_sphere_word(5), 0, 1.f, rt_within_triangle_word(0), 0));
    CHECK(rt_hits_before(1.f, rt_within_sphere_word(1), 0, 1.f, rt_within_sphere_word(2), 0));
    CHECK(rt_hits_before(1.f, 0, 9, 1.f, 1, 2) && rt_hits_before(1.f, 1, 2, 1.f, 1, 9) && !rt_hits_before(1.f, 1, 2, 1.f, 1, 2));
    CHECK(rt_hits_before(0.5f, 9, 9, 1.f, rt_within_sphere_word(0), 0));
    const RtNearest none = rt_within_not_found();
    RtNearest zero;
    memset(&zero, 0, sizeof zero);
    zero.dst = RT_MISS_DST;
    CHECK(memcmp(&none, &zero, sizeof zero) == 0);
    // the records: a sphere, and a triangle in its face region
    const RtNearest s = rt_within_sphere_record(rt_v3(0, 0, 3), rt_v3(0, 0, 0), 1.f, 4, 4.f);
    CHECK(s.dst == 2.f && s.found == 1 && s.isSphere == 1 && s.objectIndex == 4 && s.triIndex == 0 && s.uv[0] == 0.f && s.uv[1] == 0.f);
    CHECK(s.point[0] == 0.f && s.point[1] == 0.f && s.point[2] == 1.f && s._pad[0] == 0 && s._pad[1] == 0);
    const RtNearest t = rt_within_triangle_record(rt_v3(0.25f, 0.25f, 3), rt_v3(0, 0, 0), rt_v3(1, 0, 0), rt_v3(0, 1, 0), 2, 11, 9.f);
    CHECK(t.dst == 3.f && t.found == 1 && t.isSphere == 0 && t.objectIndex == 2 && t.triIndex == 11 && t.uv[0] == 0.25f && t.uv[1] == 0.25f);
    CHECK(t.point[0] == 0.25f && t.point[1] == 0.25f && t.point[2] == 0.f && t._pad[0] == 0 && t._pad[1] == 0);
}

// A hand-made scene: one mesh of two triangles (the unit right triangle in z = 0, and a copy of it at z = -5) under an interior
// root with two leaves, placed twice by the identity, so the two objects' triangles coincide; a sphere of radius 1 about
// (0.25, 0.25, 3); and a zeroed sphere slot. From q = (0.25, 0.25, 1) the sphere and the two near triangles are all at distance
// exactly 1: the sphere is listed first, then the triangles in object order.
void hand_made_scene() {
    Sphere spheres[2];
    memset(spheres, 0, sizeof spheres);
    spheres[0].position[0] = 0.25f; spheres[0].position[1] = 0.25f; spheres[0].position[2] = 3.f; spheres[0].radius = 1.f;
    RayMaterial mats[1];
    memset(mats, 0, sizeof mats);
    TrianglePoint pts[6];
    memset(pts, 0, sizeof pts);
    const float xy[3][2] = {{0, 0}, {1, 0}, {0, 1}};
    for (int t = 0; t < 2; t++)
        for (int v = 0; v < 3; v++) {
            pts[3 * t + v].position[0] = xy[v][0]; pts[3 * t + v].position[1] = xy[v][1]; pts[3 * t + v].position[2] = t ? -5.f : 0.f;
        }
    Triangle tris[2];
    memset(tris, 0, sizeof tris);
    tris[0].v0 = 0; tris[0].v1 = 1; tris[0].v2 = 2;
    tris[1].v0 = 3; tris[1].v1 = 4; tris[1].v2 = 5;
    BVHNode nodes[3] = {{{0, 1}, {0, 1}, {-5, 0}, 1, 0}, {{0, 1}, {0, 1}, {0, 0}, 0, 1}, {{0, 1}, {0, 1}, {-5, -5}, 1, 1}};
    RenderObject objs[2];
    memset(objs, 0, sizeof objs);
    for (RenderObject& o : objs) { o.transformMatrix[0] = o.transformMatrix[5] = o.transformMatrix[10] = o.transformMatrix[15] = 1.f; o.bvhIndex = 0; }
    const RtSceneArrays s{spheres, 2, mats, 1, pts, 6, tris, 2, objs, 2, nodes, 3};

    const float q[3] = {0.25f, 0.25f, 1.f};
    RtNearest out[8];
    uint32_t counts[1] = {77};
    const RtPointBatch all{q, nullptr, 1};
    CHECK(rt_within_exhaustive_host(&s, &all, 8, out, counts) == 0 && counts[0] == 5);   // without a reach every surface is a member
    CHECK(out[0].isSphere == 1 && out[0].objectIndex == 0 && out[0].dst == 1.f && out[0].point[2] == 2.f && out[0].found == 1);
    for (uint32_t e = 1; e < 5; e++) {
        const RtNearest& r = out[e];
        CHECK(r.found == 1 && r.isSphere == 0 && r.objectIndex == (e - 1) % 2 && r.triIndex == (e - 1) / 2 && r.dst == (e < 3 ? 1.f : 6.f), "entry %u", e);
        CHECK(r.uv[0] == 0.25f && r.uv[1] == 0.25f && r.point[0] == 0.25f && r.point[1] == 0.25f && r.point[2] == (e < 3 ? 0.f : -5.f));
    }
    const RtNearest none = rt_within_not_found();
    for (uint32_t e = 5; e < 8; e++) CHECK(memcmp(&out[e], &none, sizeof none) == 0);

    // reaches: a constant bound, strict; the count is exact whatever k is, and a smaller k truncates the same list
    struct Reach { float R; uint32_t count; } const reaches[] = {{1.f, 0}, {1.5f, 3}, {6.f, 3}, {6.5f, 5}, {0.f, 0}, {-0.f, 0}, {-1.f, 0}, {std::numeric_limits<float>::quiet_NaN(), 0}};
    for (const Reach& rc : reaches) {
        const RtPointBatch lim{q, &rc.R, 1};
        RtNearest got[8];
        CHECK(rt_within_exhaustive_host(&s, &lim, 8, got, counts) == 0 && counts[0] == rc.count, "reach %g: %u", (double)rc.R, counts[0]);
        CHECK(memcmp(got, out, rc.count * sizeof(RtNearest)) == 0);
        for (uint32_t e = rc.count; e < 8; e++) CHECK(memcmp(&got[e], &none, sizeof none) == 0);
        for (uint32_t k : {0u, 1u, 2u}) {
            RtNearest fewer[2];
            counts[0] = 77;
            CHECK(rt_within_exhaustive_host(&s, &lim, k, k ? fewer : nullptr, counts) == 0 && counts[0] == rc.count);
            CHECK(memcmp(fewer, got, k * sizeof(RtNearest)) == 0);
        }
        // rt_query_nearest's rule under the same limit: found iff the count is not 0, and its record is the list's first
        RtNearest nearest;
        CHECK(rt_nearest_exhaustive_host(&s, &lim, &nearest) == 0);
        CHECK((nearest.found != 0) == (rc.count > 0) && memcmp(&nearest, &got[0], sizeof nearest) == 0);
    }

    // refusals of the loop itself
    CHECK(rt_within_exhaustive_host(nullptr, &all, 1, out, counts) == -1);
    CHECK(rt_within_exhaustive_host(&s, nullptr, 1, out, counts) == -1);
    CHECK(rt_within_exhaustive_host(&s, &all, 9, out, counts) == -1);
    CHECK(rt_within_exhaustive_host(&s, &all, 1, nullptr, counts) == -1);
    CHECK(rt_within_exhaustive_host(&s, &all, 1, out, nullptr) == -1);
    const RtPointBatch noPoints{nullptr, nullptr, 1}, big{q, nullptr, 1u << 30}, empty{nullptr, nullptr, 0};
    CHECK(rt_within_exhaustive_host(&s, &noPoints, 1, out, counts) == -1);
    CHECK(rt_within_exhaustive_host(&s, &big, 1, out, counts) == -1);
    CHECK(rt_within_exhaustive_host(&s, &empty, 8, nullptr, nullptr) == 0);
    CHECK(rt_within_exhaustive_host(&s, &empty, 9, nullptr, nullptr) == -1);
    nodes[2].index = 2;   // a leaf range past the triangles
    CHECK(rt_within_exhaustive_host(&s, &all, 1, out, counts) == -1);
    nodes[2].index = 1;
    objs[1].bvhIndex = 3;   // a root past the nodes
    CHECK(rt_within_exhaustive_host(&s, &all, 1, out, counts) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    staging();
    rule_units();
    hand_made_scene();
    return check_finish("point within ok");
}
