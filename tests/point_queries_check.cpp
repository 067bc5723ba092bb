// point_queries_check.cpp — what the point queries refuse (ray_tracer_amd/csrc/point_queries.h: check_point_query), in their order and
// with their messages, the block and byte arithmetic of a batch (point_shape), the stack choice (nearest_stack), the
// identity object's pruning record, and the units of the rule (include/rt_point_query.h: rt_point_triangle in each of its seven
// regions, on the plane, at a vertex, on zero-area triangles; rt_point_sphere; rt_nearest_exhaustive_host on a hand-made scene), on
// the CPU, built with plain g++ by tests/test_point_queries_host.py. No array is ever dereferenced by the checks: the addresses are
// made up. With a file name it reads 4x4 column-major float32 matrices from it and prints "prune <sMin> <padQ>" for each (the test
// compares them with numpy's singular values). Prints "point queries ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "point_queries.h"
#include "rt_point_query.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const P = at<float>(0x10000000u);
    float* const T = at<float>(0x30000000u);
    void* const OUT = at<void>(0x40000000u);
    for (const char* fn : {"rt_query_nearest", "rt_query_nearest_host"}) {
        const std::string f(fn);
        const RtPointBatch ok{P, T, 1000}, noLimit{P, nullptr, 1000};
        CHECK(check_point_query(fn, true, &ok, OUT).empty());
        CHECK(check_point_query(fn, true, &noLimit, OUT).empty());
        CHECK(check_point_query(fn, false, &ok, OUT) == f + " before rt_upload_scene");
        CHECK(check_point_query(fn, true, nullptr, OUT) == f + ": the batch is NULL");
        const RtPointBatch noP{nullptr, T, 5};
        CHECK(check_point_query(fn, true, &noP, OUT) == f + ": points and the output are required");
        CHECK(check_point_query(fn, true, &ok, nullptr) == f + ": points and the output are required");
        const RtPointBatch big{P, T, 1u << 30}, most{P, T, (1u << 30) - 1u}, huge{P, T, 0xffffffffu};
        CHECK(check_point_query(fn, true, &big, OUT) == f + ": a batch of 1073741824 points does not fit the 30 bits of a slot id");
        CHECK(check_point_query(fn, true, &huge, OUT) == f + ": a batch of 4294967295 points does not fit the 30 bits of a slot id");
        CHECK(check_point_query(fn, true, &most, OUT).empty());
        // n == 0 succeeds whatever the pointers are, but not without a scene or a batch
        const RtPointBatch none{nullptr, nullptr, 0};
        CHECK(check_point_query(fn, true, &none, nullptr).empty());
        CHECK(check_point_query(fn, false, &none, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, the pointers, the size
        const RtPointBatch bigNoP{nullptr, T, 1u << 30};
        CHECK(check_point_query(fn, false, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_point_query(fn, false, &bigNoP, nullptr) == f + " before rt_upload_scene");
        CHECK(check_point_query(fn, true, &bigNoP, OUT) == f + ": points and the output are required");
        CHECK(check_point_query(fn, true, &big, nullptr) == f + ": points and the output are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtNearest) == 48);
    const PointShape zero = point_shape(0, 256);
    CHECK(zero.blocks == 0 && zero.pointBytes == 0 && zero.limitBytes == 0 && zero.outBytes == 0);
    struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
    for (const Row& r : rows) {
        const PointShape s = point_shape(r.n, 256);
        CHECK(s.blocks == r.blocks);
        CHECK((uint64_t)s.blocks * 256 >= r.n && (uint64_t)(s.blocks - 1) * 256 < r.n);
        CHECK(s.pointBytes == (size_t)12 * r.n && s.limitBytes == (size_t)4 * r.n && s.outBytes == (size_t)48 * r.n);
    }
    CHECK(point_shape((1u << 30) - 1u, 256).outBytes == 51539607504ull);   // past 32 bits: size_t arithmetic

    std::string e;
    CHECK(nearest_stack("f", 0, &e) == 24 && nearest_stack("f", 24, &e) == 24 && nearest_stack("f", 25, &e) == 64 && nearest_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(nearest_stack("rt_query_nearest", 65, &e) == 0);
    CHECK(e == "rt_query_nearest: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_nearest_points");
}

bool same(float a, float b) { return std::fabs(a - b) <= 1e-6f; }

void rule_units() {
    const rt_vec3 a = rt_v3(0, 0, 0), b = rt_v3(1, 0, 0), c = rt_v3(0, 1, 0);
    struct Case { rt_vec3 q; float d2, u, v; } const cases[] = {
        {rt_v3(-1, -1, 0), 2.f, 0, 0},               // vertex a
        {rt_v3(2, -0.5f, 0), 1.25f, 1, 0},           // vertex b
        {rt_v3(-0.5f, 2, 0), 1.25f, 0, 1},           // vertex c
        {rt_v3(0.5f, -1, 0), 1.f, 0.5f, 0},          // edge ab
        {rt_v3(-1, 0.5f, 0), 1.f, 0, 0.5f},          // edge ac
        {rt_v3(1, 1, 0), 0.5f, 0.5f, 0.5f},          // edge bc
        {rt_v3(0.25f, 0.25f, 2), 4.f, 0.25f, 0.25f}  // face
    };
    for (const Case& k : cases) {
        float u = -1, v = -1;
        const float d2 = rt_point_triangle(k.q, a, b, c, &u, &v);
        CHECK(same(d2, k.d2) && same(u, k.u) && same(v, k.v));
        const rt_vec3 p = rt_bary_point(a, b, c, u, v);
        CHECK(d2 == rt_dist2(k.q, p));   // the distance of the very point it returns
    }
    float u, v;
    CHECK(rt_point_triangle(rt_v3(0.25f, 0.25f, 0), a, b, c, &u, &v) == 0.f && u == 0.25f && v == 0.25f);   // on the plane, inside: exactly 0
    CHECK(rt_point_triangle(b, a, b, c, &u, &v) == 0.f && u == 1.f && v == 0.f);                             // at a vertex
    CHECK(rt_point_triangle(c, a, b, c, &u, &v) == 0.f && u == 0.f && v == 1.f);
    const rt_vec3 x = rt_v3(0.3f, -1.7f, 2.9f), y = rt_v3(1.1f, 0.2f, -0.4f), z = rt_v3(-0.6f, 0.9f, 0.1f);
    for (const rt_vec3& corner : {x, y, z}) CHECK(rt_point_triangle(corner, x, y, z, &u, &v) == 0.f);
    // zero area: two equal corners are the segment, three the point; collinear corners the longest edge
    const rt_vec3 q = rt_v3(0.5f, 1, 0);
    CHECK(same(rt_point_triangle(q, a, a, b, &u, &v), 1.f) && std::isfinite(u) && std::isfinite(v));
    CHECK(same(rt_point_triangle(q, a, b, b, &u, &v), 1.f));
    CHECK(same(rt_point_triangle(q, b, a, b, &u, &v), 1.f));
    CHECK(same(rt_point_triangle(q, a, b, rt_v3(3, 0, 0), &u, &v), 1.f));
    CHECK(same(rt_point_triangle(rt_v3(2.5f, 1, 0), a, b, rt_v3(3, 0, 0), &u, &v), 1.f));   // beyond b, on the longest edge a-c
    CHECK(same(rt_point_triangle(q, a, a, a, &u, &v), 1.25f) && std::isfinite(u) && std::isfinite(v));
    const rt_vec3 pd = rt_bary_point(a, a, a, u, v);
    CHECK(pd.x == 0.f && pd.y == 0.f && pd.z == 0.f);

    rt_vec3 p;
    CHECK(same(rt_point_sphere(rt_v3(3, 0, 0), rt_v3(1, 0, 0), 0.5f, &p), 2.25f) && same(p.x, 1.5f) && p.y == 0.f && p.z == 0.f);
    CHECK(same(rt_point_sphere(rt_v3(1, 0.25f, 0), rt_v3(1, 0, 0), 0.5f, &p), 0.0625f) && same(p.y, 0.5f));   // inside: the distance to the surface
    CHECK(rt_point_sphere(rt_v3(1, 2, 3), rt_v3(1, 2, 3), 0.5f, &p) == 0.25f && p.x == 1.5f && p.y == 2.f && p.z == 3.f);
    CHECK(!rt_sphere_is_surface(0.f) && rt_sphere_is_surface(0.1f));

    bool search;
    CHECK(std::isinf(rt_nearest_start(false, 0.f, &search)) && search);
    CHECK(rt_nearest_start(true, 2.f, &search) == 4.f && search);
    for (float bad : {0.f, -0.f, -1.f, std::numeric_limits<float>::quiet_NaN()}) { rt_nearest_start(true, bad, &search); CHECK(!search); }

    // pruning: the box distance, and a threshold that never discards what it must keep
    CHECK(rt_point_box2(rt_v3(0.5f, 0.5f, 0.5f), a, rt_v3(1, 1, 1)) == 0.f);
    CHECK(rt_point_box2(rt_v3(3, 0.5f, -2), a, rt_v3(1, 1, 1)) == 8.f);
    CHECK(rt_nearest_threshold(4.f, 0.f, 1.f) >= 4.f && rt_nearest_threshold(4.f, 0.f, 1.f) < 4.0001f);
    CHECK(rt_nearest_threshold(4.f, 0.f, 0.5f) >= 16.f);
    CHECK(!(1e30f > rt_nearest_threshold(4.f, 0.f, 0.f)));                                   // a singular matrix discards nothing
    CHECK(!(1e30f > rt_nearest_threshold(0.f, 0.f, 0.f)));
    CHECK(!(1e30f > rt_nearest_threshold(4.f, std::numeric_limits<float>::infinity(), 1.f)));   // nor an unbounded object
    CHECK(!(1e30f > rt_nearest_threshold(std::numeric_limits<float>::infinity(), 0.f, 1.f)));   // nor a search without an answer yet
}

void prune_records() {
    const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const NearestPrune pi = nearest_prune(ident, true);
    CHECK(pi.sMin == 1.f && pi.padQ == 0.f);   // exactly
    float scaled[16];
    memcpy(scaled, ident, sizeof ident);
    scaled[0] = 2.f; scaled[5] = 0.5f; scaled[10] = 3.f; scaled[12] = 7.f;
    const NearestPrune ps = nearest_prune(scaled, false);
    CHECK(ps.sMin <= 0.5f && ps.sMin >= 0.5f * (1.f - 2e-6f) && ps.padQ > 0.f && ps.padQ < 1e-4f);
    float bad[16];
    memcpy(bad, ident, sizeof ident);
    bad[5] = std::numeric_limits<float>::quiet_NaN();
    CHECK(nearest_prune(bad, false).sMin == 0.f);
    float singular[16];
    memcpy(singular, ident, sizeof ident);
    singular[10] = 0.f;
    CHECK(nearest_prune(singular, false).sMin == 0.f);
}

// two triangles under a translated, scaled object and one sphere: the exhaustive loop against answers worked out by hand
void exhaustive() {
    TrianglePoint pts[4] = {};
    const float xyz[4][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}};
    for (int i = 0; i < 4; i++) memcpy(pts[i].position, xyz[i], 12);
    Triangle tris[2] = {};
    tris[0].v0 = 0; tris[0].v1 = 1; tris[0].v2 = 2;
    tris[1].v0 = 1; tris[1].v1 = 3; tris[1].v2 = 2;
    BVHNode nodes[3] = {};
    nodes[0].index = 1; nodes[0].triCount = 0;
    nodes[1].index = 0; nodes[1].triCount = 1;
    nodes[2].index = 1; nodes[2].triCount = 1;
    RenderObject obj = {};
    const float m[16] = {2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 10, 0, 0, 1};   // scale 2, then x + 10: the square [10, 12] x [0, 2] at z = 0
    memcpy(obj.transformMatrix, m, sizeof m);
    Sphere sph[2] = {};
    sph[1].position[0] = -5.f; sph[1].radius = 1.f;                           // slot 0 is zeroed: no surface
    RayMaterial mat = {};
    const RtSceneArrays s{sph, 2, &mat, 1, pts, 4, tris, 2, &obj, 1, nodes, 3};
    const float q[5][3] = {{11.5f, 1.5f, 3.f}, {0.f, 0.f, 0.f}, {11.f, 1.f, 0.f}, {13.f, 1.f, 0.f}, {13.f, 1.f, 0.f}};
    const float lim[5] = {100.f, 100.f, 100.f, 1.f, std::numeric_limits<float>::quiet_NaN()};
    RtNearest out[5];
    const RtPointBatch b{&q[0][0], lim, 5};
    CHECK(rt_nearest_exhaustive_host(&s, &b, out) == 0);
    CHECK(out[0].found == 1 && out[0].isSphere == 0 && out[0].objectIndex == 0 && out[0].triIndex == 1 && out[0].dst == 3.f);
    CHECK(out[0].point[0] == 11.5f && out[0].point[1] == 1.5f && out[0].point[2] == 0.f);
    CHECK(out[1].found == 1 && out[1].isSphere == 1 && out[1].objectIndex == 1 && out[1].dst == 4.f && out[1].point[0] == -4.f);
    CHECK(out[1].triIndex == 0 && out[1].uv[0] == 0.f && out[1].uv[1] == 0.f);
    CHECK(out[2].found == 1 && out[2].dst == 0.f && out[2].triIndex == 0);    // on the shared edge: the first of the equally near ones
    CHECK(out[3].found == 0 && out[3].dst == RT_MISS_DST);                    // dst 1 is not < the limit 1
    RtNearest none;
    memset(&none, 0, sizeof none);
    none.dst = RT_MISS_DST;
    CHECK(memcmp(&out[3], &none, sizeof none) == 0 && memcmp(&out[4], &none, sizeof none) == 0);
    const RtPointBatch noLimit{&q[3][0], nullptr, 1};
    CHECK(rt_nearest_exhaustive_host(&s, &noLimit, out) == 0 && out[0].found == 1 && out[0].dst == 1.f);
    const RtPointBatch empty{nullptr, nullptr, 0};
    CHECK(rt_nearest_exhaustive_host(&s, &empty, nullptr) == 0);
    CHECK(rt_nearest_exhaustive_host(nullptr, &b, out) == -1 && rt_nearest_exhaustive_host(&s, nullptr, out) == -1);
    CHECK(rt_nearest_exhaustive_host(&s, &b, nullptr) == -1);
}

}  // namespace

int main(int argc, char** argv) {
    refusals();
    arithmetic();
    rule_units();
    prune_records();
    exhaustive();
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("cannot open %s\n", argv[1]); return 1; }
        float m[16];
        while (fread(m, sizeof(float), 16, f) == 16) {
            const NearestPrune p = nearest_prune(m, false);
            printf("prune %.9g %.9g\n", (double)p.sMin, (double)p.padQ);
        }
        fclose(f);
    }
    return check_finish("point queries ok");
}
