// tri_queries_check.cpp — what the triangle queries refuse (ray_tracer_amd/csrc/tri_queries.h: check_tris_query), in their order
// and with their messages, the block and byte arithmetic of a batch (tris_shape) at n = 0, 1, ... 2^30 - 1 and k = 0, 1, 8, the
// stack choice (tris_stack) at depths 24, 25, 64 and 65, the part layout of the _host form for 65 triangles (stage_layout), the
// rule (include/rt_tri_overlap.h) on hand-made cases in small integers and halves, where every fp32 operation is exact so that
// the rule must give the true answer, the pruning comparisons, and rt_tris_exhaustive_host on a hand-made scene, on the CPU,
// built with plain g++ by tests/test_triangles_host.py. No array of a batch is ever dereferenced by the checks: the addresses are
// made up. Prints "triangle queries ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "tri_queries.h"
#include "box_queries.h"
#include "host_staging.h"
#include "rt_tri_overlap.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const P = at<float>(0x10000000u);
    void* const O = at<void>(0x40000000u);
    void* const C = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_triangles", "rt_query_triangles_host"}) {
        const std::string f(fn);
        const RtTriangleBatch ok{P, 1000};
        for (uint32_t k : {0u, 1u, 8u}) CHECK(check_tris_query(fn, true, &ok, k, O, C).empty());
        CHECK(check_tris_query(fn, true, &ok, 0, nullptr, C).empty());   // counts only
        CHECK(check_tris_query(fn, false, &ok, 8, O, C) == f + " before rt_upload_scene");
        CHECK(check_tris_query(fn, true, nullptr, 8, O, C) == f + ": the batch is NULL");
        const RtTriangleBatch noCorners{nullptr, 5};
        CHECK(check_tris_query(fn, true, &noCorners, 8, O, C) == f + ": corners are required");
        CHECK(check_tris_query(fn, true, &ok, 9, O, C) == f + ": k = 9 is above RT_BOXES_MAX_K = 8");
        CHECK(check_tris_query(fn, true, &ok, 0xffffffffu, O, C) == f + ": k = 4294967295 is above RT_BOXES_MAX_K = 8");
        CHECK(check_tris_query(fn, true, &ok, 8, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_tris_query(fn, true, &ok, 0, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_tris_query(fn, true, &ok, 1, nullptr, C) == f + ": counts and, with k > 0, the output are required");
        const RtTriangleBatch big{P, 1u << 30}, most{P, (1u << 30) - 1u}, huge{P, 0xffffffffu};
        CHECK(check_tris_query(fn, true, &big, 8, O, C) == f + ": a batch of 1073741824 triangles does not fit the 30 bits of a slot id");
        CHECK(check_tris_query(fn, true, &huge, 0, nullptr, C) == f + ": a batch of 4294967295 triangles does not fit the 30 bits of a slot id");
        CHECK(check_tris_query(fn, true, &most, 8, O, C).empty());
        // n == 0 succeeds whatever the pointers and k are, but not without a scene or a batch
        const RtTriangleBatch none{nullptr, 0};
        CHECK(check_tris_query(fn, true, &none, 99, nullptr, nullptr).empty());
        CHECK(check_tris_query(fn, false, &none, 99, nullptr, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, the corners, k, the outputs, the size
        const RtTriangleBatch bigNoCorners{nullptr, 1u << 30};
        CHECK(check_tris_query(fn, false, nullptr, 9, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_tris_query(fn, true, nullptr, 9, nullptr, nullptr) == f + ": the batch is NULL");
        CHECK(check_tris_query(fn, true, &bigNoCorners, 9, nullptr, nullptr) == f + ": corners are required");
        CHECK(check_tris_query(fn, true, &big, 9, nullptr, nullptr) == f + ": k = 9 is above RT_BOXES_MAX_K = 8");
        CHECK(check_tris_query(fn, true, &big, 8, nullptr, C) == f + ": counts and, with k > 0, the output are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtOverlap) == 16 && RT_BOXES_MAX_K == 8 && RT_BOX_WORDS == 2 && sizeof(RtTriangleBatch) == 16);
    for (uint32_t k : {0u, 1u, 8u}) {
        const TrisShape zero = tris_shape(0, k, 256);
        CHECK(zero.blocks == 0 && zero.cornerBytes == 0 && zero.outBytes == 0 && zero.countBytes == 0 && zero.listBytes == 0);
        struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
        for (const Row& r : rows) {
            const TrisShape s = tris_shape(r.n, k, 256);
            CHECK(s.blocks == r.blocks);
            CHECK(s.cornerBytes == (size_t)36 * r.n && s.countBytes == (size_t)4 * r.n);
            CHECK(s.outBytes == (size_t)16 * r.n * k);
            CHECK(s.listBytes == (size_t)r.blocks * 256 * 64);   // 8 entries of 2 words for every lane of the grid
            CHECK(s.listBytes == boxes_shape(r.n, k, 256).listBytes);   // the buffer is the box queries'
        }
    }
    CHECK(tris_shape((1u << 30) - 1u, 8, 256).outBytes == 137438953344ull);   // past 32 bits: size_t arithmetic
    CHECK(tris_shape((1u << 30) - 1u, 8, 256).cornerBytes == 38654705628ull);

    std::string e;
    CHECK(tris_stack("f", 0, &e) == 24 && tris_stack("f", 24, &e) == 24 && tris_stack("f", 25, &e) == 64 && tris_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(tris_stack("rt_query_triangles", 65, &e) == 0);
    CHECK(e == "rt_query_triangles: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_tris_overlap");
}

// corners, out, counts of the _host form for 65 triangles, by the one rule of host_staging.h
void staging() {
    struct Case { uint32_t k; size_t offset[3], total; } const cases[] = {
        {8, {0, 2560, 11008}, 11520},   // 2340, 8320, 260 bytes, each from a multiple of 256
        {0, {0, 2560, 2560}, 3072},     // counts only: no records
        {1, {0, 2560, 3840}, 4352}};
    for (const Case& c : cases) {
        const TrisShape s = tris_shape(65, c.k, 256);
        const size_t bytes[3] = {s.cornerBytes, s.outBytes, s.countBytes};
        CHECK(bytes[0] == 2340 && bytes[2] == 260 && bytes[1] == (size_t)1040 * c.k);
        const StageLayout g = stage_layout(bytes, 3);
        CHECK(g.ok && g.bytes == c.total, "k %u: %zu", c.k, g.bytes);
        for (int p = 0; p < 3; p++) CHECK(g.offset[p] == c.offset[p], "k %u part %d: %zu", c.k, p, g.offset[p]);
    }
}

struct V { float x, y, z; };
rt_vec3 v3(const V& v) { return rt_v3(v.x, v.y, v.z); }
struct PairCase { const char* what; V a, b, c; bool touch; };

// the verdict under every order of the query's and the triangle's corners; `swap`: and with the roles exchanged (the geometric
// truth is symmetric, and on these numbers the rule is exact)
void pair_all_orders(const V q[3], const PairCase& c, bool swap) {
    static const int perm[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
    const V t[3] = {c.a, c.b, c.c};
    for (const auto& pq : perm)
        for (const auto& pt : perm) {
            CHECK(rt_tri_triangle(v3(q[pq[0]]), v3(q[pq[1]]), v3(q[pq[2]]), v3(t[pt[0]]), v3(t[pt[1]]), v3(t[pt[2]])) == c.touch, "%s", c.what);
            if (swap) CHECK(rt_tri_triangle(v3(t[pt[0]]), v3(t[pt[1]]), v3(t[pt[2]]), v3(q[pq[0]]), v3(q[pq[1]]), v3(q[pq[2]])) == c.touch, "%s (roles exchanged)", c.what);
        }
}

// the first eleven axes alone (nQ, nT, eQi x eTj): what the test would be without the six in-plane axes
bool eleven_axes(rt_vec3 p, rt_vec3 q, rt_vec3 r, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    const RtTriQuery t = rt_tri_prepare(p, q, r);
    if (!rt_box_triangle_stage1(t.lo, t.hi, a, b, c)) return false;
    const rt_vec3 A = rt_sub(a, t.m), B = rt_sub(b, t.m), C = rt_sub(c, t.m);
    const rt_vec3 f0 = rt_sub(B, A), f1 = rt_sub(C, B), f2 = rt_sub(A, C);
    if (rt_tri_known_out(t.nLo, t.nHi, t.n, A, B, C) || rt_tri_axis_out(rt_cross(f0, f1), t.P, t.Q, t.R, A, B, C)) return false;
    return !(rt_tri_edge_out(&t, t.e0, f0, f1, f2, A, B, C) || rt_tri_edge_out(&t, t.e1, f0, f1, f2, A, B, C) || rt_tri_edge_out(&t, t.e2, f0, f1, f2, A, B, C));
}

void rule_table() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the query (0,0,0) (4,0,0) (0,4,0): small integers and halves, every operation of the rule is exact
    const V Q0[3] = {{0, 0, 0}, {4, 0, 0}, {0, 4, 0}};
    const PairCase flat[] = {
        {"a shared corner", {0, 0, 0}, {-4, 0, 0}, {0, -4, 4}, true},
        {"a shared edge", {0, 0, 0}, {4, 0, 0}, {0, -4, 4}, true},
        {"the same triangle", {0, 0, 0}, {4, 0, 0}, {0, 4, 0}, true},
        {"an edge crossing an edge in one plane", {2, -2, 0}, {2, 1, 0}, {6, -2, 0}, true},
        {"coplanar, touching the hypotenuse with a corner", {2, 2, 0}, {6, 2, 0}, {2, 6, 0}, true},
        {"coplanar, beyond the hypotenuse: only an in-plane edge normal separates", {3, 3, 0}, {6, 3, 0}, {3, 6, 0}, false},
        {"coplanar, beyond the hypotenuse by half a unit", {2.5f, 2, 0}, {6, 2, 0}, {2.5f, 6, 0}, false},
        {"coplanar, inside the query", {0.5f, 0.5f, 0}, {1.5f, 0.5f, 0}, {0.5f, 1.5f, 0}, true},
        {"coplanar, around the query", {-8, -8, 0}, {16, -8, 0}, {-8, 16, 0}, true},
        {"parallel planes one unit apart", {0, 0, 1}, {4, 0, 1}, {0, 4, 1}, false},
        {"an edge piercing the face", {1, 1, -1}, {1, 1, 1}, {5, 5, 1}, true},
        {"an edge passing the face outside the hypotenuse", {3, 3, -1}, {3, 3, 1}, {7, 7, 1}, false},
        {"a corner resting on the face", {1, 1, 0}, {1, 1, 4}, {2, 1, 4}, true},
        {"a corner half a unit over the face", {1, 1, 0.5f}, {1, 1, 4}, {2, 1, 4}, false},
        {"an edge resting on the face", {1, 1, 0}, {2, 1, 0}, {1, 1, 4}, true},
        {"a corner resting on an edge", {2, 0, 0}, {2, -4, 4}, {3, -4, 4}, true},
        {"crossing planes, the triangle beside the query", {5, -1, -1}, {5, 1, 1}, {5, 3, -1}, false},
        {"crossing planes, through the query", {1, -1, -1}, {1, 1, 1}, {1, 3, -1}, true},
    };
    for (const PairCase& c : flat) pair_all_orders(Q0, c, true);
    // the coplanar pair that only the six in-plane axes separate: the first eleven call it touching
    CHECK(eleven_axes(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), rt_v3(3, 3, 0), rt_v3(6, 3, 0), rt_v3(3, 6, 0)));
    CHECK(!rt_tri_triangle(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), rt_v3(3, 3, 0), rt_v3(6, 3, 0), rt_v3(3, 6, 0)));

    // a tilted query (0,0,0) (4,0,4) (0,4,4), plane x + y - z = 0: pairs whose boxes overlap and only a normal separates
    const V Q1[3] = {{0, 0, 0}, {4, 0, 4}, {0, 4, 4}};
    const PairCase tilted[] = {
        {"parallel tilted planes one unit apart", {0, 0, -1}, {4, 0, 3}, {0, 4, 3}, false},
        {"under the tilted plane", {1, 1, 0}, {2, 1, 0}, {1, 2, 0}, false},
        {"touching the tilted plane with a corner", {1, 1, 2}, {2, 1, 0}, {1, 2, 0}, true},
        {"through the tilted plane", {1, 1, 3}, {2, 1, 0}, {1, 2, 0}, true},
    };
    for (const PairCase& c : tilted) pair_all_orders(Q1, c, true);

    // a query with two equal corners is its segment: against the triangle (2,0,-2) (2,4,-2) (2,2,2) in the plane x = 2
    const V T2[3] = {{2, 0, -2}, {2, 4, -2}, {2, 2, 2}};
    struct SegCase { const char* what; V s0, s1; bool touch; } const segs[] = {
        {"segment through the face", {0, 2, 0}, {4, 2, 0}, true},
        {"segment ending on the face", {0, 2, 0}, {2, 2, 0}, true},
        {"segment ending before the face", {0, 2, 0}, {1, 2, 0}, false},
        {"segment over the triangle's box", {0, 2, 3}, {4, 2, 3}, false},
        {"segment beside the slanted edge: only an edge-cross axis separates", {0, 3.5f, 1}, {4, 3.5f, 1}, false},
        {"segment through the slanted edge", {0, 2.5f, 1}, {4, 2.5f, 1}, true},
    };
    for (const SegCase& c : segs) {
        const rt_vec3 s0 = v3(c.s0), s1 = v3(c.s1), a = v3(T2[0]), b = v3(T2[1]), cc = v3(T2[2]);
        CHECK(rt_tri_triangle(s0, s0, s1, a, b, cc) == c.touch, "%s (p == q)", c.what);
        CHECK(rt_tri_triangle(s0, s1, s1, b, cc, a) == c.touch, "%s (q == r)", c.what);
        CHECK(rt_tri_triangle(s1, s0, s1, cc, a, b) == c.touch, "%s (p == r)", c.what);
    }
    // ... and with three its point
    struct PtCase { const char* what; V p; bool touch; } const pts[] = {
        {"point inside the face", {2, 2, 0}, true},
        {"point on a corner", {2, 2, 2}, true},
        {"point on the slanted edge", {2, 2.5f, 1}, true},
        {"point in the plane, beside the slanted edge: only nT x eT separates", {2, 3.5f, 1}, false},
        {"point off the plane", {3, 2, 0}, false},
    };
    for (const PtCase& c : pts) CHECK(rt_tri_triangle(v3(c.p), v3(c.p), v3(c.p), v3(T2[0]), v3(T2[1]), v3(T2[2])) == c.touch, "%s", c.what);

    // NaN separates nothing: a scene triangle of NaN corners is a member of every valid query; one finite axis that separates does
    const rt_vec3 N = rt_v3(nan, nan, nan);
    CHECK(rt_tri_triangle(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), N, N, N));
    CHECK(rt_tri_triangle(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), rt_v3(nan, 1, 0), rt_v3(1, 1, 0), rt_v3(1, 2, 0)));
    CHECK(!rt_tri_triangle(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), rt_v3(nan, 0, 5), rt_v3(1, 0, 5), rt_v3(0, 1, 5)));
    CHECK(!rt_tri_triangle(v3(Q1[0]), v3(Q1[1]), v3(Q1[2]), rt_v3(nan, 1, 0), rt_v3(2, 1, 0), rt_v3(1, 2, 0)));   // nQ, on the two finite corners

    // valid queries: nine finite numbers; equal corners are valid
    CHECK(rt_tri_valid(rt_v3(0, 0, 0), rt_v3(0, 0, 0), rt_v3(0, 0, 0)) && rt_tri_valid(rt_v3(-3.4e38f, 0, 0), rt_v3(3.4e38f, 1, 2), rt_v3(0, 0, 0)));
    CHECK(!rt_tri_valid(rt_v3(nan, 0, 0), rt_v3(1, 0, 0), rt_v3(0, 1, 0)) && !rt_tri_valid(rt_v3(0, 0, 0), rt_v3(1, inf, 0), rt_v3(0, 1, 0)) && !rt_tri_valid(rt_v3(0, 0, 0), rt_v3(1, 0, 0), rt_v3(0, 1, -inf)));

    // the sphere of radius 2 about (0,0,0): the shell
    struct SphCase { const char* what; V p, q, r; bool touch; } const sph[] = {
        {"triangle inside the ball", {0.5f, 0, 0}, {0, 0.5f, 0}, {0, 0, 0.5f}, false},
        {"triangle across the shell", {1, 0, 0}, {3, 0, 0}, {1, 1, 0}, true},
        {"triangle outside", {3, 0, 0}, {4, 0, 0}, {3, 1, 0}, false},
        {"tangent from outside, with its face", {-1, -1, 2}, {3, -1, 2}, {-1, 3, 2}, true},
        {"farthest corner exactly on the shell", {2, 0, 0}, {0, 0, 0}, {0, 1, 0}, true},
        {"around the ball, cutting it", {-8, -8, 0}, {16, -8, 0}, {-8, 16, 0}, true},
        {"point on the shell", {0, 2, 0}, {0, 2, 0}, {0, 2, 0}, true},
        {"point at the centre", {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, false},
        {"segment from inside to outside", {0, 0, 1}, {0, 0, 1}, {0, 0, 3}, true},
    };
    for (const SphCase& c : sph) {
        CHECK(rt_tri_sphere(v3(c.p), v3(c.q), v3(c.r), rt_v3(0, 0, 0), 2.f) == c.touch, "%s", c.what);
        CHECK(rt_tri_sphere(v3(c.r), v3(c.p), v3(c.q), rt_v3(0, 0, 0), 2.f) == c.touch, "%s (corners in another order)", c.what);
    }
    CHECK(!rt_tri_sphere(rt_v3(1, 0, 0), rt_v3(3, 0, 0), rt_v3(1, 1, 0), rt_v3(0, 0, 0), nan) && !rt_tri_sphere(rt_v3(1, 0, 0), rt_v3(3, 0, 0), rt_v3(1, 1, 0), rt_v3(nan, 0, 0), 2.f));

    // pruning (b): strict, a box that touches the plane stays; nothing is discarded for a box without bounds or a query without
    // a normal. Q0's plane is z = 0, Q1's x + y - z = 0
    const RtTriQuery t0 = rt_tri_prepare(v3(Q0[0]), v3(Q0[1]), v3(Q0[2])), t1 = rt_tri_prepare(v3(Q1[0]), v3(Q1[1]), v3(Q1[2]));
    CHECK(t0.n.x == 0.f && t0.n.y == 0.f && t0.n.z == 16.f && t0.nLo == 0.f && t0.nHi == 0.f && t0.m.x == 2.f && t0.m.y == 2.f && t0.m.z == 0.f);
    CHECK(rt_tri_plane_apart(&t0, rt_v3(0, 0, 1), rt_v3(4, 4, 2)) && rt_tri_plane_apart(&t0, rt_v3(0, 0, -2), rt_v3(4, 4, -1)));
    CHECK(!rt_tri_plane_apart(&t0, rt_v3(0, 0, 0), rt_v3(4, 4, 2)) && !rt_tri_plane_apart(&t0, rt_v3(0, 0, -1), rt_v3(4, 4, 1)) && !rt_tri_plane_apart(&t0, rt_v3(0, 0, -2), rt_v3(4, 4, 0)));
    CHECK(rt_tri_plane_apart(&t1, rt_v3(1, 1, -2), rt_v3(2, 2, 1)) && !rt_tri_plane_apart(&t1, rt_v3(1, 1, -2), rt_v3(2, 2, 2)));   // x + y - z >= 1 on the first, 0 at a corner of the second
    CHECK(rt_tri_plane_apart(&t1, rt_v3(0, 0, 3), rt_v3(1, 1, 4)) && !rt_tri_plane_apart(&t1, rt_v3(0, 0, 2), rt_v3(1, 1, 4)));
    CHECK(!rt_tri_plane_apart(&t0, rt_v3(-inf, -inf, -inf), rt_v3(inf, inf, inf)) && !rt_tri_plane_apart(&t0, N, N) && !rt_tri_plane_apart(&t1, rt_v3(-inf, -inf, -inf), rt_v3(inf, inf, inf)));
    const RtTriQuery seg = rt_tri_prepare(rt_v3(0, 0, 0), rt_v3(0, 0, 0), rt_v3(4, 4, 0)), pt = rt_tri_prepare(rt_v3(1, 1, 1), rt_v3(1, 1, 1), rt_v3(1, 1, 1));
    CHECK(!rt_tri_plane_apart(&seg, rt_v3(0, 0, 1), rt_v3(4, 4, 2)) && !rt_tri_plane_apart(&pt, rt_v3(5, 5, 5), rt_v3(6, 6, 6)));
    // the world box of a placed node is the box rt_box_placed_apart tests: (x, y, z) -> (10 - y, x, z) takes [1,2] x [3,5] x [0,1]
    // to [5,7] x [1,2] x [0,1]
    const rt_vec3 r0 = rt_v3(0, -1, 0), r1 = rt_v3(1, 0, 0), r2 = rt_v3(0, 0, 1), tr = rt_v3(10, 0, 0);
    const float pad = rt_box_pad(16.f);
    rt_vec3 wlo, whi;
    rt_tri_world_box(r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad, &wlo, &whi);
    CHECK(wlo.x == 5.f - pad && wlo.y == 1.f - pad && wlo.z == 0.f - pad && whi.x == 7.f + pad && whi.y == 2.f + pad && whi.z == 1.f + pad);
    const float qlo[4][3] = {{6, 1.5f, 0.5f}, {7, 2, 1}, {7.5f, 1, 0}, {5, 2.5f, 0}}, qhi[4][3] = {{6, 1.5f, 0.5f}, {8, 3, 2}, {8, 2, 1}, {7, 3, 1}};
    for (int i = 0; i < 4; i++) {
        const rt_vec3 lo = rt_v3(qlo[i][0], qlo[i][1], qlo[i][2]), hi = rt_v3(qhi[i][0], qhi[i][1], qhi[i][2]);
        CHECK(rt_box_apart(lo, hi, wlo, whi) == rt_box_placed_apart(lo, hi, r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad), "box %d", i);
    }
    rt_tri_world_box(r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), rt_box_pad(inf), &wlo, &whi);
    CHECK(wlo.x == -inf && whi.z == inf && !rt_tri_plane_apart(&t0, wlo, whi));
}

// box_queries_check.cpp's hand-made scene: one mesh of two triangles (the triangle (0,0,0) (4,0,0) (0,4,0), and a copy of it at
// z = -8) under an interior root with two leaves, placed twice: by the identity, and moved by (0, 0, 16); a sphere of radius 2
// about (0, 0, 4); and a zeroed sphere slot.
void hand_made_scene() {
    Sphere spheres[2];
    memset(spheres, 0, sizeof spheres);
    spheres[0].position[2] = 4.f; spheres[0].radius = 2.f;
    RayMaterial mats[1];
    memset(mats, 0, sizeof mats);
    TrianglePoint pts[6];
    memset(pts, 0, sizeof pts);
    const float xy[3][2] = {{0, 0}, {4, 0}, {0, 4}};
    for (int t = 0; t < 2; t++)
        for (int v = 0; v < 3; v++) {
            pts[3 * t + v].position[0] = xy[v][0]; pts[3 * t + v].position[1] = xy[v][1]; pts[3 * t + v].position[2] = t ? -8.f : 0.f;
        }
    Triangle tris[2];
    memset(tris, 0, sizeof tris);
    tris[0].v0 = 0; tris[0].v1 = 1; tris[0].v2 = 2;
    tris[1].v0 = 3; tris[1].v1 = 4; tris[1].v2 = 5;
    BVHNode nodes[3] = {{{0, 4}, {0, 4}, {-8, 0}, 1, 0}, {{0, 4}, {0, 4}, {0, 0}, 0, 1}, {{0, 4}, {0, 4}, {-8, -8}, 1, 1}};
    RenderObject objs[2];
    memset(objs, 0, sizeof objs);
    for (RenderObject& o : objs) { o.transformMatrix[0] = o.transformMatrix[5] = o.transformMatrix[10] = o.transformMatrix[15] = 1.f; o.bvhIndex = 0; }
    objs[1].transformMatrix[14] = 16.f;   // its triangles at z = 16 and z = 8
    const RtSceneArrays s{spheres, 2, mats, 1, pts, 6, tris, 2, objs, 2, nodes, 3};

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // 0: an upright triangle whose edge x = y = 1 runs through all four triangles and the ball; 1: a small triangle in the
    // plane z = 0, inside object 0's triangle 0; 2: inside the ball: nothing; 3, 4: invalid; 5: a point on object 1's triangle 1
    const float q[6][9] = {{1, 1, -20, 1, 1, 20, 1, 2, 0}, {1, 1, 0, 2, 1, 0, 1, 2, 0}, {0, 0, 4, 0.5f, 0, 4, 0, 0.5f, 4},
                           {1, 1, 0, 2, nan, 0, 1, 2, 0}, {1, 1, 0, 2, 1, 0, 1, 2, inf}, {1, 1, 8, 1, 1, 8, 1, 1, 8}};
    const RtTriangleBatch all{&q[0][0], 6};
    RtOverlap out[6 * 8];
    uint32_t counts[6];
    memset(counts, 0x77, sizeof counts);
    CHECK(rt_tris_exhaustive_host(&s, &all, 8, out, counts) == 0);
    const uint32_t want[6] = {5, 1, 0, 0, 0, 1};
    for (int i = 0; i < 6; i++) CHECK(counts[i] == want[i], "triangle %d: %u", i, counts[i]);
    const RtOverlap none = rt_box_no_member();
    // query 0: the sphere, then object 0's triangles 0 and 1, then object 1's
    CHECK(out[0].found == 1 && out[0].isSphere == 1 && out[0].objectIndex == 0 && out[0].triIndex == 0);
    for (uint32_t e = 1; e < 5; e++)
        CHECK(out[e].found == 1 && out[e].isSphere == 0 && out[e].objectIndex == (e - 1) / 2 && out[e].triIndex == (e - 1) % 2, "entry %u", e);
    for (uint32_t e = 5; e < 8; e++) CHECK(memcmp(&out[e], &none, sizeof none) == 0);
    CHECK(out[8].found == 1 && out[8].isSphere == 0 && out[8].objectIndex == 0 && out[8].triIndex == 0 && out[9].found == 0);
    CHECK(out[40].found == 1 && out[40].isSphere == 0 && out[40].objectIndex == 1 && out[40].triIndex == 1 && out[41].found == 0);
    for (int i : {2, 3, 4})
        for (uint32_t e = 0; e < 8; e++) CHECK(memcmp(&out[i * 8 + e], &none, sizeof none) == 0);
    // counts are the same for every k, and a smaller k is the head of the same list
    for (uint32_t k : {0u, 1u, 2u}) {
        RtOverlap fewer[6 * 2];
        uint32_t c2[6];
        CHECK(rt_tris_exhaustive_host(&s, &all, k, k ? fewer : nullptr, c2) == 0 && memcmp(c2, counts, sizeof counts) == 0);
        for (int i = 0; i < 6; i++) CHECK(memcmp(&fewer[i * k], &out[i * 8], k * sizeof(RtOverlap)) == 0, "k %u triangle %d", k, i);
    }

    // refusals of the loop itself
    CHECK(rt_tris_exhaustive_host(nullptr, &all, 1, out, counts) == -1);
    CHECK(rt_tris_exhaustive_host(&s, nullptr, 1, out, counts) == -1);
    CHECK(rt_tris_exhaustive_host(&s, &all, 9, out, counts) == -1);
    CHECK(rt_tris_exhaustive_host(&s, &all, 1, nullptr, counts) == -1);
    CHECK(rt_tris_exhaustive_host(&s, &all, 1, out, nullptr) == -1);
    const RtTriangleBatch noCorners{nullptr, 1}, big{&q[0][0], 1u << 30}, empty{nullptr, 0};
    CHECK(rt_tris_exhaustive_host(&s, &noCorners, 1, out, counts) == -1);
    CHECK(rt_tris_exhaustive_host(&s, &big, 1, out, counts) == -1);
    CHECK(rt_tris_exhaustive_host(&s, &empty, 8, nullptr, nullptr) == 0);
    CHECK(rt_tris_exhaustive_host(&s, &empty, 9, nullptr, nullptr) == -1);
    nodes[2].index = 2;   // a leaf range past the triangles
    CHECK(rt_tris_exhaustive_host(&s, &all, 1, out, counts) == -1);
    nodes[2].index = 1;
    objs[1].bvhIndex = 3;   // a root past the nodes
    CHECK(rt_tris_exhaustive_host(&s, &all, 1, out, counts) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    staging();
    rule_table();
    hand_made_scene();
    return check_finish("triangle queries ok");
}
