// box_queries_check.cpp — what the box queries refuse (ray_tracer_amd/csrc/box_queries.h: check_boxes_query), in their order and
// with their messages, the block and byte arithmetic of a batch (boxes_shape) at n = 0, 1, ... 2^30 - 1 and k = 0, 1, 8, the stack
// choice (boxes_stack) at depths 24, 25, 64 and 65, the part layout of the _host form for 65 boxes (stage_layout), the rule
// (include/rt_box_overlap.h) on a table of cases in small integers and halves, where every fp32 operation is exact so that the
// rule must give the true answer, the pruning comparisons, and rt_boxes_exhaustive_host on a hand-made scene, on the CPU, built
// with plain g++ by tests/test_boxes_host.py. No array of a batch is ever dereferenced by the checks: the addresses are made up.
// Prints "box queries ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "box_queries.h"
#include "host_staging.h"
#include "rt_box_overlap.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const L = at<float>(0x10000000u);
    float* const H = at<float>(0x30000000u);
    void* const O = at<void>(0x40000000u);
    void* const C = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_boxes", "rt_query_boxes_host"}) {
        const std::string f(fn);
        const RtBoxBatch ok{L, H, 1000};
        for (uint32_t k : {0u, 1u, 8u}) CHECK(check_boxes_query(fn, true, &ok, k, O, C).empty());
        CHECK(check_boxes_query(fn, true, &ok, 0, nullptr, C).empty());   // counts only
        CHECK(check_boxes_query(fn, false, &ok, 8, O, C) == f + " before rt_upload_scene");
        CHECK(check_boxes_query(fn, true, nullptr, 8, O, C) == f + ": the batch is NULL");
        const RtBoxBatch noLo{nullptr, H, 5}, noHi{L, nullptr, 5};
        CHECK(check_boxes_query(fn, true, &noLo, 8, O, C) == f + ": lo and hi are required");
        CHECK(check_boxes_query(fn, true, &noHi, 8, O, C) == f + ": lo and hi are required");
        CHECK(check_boxes_query(fn, true, &ok, 9, O, C) == f + ": k = 9 is above RT_BOXES_MAX_K = 8");
        CHECK(check_boxes_query(fn, true, &ok, 0xffffffffu, O, C) == f + ": k = 4294967295 is above RT_BOXES_MAX_K = 8");
        CHECK(check_boxes_query(fn, true, &ok, 8, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_boxes_query(fn, true, &ok, 0, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_boxes_query(fn, true, &ok, 1, nullptr, C) == f + ": counts and, with k > 0, the output are required");
        const RtBoxBatch big{L, H, 1u << 30}, most{L, H, (1u << 30) - 1u}, huge{L, H, 0xffffffffu};
        CHECK(check_boxes_query(fn, true, &big, 8, O, C) == f + ": a batch of 1073741824 boxes does not fit the 30 bits of a slot id");
        CHECK(check_boxes_query(fn, true, &huge, 0, nullptr, C) == f + ": a batch of 4294967295 boxes does not fit the 30 bits of a slot id");
        CHECK(check_boxes_query(fn, true, &most, 8, O, C).empty());
        // n == 0 succeeds whatever the pointers and k are, but not without a scene or a batch
        const RtBoxBatch none{nullptr, nullptr, 0};
        CHECK(check_boxes_query(fn, true, &none, 99, nullptr, nullptr).empty());
        CHECK(check_boxes_query(fn, false, &none, 99, nullptr, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, the corners, k, the outputs, the size
        const RtBoxBatch bigNoLo{nullptr, H, 1u << 30};
        CHECK(check_boxes_query(fn, false, nullptr, 9, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_boxes_query(fn, true, nullptr, 9, nullptr, nullptr) == f + ": the batch is NULL");
        CHECK(check_boxes_query(fn, true, &bigNoLo, 9, nullptr, nullptr) == f + ": lo and hi are required");
        CHECK(check_boxes_query(fn, true, &big, 9, nullptr, nullptr) == f + ": k = 9 is above RT_BOXES_MAX_K = 8");
        CHECK(check_boxes_query(fn, true, &big, 8, nullptr, C) == f + ": counts and, with k > 0, the output are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtOverlap) == 16 && RT_BOXES_MAX_K == 8 && RT_BOX_WORDS == 2);
    for (uint32_t k : {0u, 1u, 8u}) {
        const BoxesShape zero = boxes_shape(0, k, 256);
        CHECK(zero.blocks == 0 && zero.cornerBytes == 0 && zero.outBytes == 0 && zero.countBytes == 0 && zero.listBytes == 0);
        struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
        for (const Row& r : rows) {
            const BoxesShape s = boxes_shape(r.n, k, 256);
            CHECK(s.blocks == r.blocks);
            CHECK(s.cornerBytes == (size_t)12 * r.n && s.countBytes == (size_t)4 * r.n);
            CHECK(s.outBytes == (size_t)16 * r.n * k);
            CHECK(s.listBytes == (size_t)r.blocks * 256 * 64);   // 8 entries of 2 words for every lane of the grid
        }
    }
    CHECK(boxes_shape((1u << 30) - 1u, 8, 256).outBytes == 137438953344ull);   // past 32 bits: size_t arithmetic
    CHECK(boxes_shape((1u << 30) - 1u, 8, 256).cornerBytes == 12884901876ull);
    CHECK(boxes_shape((1u << 30) - 1u, 1, 256).outBytes == 17179869168ull);
    CHECK(boxes_shape((1u << 30) - 1u, 8, 256).listBytes == 68719476736ull);

    std::string e;
    CHECK(boxes_stack("f", 0, &e) == 24 && boxes_stack("f", 24, &e) == 24 && boxes_stack("f", 25, &e) == 64 && boxes_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(boxes_stack("rt_query_boxes", 65, &e) == 0);
    CHECK(e == "rt_query_boxes: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_boxes_overlap");
}

// lo, hi, out, counts of the _host form for 65 boxes, by the one rule of host_staging.h
void staging() {
    struct Case { uint32_t k; size_t offset[4], total; } const cases[] = {
        {8, {0, 1024, 2048, 10496}, 11008},   // 780, 780, 8320, 260 bytes, each from a multiple of 256
        {0, {0, 1024, 2048, 2048}, 2560},     // counts only: no records
        {1, {0, 1024, 2048, 3328}, 3840}};
    for (const Case& c : cases) {
        const BoxesShape s = boxes_shape(65, c.k, 256);
        const size_t bytes[4] = {s.cornerBytes, s.cornerBytes, s.outBytes, s.countBytes};
        CHECK(bytes[0] == 780 && bytes[3] == 260 && bytes[2] == (size_t)1040 * c.k);
        const StageLayout g = stage_layout(bytes, 4);
        CHECK(g.ok && g.bytes == c.total, "k %u: %zu", c.k, g.bytes);
        for (int p = 0; p < 4; p++) CHECK(g.offset[p] == c.offset[p], "k %u part %d: %zu", c.k, p, g.offset[p]);
    }
}

struct TriCase { const char* what; float lo[3], hi[3]; bool touch; };
bool tri(const TriCase& c, rt_vec3 a, rt_vec3 b, rt_vec3 cc) {
    return rt_box_triangle(rt_v3(c.lo[0], c.lo[1], c.lo[2]), rt_v3(c.hi[0], c.hi[1], c.hi[2]), a, b, cc);
}

void rule_table() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the triangle (0,0,0) (4,0,0) (0,4,0): small integers and halves, every operation of the rule is exact
    const rt_vec3 A = rt_v3(0, 0, 0), B = rt_v3(4, 0, 0), Cc = rt_v3(0, 4, 0);
    const TriCase cases[] = {
        {"touches at the vertex (0,0,0)", {-1, -1, -1}, {0, 0, 0}, true},
        {"touches at the vertex (4,0,0)", {4, -2, -1}, {6, 0, 1}, true},
        {"just off the vertex (4,0,0)", {4.5f, -2, -1}, {6, 0, 1}, false},
        {"touches along the edge y = 0", {1, -2, -1}, {3, 0, 1}, true},
        {"just below the edge y = 0", {1, -2, -1}, {3, -0.5f, 1}, false},
        {"touches in the plane from above", {0.5f, 0.5f, 0}, {1.5f, 1.5f, 2}, true},
        {"touches in the plane from below", {0.5f, 0.5f, -2}, {1.5f, 1.5f, 0}, true},
        {"straddles the plane", {0.5f, 0.5f, -1}, {1.5f, 1.5f, 1}, true},
        {"above the plane: only stage 1's z separates", {0.5f, 0.5f, 0.5f}, {1.5f, 1.5f, 2}, false},
        {"beyond the hypotenuse: only an edge-cross axis separates", {2.5f, 2.5f, -1}, {4, 4, 1}, false},
        {"touches the hypotenuse at its corner", {2, 2, -1}, {4, 4, 1}, true},
        {"cuts the hypotenuse", {1.5f, 1.5f, -1}, {3, 3, 1}, true},
        {"point box on the vertex (4,0,0)", {4, 0, 0}, {4, 0, 0}, true},
        {"point box on the hypotenuse", {2, 2, 0}, {2, 2, 0}, true},
        {"point box inside the face", {1, 1, 0}, {1, 1, 0}, true},
        {"point box off the face, in the plane", {2.5f, 2, 0}, {2.5f, 2, 0}, false},
        {"point box above the face", {1, 1, 0.5f}, {1, 1, 0.5f}, false},
        {"flat box in the plane, overlapping", {1, 1, 0}, {6, 6, 0}, true},
        {"flat box in the plane, beyond the hypotenuse", {3, 3, 0}, {6, 6, 0}, false},
        {"flat box in the plane, touching the hypotenuse", {3, 1, 0}, {6, 6, 0}, true},
        {"flat box across the plane", {1, 1, -1}, {1, 3, 1}, true},
        {"the whole triangle inside", {-8, -8, -8}, {8, 8, 8}, true},
        {"the box inside the triangle's outline, flat", {0.5f, 0.5f, 0}, {1, 1, 0}, true},
    };
    for (const TriCase& c : cases) {
        CHECK(tri(c, A, B, Cc) == c.touch, "%s", c.what);
        CHECK(tri(c, B, Cc, A) == c.touch && tri(c, Cc, A, B) == c.touch && tri(c, A, Cc, B) == c.touch, "%s (corners in another order)", c.what);
    }
    // a tilted triangle (0,0,0) (4,0,4) (0,4,4), plane x + y - z = 0: boxes that pass the three box axes and only the plane separates
    const rt_vec3 P = rt_v3(0, 0, 0), Q = rt_v3(4, 0, 4), R = rt_v3(0, 4, 4);
    const TriCase plane[] = {
        {"under the tilted plane: only the plane axis separates", {1, 1, 0}, {1.5f, 1.5f, 1.5f}, false},
        {"touches the tilted plane with a corner", {1, 1, 0}, {1.5f, 1.5f, 2}, true},
        {"over the tilted plane: only the plane axis separates", {0.5f, 0.5f, 2.5f}, {1, 1, 4}, false},
        {"touches the tilted plane from over it", {0.5f, 0.5f, 1}, {1, 1, 4}, true},
    };
    for (const TriCase& c : plane) CHECK(tri(c, P, Q, R) == c.touch && tri(c, Q, R, P) == c.touch, "%s", c.what);

    // degenerate triangles: the segment (0,0,0)-(4,4,0) three ways, and the point (2,2,0)
    const rt_vec3 S0 = rt_v3(0, 0, 0), S1 = rt_v3(4, 4, 0);
    const TriCase seg[] = {
        {"segment through the box", {1, 1, -1}, {2, 2, 1}, true},
        {"segment touches the box's edge", {2, 0, -1}, {4, 2, 1}, true},
        {"segment passes the box's corner region: only e x unit_z separates", {2.5f, 0, -1}, {4, 2, 1}, false},
        {"box beyond the segment's end", {4.5f, 4.5f, -1}, {6, 6, 1}, false},
        {"box touches the segment's end", {4, 4, 0}, {6, 6, 1}, true},
        {"box above the segment", {1, 1, 0.5f}, {2, 2, 1}, false},
    };
    for (const TriCase& c : seg) {
        CHECK(tri(c, S0, S0, S1) == c.touch, "%s (a == b)", c.what);
        CHECK(tri(c, S0, S1, S1) == c.touch, "%s (b == c)", c.what);
        CHECK(tri(c, S1, S0, S1) == c.touch, "%s (a == c)", c.what);
    }
    const rt_vec3 Pt = rt_v3(2, 2, 0);
    const TriCase pts[] = {
        {"point inside", {1, 1, -1}, {3, 3, 1}, true},
        {"point on a face", {2, 1, -1}, {3, 3, 1}, true},
        {"point on a corner", {2, 2, 0}, {3, 3, 1}, true},
        {"point box on the point", {2, 2, 0}, {2, 2, 0}, true},
        {"point outside", {2.5f, 1, -1}, {3, 3, 1}, false},
    };
    for (const TriCase& c : pts) CHECK(tri(c, Pt, Pt, Pt) == c.touch, "%s", c.what);
    // NaN separates nothing: a triangle of NaN corners is a member of every valid box; one finite axis that separates does
    const rt_vec3 N = rt_v3(nan, nan, nan);
    CHECK(rt_box_triangle(rt_v3(0, 0, 0), rt_v3(1, 1, 1), N, N, N));
    CHECK(!rt_box_triangle(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(nan, 2, 0), rt_v3(nan, 3, 0), rt_v3(nan, 2, 1)));

    // the sphere of radius 2 about (0,0,0): the shell
    struct SphCase { const char* what; float lo[3], hi[3]; bool touch; } const sph[] = {
        {"box inside the ball", {-1, -1, -1}, {1, 1, 1}, false},
        {"box straddles the shell", {1, -1, -1}, {3, 1, 1}, true},
        {"box outside", {2.5f, -1, -1}, {3, 1, 1}, false},
        {"box tangent from outside", {2, -1, -1}, {3, 1, 1}, true},
        {"box around the whole ball", {-3, -3, -3}, {3, 3, 3}, true},
        {"farthest corner exactly on the shell", {0, 0, 0}, {2, 0, 0}, true},
        {"point box on the shell", {0, 2, 0}, {0, 2, 0}, true},
        {"point box at the centre", {0, 0, 0}, {0, 0, 0}, false},
        {"point box outside", {0, 2.5f, 0}, {0, 2.5f, 0}, false},
    };
    for (const SphCase& c : sph)
        CHECK(rt_box_sphere(rt_v3(c.lo[0], c.lo[1], c.lo[2]), rt_v3(c.hi[0], c.hi[1], c.hi[2]), rt_v3(0, 0, 0), 2.f) == c.touch, "%s", c.what);
    CHECK(!rt_box_sphere(rt_v3(1, -1, -1), rt_v3(3, 1, 1), rt_v3(0, 0, 0), nan) && !rt_box_sphere(rt_v3(1, -1, -1), rt_v3(3, 1, 1), rt_v3(nan, 0, 0), 2.f));
    CHECK(rt_box_far2(rt_v3(0, 0, 0), rt_v3(1, -1, -1), rt_v3(3, 1, 1)) == 11.f && rt_box_far2(rt_v3(5, 0, 0), rt_v3(1, -1, -1), rt_v3(3, 2, 1)) == 21.f);

    // valid boxes
    CHECK(rt_box_valid(rt_v3(0, 0, 0), rt_v3(1, 1, 1)) && rt_box_valid(rt_v3(0, 0, 0), rt_v3(0, 0, 0)) && rt_box_valid(rt_v3(-1, 2, 3), rt_v3(-1, 5, 3)));
    CHECK(rt_box_valid(rt_v3(-3.4e38f, -3.4e38f, -3.4e38f), rt_v3(3.4e38f, 3.4e38f, 3.4e38f)));
    CHECK(!rt_box_valid(rt_v3(nan, 0, 0), rt_v3(1, 1, 1)) && !rt_box_valid(rt_v3(0, 0, 0), rt_v3(1, nan, 1)));
    CHECK(!rt_box_valid(rt_v3(0, 0, 2), rt_v3(1, 1, 1)) && !rt_box_valid(rt_v3(0, 0, 0), rt_v3(1, inf, 1)) && !rt_box_valid(rt_v3(-inf, 0, 0), rt_v3(1, 1, 1)));
    // the widest finite box: centre and half-extent do not overflow, and the triangle is a member
    CHECK(rt_box_triangle(rt_v3(-3.4e38f, -3.4e38f, -3.4e38f), rt_v3(3.4e38f, 3.4e38f, 3.4e38f), A, B, Cc));

    // the key and the list: spheres first, then the object, then the triangle; 2 words an entry
    CHECK(rt_box_sphere_word(3) == rt_hits_sphere_word(3, false) && rt_box_triangle_word(7) == 7);
    uint32_t list[2 * RT_BOX_WORDS], have = 0;
    have = rt_box_insert(list, 1, 2, have, rt_box_triangle_word(1), 9);
    have = rt_box_insert(list, 1, 2, have, rt_box_triangle_word(1), 2);
    CHECK(have == 2 && list[0] == 1 && list[1] == 2 && list[2] == 1 && list[3] == 9);
    have = rt_box_insert(list, 1, 2, have, rt_box_triangle_word(2), 0);        // does not come before the last: dropped
    CHECK(have == 2 && list[2] == 1 && list[3] == 9);
    have = rt_box_insert(list, 1, 2, have, rt_box_sphere_word(5), 0);          // a sphere comes first
    CHECK(have == 2 && list[0] == rt_box_sphere_word(5) && list[2] == 1 && list[3] == 2);
    CHECK(rt_box_insert(list, 1, 0, 0, 1, 1) == 0);
    const RtOverlap none = rt_box_no_member(), s = rt_box_record(rt_box_sphere_word(5), 0), t = rt_box_record(3, 11);
    RtOverlap zero;
    memset(&zero, 0, sizeof zero);
    CHECK(memcmp(&none, &zero, sizeof zero) == 0);
    CHECK(s.found == 1 && s.isSphere == 1 && s.objectIndex == 5 && s.triIndex == 0);
    CHECK(t.found == 1 && t.isSphere == 0 && t.objectIndex == 3 && t.triIndex == 11);

    // the pruning comparisons: strict, touching boxes are not apart; the placed form on a translation and a rotation by 90 degrees
    CHECK(!rt_box_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(1, 1, 1), rt_v3(2, 2, 2)) && rt_box_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(1.5f, 0, 0), rt_v3(2, 1, 1)));
    CHECK(rt_box_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(0, 0, -2), rt_v3(1, 1, -1)) && !rt_box_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(nan, nan, nan), rt_v3(nan, nan, nan)));
    const rt_vec3 r0 = rt_v3(0, -1, 0), r1 = rt_v3(1, 0, 0), r2 = rt_v3(0, 0, 1), tr = rt_v3(10, 0, 0);   // (x, y, z) -> (10 - y, x, z)
    const float pad = rt_box_pad(16.f);
    CHECK(pad > 0.f && pad < 1e-4f);
    // the node box [1,2] x [3,5] x [0,1] goes to [5,7] x [1,2] x [0,1]
    CHECK(!rt_box_placed_apart(rt_v3(6, 1.5f, 0.5f), rt_v3(6, 1.5f, 0.5f), r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));
    CHECK(!rt_box_placed_apart(rt_v3(7, 2, 1), rt_v3(8, 3, 2), r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));      // touching
    CHECK(rt_box_placed_apart(rt_v3(7.5f, 1, 0), rt_v3(8, 2, 1), r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));
    CHECK(rt_box_placed_apart(rt_v3(5, 2.5f, 0), rt_v3(7, 3, 1), r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));
    CHECK(!rt_box_placed_apart(rt_v3(7.5f, 1, 0), rt_v3(8, 2, 1), r0, r1, r2, tr, rt_v3(1, 3, 0), rt_v3(2, 5, 1), rt_box_pad(inf)));   // an unbounded object: never
    CHECK(rt_box_object_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(2, 0, 0), rt_v3(3, 1, 1), pad) && !rt_box_object_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(1, 0, 0), rt_v3(3, 1, 1), pad));
    CHECK(!rt_box_object_apart(rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(-inf, -inf, -inf), rt_v3(inf, inf, inf), rt_box_pad(inf)));
}

// A hand-made scene: one mesh of two triangles (the triangle (0,0,0) (4,0,0) (0,4,0), and a copy of it at z = -8) under an
// interior root with two leaves, placed twice: by the identity, and moved by (0, 0, 16); a sphere of radius 2 about (0, 0, 4); and a
// zeroed sphere slot.
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
    // box 0: everything; 1: the sphere's shell and object 0's triangle 0 (touching its plane); 2: inside the ball: nothing;
    // 3: object 1's triangle 1 at z = 8 only, a flat box in its plane; 4..6: invalid
    const float lo[7][3] = {{-20, -20, -20}, {0, 0, 0}, {-0.5f, -0.5f, 3.5f}, {1, 1, 8}, {nan, 0, 0}, {0, 2, 0}, {0, 0, 0}};
    const float hi[7][3] = {{20, 20, 20}, {1, 1, 2}, {0.5f, 0.5f, 4.5f}, {2, 2, 8}, {1, 1, 1}, {1, 1, 1}, {1, inf, 1}};
    const RtBoxBatch all{&lo[0][0], &hi[0][0], 7};
    RtOverlap out[7 * 8];
    uint32_t counts[7];
    memset(counts, 0x77, sizeof counts);
    CHECK(rt_boxes_exhaustive_host(&s, &all, 8, out, counts) == 0);
    const uint32_t want[7] = {5, 2, 0, 1, 0, 0, 0};
    for (int i = 0; i < 7; i++) CHECK(counts[i] == want[i], "box %d: %u", i, counts[i]);
    const RtOverlap none = rt_box_no_member();
    // box 0: the sphere, then object 0's triangles 0 and 1, then object 1's
    CHECK(out[0].found == 1 && out[0].isSphere == 1 && out[0].objectIndex == 0 && out[0].triIndex == 0);
    for (uint32_t e = 1; e < 5; e++)
        CHECK(out[e].found == 1 && out[e].isSphere == 0 && out[e].objectIndex == (e - 1) / 2 && out[e].triIndex == (e - 1) % 2, "entry %u", e);
    for (uint32_t e = 5; e < 8; e++) CHECK(memcmp(&out[e], &none, sizeof none) == 0);
    CHECK(out[8].isSphere == 1 && out[9].found == 1 && out[9].isSphere == 0 && out[9].objectIndex == 0 && out[9].triIndex == 0 && out[10].found == 0);
    CHECK(out[24].found == 1 && out[24].isSphere == 0 && out[24].objectIndex == 1 && out[24].triIndex == 1 && out[25].found == 0);
    for (int i : {2, 4, 5, 6})
        for (uint32_t e = 0; e < 8; e++) CHECK(memcmp(&out[i * 8 + e], &none, sizeof none) == 0);
    // counts are the same for every k, and a smaller k is the head of the same list
    for (uint32_t k : {0u, 1u, 2u}) {
        RtOverlap fewer[7 * 2];
        uint32_t c2[7];
        CHECK(rt_boxes_exhaustive_host(&s, &all, k, k ? fewer : nullptr, c2) == 0 && memcmp(c2, counts, sizeof counts) == 0);
        for (int i = 0; i < 7; i++) CHECK(memcmp(&fewer[i * k], &out[i * 8], k * sizeof(RtOverlap)) == 0, "k %u box %d", k, i);
    }

    // refusals of the loop itself
    CHECK(rt_boxes_exhaustive_host(nullptr, &all, 1, out, counts) == -1);
    CHECK(rt_boxes_exhaustive_host(&s, nullptr, 1, out, counts) == -1);
    CHECK(rt_boxes_exhaustive_host(&s, &all, 9, out, counts) == -1);
    CHECK(rt_boxes_exhaustive_host(&s, &all, 1, nullptr, counts) == -1);
    CHECK(rt_boxes_exhaustive_host(&s, &all, 1, out, nullptr) == -1);
    const RtBoxBatch noLo{nullptr, &hi[0][0], 1}, noHi{&lo[0][0], nullptr, 1}, big{&lo[0][0], &hi[0][0], 1u << 30}, empty{nullptr, nullptr, 0};
    CHECK(rt_boxes_exhaustive_host(&s, &noLo, 1, out, counts) == -1 && rt_boxes_exhaustive_host(&s, &noHi, 1, out, counts) == -1);
    CHECK(rt_boxes_exhaustive_host(&s, &big, 1, out, counts) == -1);
    CHECK(rt_boxes_exhaustive_host(&s, &empty, 8, nullptr, nullptr) == 0);
    CHECK(rt_boxes_exhaustive_host(&s, &empty, 9, nullptr, nullptr) == -1);
    nodes[2].index = 2;   // a leaf range past the triangles
    CHECK(rt_boxes_exhaustive_host(&s, &all, 1, out, counts) == -1);
    nodes[2].index = 1;
    objs[1].bvhIndex = 3;   // a root past the nodes
    CHECK(rt_boxes_exhaustive_host(&s, &all, 1, out, counts) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    staging();
    rule_table();
    hand_made_scene();
    return check_finish("box queries ok");
}
