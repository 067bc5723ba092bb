// obb_queries_check.cpp — what the oriented box queries refuse (ray_tracer_amd/csrc/obb_queries.h: check_obbs_query), in their
// order and with their messages, the block and byte arithmetic of a batch (obbs_shape) at n = 0, 1, 256, 257 and 2^30 - 1, k = 0,
// 1, 8, shared and not, the stack choice (obbs_stack) at depths 24, 25, 64 and 65, the part layout of the _host form for 65 boxes
// (stage_layout), the rule (include/rt_obb_overlap.h) on a table of hand-made cases in small integers and halves, where every
// fp32 operation is exact so that the rule must give the true answer, the pruning's arithmetic, and rt_obbs_exhaustive_host and
// rt_object_frames_host on a hand-made scene, on the CPU, built with plain g++ by tests/test_obbs_host.py. No array of a batch is
// ever dereferenced by the checks: the addresses are made up. Prints "obb queries ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "obb_queries.h"
#include "host_staging.h"
#include "rt_obb_overlap.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const F = at<float>(0x08000000u);
    float* const L = at<float>(0x10000000u);
    float* const H = at<float>(0x30000000u);
    void* const O = at<void>(0x40000000u);
    void* const C = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_oriented_boxes", "rt_query_oriented_boxes_host"}) {
        const std::string f(fn);
        const RtObbBatch ok{F, L, H, 1000, 0}, shared{F, L, H, 1000, 1};
        for (uint32_t k : {0u, 1u, 8u}) CHECK(check_obbs_query(fn, true, &ok, k, O, C).empty() && check_obbs_query(fn, true, &shared, k, O, C).empty());
        CHECK(check_obbs_query(fn, true, &ok, 0, nullptr, C).empty());   // counts only
        CHECK(check_obbs_query(fn, false, &ok, 8, O, C) == f + " before rt_upload_scene");
        CHECK(check_obbs_query(fn, true, nullptr, 8, O, C) == f + ": the batch is NULL");
        const RtObbBatch noF{nullptr, L, H, 5, 0}, noLo{F, nullptr, H, 5, 0}, noHi{F, L, nullptr, 5, 1};
        for (const RtObbBatch* b : {&noF, &noLo, &noHi}) CHECK(check_obbs_query(fn, true, b, 8, O, C) == f + ": frames, lo and hi are required");
        CHECK(check_obbs_query(fn, true, &ok, 9, O, C) == f + ": k = 9 is above RT_BOXES_MAX_K = 8");
        CHECK(check_obbs_query(fn, true, &ok, 0xffffffffu, O, C) == f + ": k = 4294967295 is above RT_BOXES_MAX_K = 8");
        const RtObbBatch two{F, L, H, 5, 2}, many{F, L, H, 5, 0xffffffffu};
        CHECK(check_obbs_query(fn, true, &two, 8, O, C) == f + ": sharedFrame = 2 is neither 0 nor 1");
        CHECK(check_obbs_query(fn, true, &many, 0, nullptr, C) == f + ": sharedFrame = 4294967295 is neither 0 nor 1");
        CHECK(check_obbs_query(fn, true, &ok, 8, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_obbs_query(fn, true, &ok, 0, O, nullptr) == f + ": counts and, with k > 0, the output are required");
        CHECK(check_obbs_query(fn, true, &ok, 1, nullptr, C) == f + ": counts and, with k > 0, the output are required");
        const RtObbBatch big{F, L, H, 1u << 30, 0}, most{F, L, H, (1u << 30) - 1u, 1}, huge{F, L, H, 0xffffffffu, 0};
        CHECK(check_obbs_query(fn, true, &big, 8, O, C) == f + ": a batch of 1073741824 boxes does not fit the 30 bits of a slot id");
        CHECK(check_obbs_query(fn, true, &huge, 0, nullptr, C) == f + ": a batch of 4294967295 boxes does not fit the 30 bits of a slot id");
        CHECK(check_obbs_query(fn, true, &most, 8, O, C).empty());
        // n == 0 succeeds whatever the pointers, k and sharedFrame are, but not without a scene or a batch
        const RtObbBatch none{nullptr, nullptr, nullptr, 0, 7};
        CHECK(check_obbs_query(fn, true, &none, 99, nullptr, nullptr).empty());
        CHECK(check_obbs_query(fn, false, &none, 99, nullptr, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, the arrays, k, sharedFrame, the outputs, the size
        const RtObbBatch bigNoF{nullptr, L, H, 1u << 30, 2}, bigTwo{F, L, H, 1u << 30, 2};
        CHECK(check_obbs_query(fn, false, nullptr, 9, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_obbs_query(fn, true, nullptr, 9, nullptr, nullptr) == f + ": the batch is NULL");
        CHECK(check_obbs_query(fn, true, &bigNoF, 9, nullptr, nullptr) == f + ": frames, lo and hi are required");
        CHECK(check_obbs_query(fn, true, &bigTwo, 9, nullptr, nullptr) == f + ": k = 9 is above RT_BOXES_MAX_K = 8");
        CHECK(check_obbs_query(fn, true, &bigTwo, 8, nullptr, nullptr) == f + ": sharedFrame = 2 is neither 0 nor 1");
        CHECK(check_obbs_query(fn, true, &big, 8, nullptr, C) == f + ": counts and, with k > 0, the output are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtOverlap) == 16 && RT_BOXES_MAX_K == 8 && RT_BOX_WORDS == 2 && RT_OBB_FRAME_FLOATS == 16 && sizeof(RtObbBatch) == 32);
    for (bool shared : {false, true})
        for (uint32_t k : {0u, 1u, 8u}) {
            const ObbShape zero = obbs_shape(0, k, shared, 256);
            CHECK(zero.blocks == 0 && zero.frameBytes == 0 && zero.cornerBytes == 0 && zero.outBytes == 0 && zero.countBytes == 0 && zero.listBytes == 0);
            struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {256, 1}, {257, 2}, {(1u << 30) - 1u, 1u << 22}};
            for (const Row& r : rows) {
                const ObbShape s = obbs_shape(r.n, k, shared, 256);
                CHECK(s.blocks == r.blocks);
                CHECK(s.frameBytes == (shared ? (size_t)64 : (size_t)64 * r.n));
                CHECK(s.cornerBytes == (size_t)12 * r.n && s.countBytes == (size_t)4 * r.n);
                CHECK(s.outBytes == (size_t)16 * r.n * k);
                CHECK(s.listBytes == (size_t)r.blocks * 256 * 64);   // 8 entries of 2 words for every lane of the grid
            }
        }
    CHECK(obbs_shape((1u << 30) - 1u, 8, false, 256).frameBytes == 68719476672ull);   // past 32 bits: size_t arithmetic
    CHECK(obbs_shape((1u << 30) - 1u, 8, false, 256).outBytes == 137438953344ull);
    CHECK(obbs_shape((1u << 30) - 1u, 8, true, 256).listBytes == 68719476736ull);

    std::string e;
    CHECK(obbs_stack("f", 0, &e) == 24 && obbs_stack("f", 24, &e) == 24 && obbs_stack("f", 25, &e) == 64 && obbs_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(obbs_stack("rt_query_oriented_boxes", 65, &e) == 0);
    CHECK(e == "rt_query_oriented_boxes: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_obbs_overlap", "%s", e.c_str());
}

// frames, lo, hi, out, counts of the _host form for 65 boxes, by the one rule of host_staging.h
void staging() {
    struct Case { uint32_t k; bool shared; size_t offset[5], total; } const cases[] = {
        {8, false, {0, 4352, 5376, 6400, 14848}, 15360},   // 4160, 780, 780, 8320, 260 bytes, each from a multiple of 256
        {8, true, {0, 256, 1280, 2304, 10752}, 11264},     // one frame: 64 bytes
        {0, false, {0, 4352, 5376, 6400, 6400}, 6912},     // counts only: no records
        {1, true, {0, 256, 1280, 2304, 3584}, 4096}};
    for (const Case& c : cases) {
        const ObbShape s = obbs_shape(65, c.k, c.shared, 256);
        const size_t bytes[5] = {s.frameBytes, s.cornerBytes, s.cornerBytes, s.outBytes, s.countBytes};
        CHECK(bytes[0] == (c.shared ? 64u : 4160u) && bytes[1] == 780 && bytes[4] == 260 && bytes[3] == (size_t)1040 * c.k);
        const StageLayout g = stage_layout(bytes, 5);
        CHECK(g.ok && g.bytes == c.total, "k %u: %zu", c.k, g.bytes);
        for (int p = 0; p < 5; p++) CHECK(g.offset[p] == c.offset[p], "k %u part %d: %zu", c.k, p, g.offset[p]);
    }
}

// column-major frames from their rows
void frame_rows(float* m, const float r0[4], const float r1[4], const float r2[4]) {
    for (int c = 0; c < 4; c++) { m[4 * c] = r0[c]; m[4 * c + 1] = r1[c]; m[4 * c + 2] = r2[c]; m[4 * c + 3] = c == 3 ? 1.f : 0.f; }
}
void identity_frame(float* m) {
    const float r0[4] = {1, 0, 0, 0}, r1[4] = {0, 1, 0, 0}, r2[4] = {0, 0, 1, 0};
    frame_rows(m, r0, r1, r2);
}
// turned by 90 degrees about z: (x, y, z) -> (y, -x, z)
void quarter_frame(float* m) {
    const float r0[4] = {0, 1, 0, 0}, r1[4] = {-1, 0, 0, 0}, r2[4] = {0, 0, 1, 0};
    frame_rows(m, r0, r1, r2);
}
// turned by 45 degrees about z, times sqrt 2 so that it stays in integers: (x, y, z) -> (x + y, -x + y, z); a similarity about z
// only (z is not scaled), which the triangle rule does not mind
void eighth_frame(float* m) {
    const float r0[4] = {1, 1, 0, 0}, r1[4] = {-1, 1, 0, 0}, r2[4] = {0, 0, 1, 0};
    frame_rows(m, r0, r1, r2);
}

struct Case { const char* what; float lo[3], hi[3]; bool touch; };
bool tri(const float* m, const Case& c, rt_vec3 a, rt_vec3 b, rt_vec3 cc) {
    return rt_obb_triangle(rt_obb_frame(m), rt_v3(c.lo[0], c.lo[1], c.lo[2]), rt_v3(c.hi[0], c.hi[1], c.hi[2]), a, b, cc);
}

uint32_t g_lcg = 12345u;
float small_number() {   // multiples of 1/8 in [-16, 16)
    g_lcg = g_lcg * 1664525u + 1013904223u;
    return (float)((int)((g_lcg >> 8) & 255u) - 128) * 0.125f;
}

void rule_table() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    float I[16], Q[16], E[16];
    identity_frame(I); quarter_frame(Q); eighth_frame(E);
    // rt_obb_point is rt_xform_point, bit for bit; the four floats that are not read may hold anything
    for (int round = 0; round < 200; round++) {
        float m[16];
        for (float& x : m) x = small_number() * 1.1f + 0.3f;
        const rt_vec3 p = rt_v3(small_number() * 0.7f, small_number() * 1.3f, small_number());
        const rt_vec3 want = rt_xform_point(m, p);
        m[3] = nan; m[7] = inf; m[11] = -inf; m[15] = nan;
        const rt_vec3 got = rt_obb_point(rt_obb_frame(m), p);
        CHECK(memcmp(&got, &want, sizeof got) == 0);
        CHECK(rt_obb_valid(rt_obb_frame(m), rt_v3(0, 0, 0), rt_v3(1, 1, 1)));
    }
    // the triangle (0,0,0) (4,0,0) (0,4,0). Under the quarter turn its corners are (0,0,0) (0,-4,0) (4,0,0)
    const rt_vec3 A = rt_v3(0, 0, 0), B = rt_v3(4, 0, 0), Cc = rt_v3(0, 4, 0);
    const Case quarter[] = {
        {"a corner of the triangle in a face of the box", {4, -1, -1}, {6, 1, 1}, true},
        {"just off that face", {4.5f, -1, -1}, {6, 1, 1}, false},
        {"a corner of the triangle on an edge of the box", {4, 0, -1}, {6, 2, 1}, true},
        {"just off that edge", {4, 0.5f, -1}, {6, 2, 1}, false},
        {"a corner of the triangle on a corner of the box", {4, 0, 0}, {6, 2, 2}, true},
        {"just off that corner", {4, 0, 0.5f}, {6, 2, 2}, false},
        {"the plane of the triangle in a face of the box", {0.5f, -1.5f, 0}, {1, -0.5f, 2}, true},
        {"beyond the hypotenuse: only an edge-cross axis separates", {2.5f, -4, -1}, {4, -2.5f, 1}, false},
        {"touches the hypotenuse with an edge of the box", {2, -4, -1}, {4, -2, 1}, true},
        {"the whole triangle inside", {-8, -8, -8}, {8, 8, 8}, true},
        {"where the unturned box would touch: not this one", {1, 1, -1}, {3, 3, 1}, false},
    };
    for (const Case& c : quarter) {
        CHECK(tri(Q, c, A, B, Cc) == c.touch, "quarter turn: %s", c.what);
        CHECK(tri(Q, c, B, Cc, A) == c.touch && tri(Q, c, A, Cc, B) == c.touch, "quarter turn: %s (corners in another order)", c.what);
    }
    // under the eighth turn the corners are (0,0,0) (4,-4,0) (4,4,0): the hypotenuse lies along the box's own y
    const Case eighth[] = {
        {"the hypotenuse in a face of the box", {4, -1, -1}, {6, 1, 1}, true},
        {"just off that face", {4.5f, -1, -1}, {6, 1, 1}, false},
        {"a corner of the triangle on an edge of the box", {4, 4, -1}, {6, 6, 1}, true},
        {"just off that edge", {4, 4.5f, -1}, {6, 6, 1}, false},
        {"a corner of the triangle on a corner of the box", {4, 4, 0}, {5, 5, 1}, true},
        {"just off that corner", {4, 4, 0.5f}, {5, 5, 1}, false},
        {"beside a leg: only an edge-cross axis separates", {0, 2, -1}, {1, 3, 1}, false},
        {"touches a leg with an edge of the box", {0, 1, -1}, {1, 3, 1}, true},
        {"above the plane", {1, 0, 0.5f}, {2, 1, 1}, false},
        {"in the plane", {1, 0, 0}, {2, 1, 1}, true},
    };
    for (const Case& c : eighth) {
        CHECK(tri(E, c, A, B, Cc) == c.touch, "eighth turn: %s", c.what);
        CHECK(tri(E, c, Cc, A, B) == c.touch && tri(E, c, B, A, Cc) == c.touch, "eighth turn: %s (corners in another order)", c.what);
    }
    // a segment (0,0,0)-(2,2,0), under the eighth turn (0,0,0)-(4,0,0), three ways; and the point (1,1,0), there (2,0,0)
    const rt_vec3 S0 = rt_v3(0, 0, 0), S1 = rt_v3(2, 2, 0), Pt = rt_v3(1, 1, 0);
    const Case seg[] = {
        {"segment through the box", {1, -1, -1}, {2, 1, 1}, true},
        {"segment along an edge of the box", {1, 0, 0}, {2, 1, 1}, true},
        {"box beside the segment", {1, 0.5f, -1}, {2, 1, 1}, false},
        {"box touches the segment's end", {4, -1, -1}, {5, 1, 1}, true},
        {"box beyond the segment's end", {4.5f, -1, -1}, {5, 1, 1}, false},
    };
    for (const Case& c : seg)
        CHECK(tri(E, c, S0, S0, S1) == c.touch && tri(E, c, S0, S1, S1) == c.touch && tri(E, c, S1, S0, S1) == c.touch, "segment: %s", c.what);
    const Case pts[] = {
        {"point inside", {1, -1, -1}, {3, 1, 1}, true},
        {"point on a corner", {2, 0, 0}, {3, 1, 1}, true},
        {"point box on the point", {2, 0, 0}, {2, 0, 0}, true},
        {"point outside", {2.5f, -1, -1}, {3, 1, 1}, false},
        {"where the point is in world space: not in the frame", {1, 1, 0}, {1, 1, 0}, false},
    };
    for (const Case& c : pts) CHECK(tri(E, c, Pt, Pt, Pt) == c.touch, "point: %s", c.what);

    // spheres. The sphere of radius 2 about (2,0,0), under the quarter turn about (0,-2,0); the first column (0,-1,0) has length 1
    struct SphCase { const char* what; float lo[3], hi[3]; bool touch; } const sph[] = {
        {"the shell touches a face from outside", {2, -3, -1}, {3, -1, 1}, true},
        {"just off it", {2.5f, -3, -1}, {3, -1, 1}, false},
        {"the farthest corner on the shell from inside", {0, -2, 0}, {2, -2, 0}, true},
        {"a box wholly inside the ball", {-0.5f, -2.5f, -0.5f}, {0.5f, -1.5f, 0.5f}, false},
        {"a box about the whole ball", {-3, -5, -3}, {3, 1, 3}, true},
        {"where the sphere is in world space: inside it, no member", {1.5f, -0.5f, -0.5f}, {2.5f, 0.5f, 0.5f}, false},
    };
    const RtObbFrame q = rt_obb_frame(Q);
    CHECK(rt_obb_scale(q) == 1.f);
    for (const SphCase& c : sph)
        CHECK(rt_obb_sphere(q, rt_obb_scale(q), rt_v3(c.lo[0], c.lo[1], c.lo[2]), rt_v3(c.hi[0], c.hi[1], c.hi[2]), rt_v3(2, 0, 0), 2.f) == c.touch, "%s", c.what);
    // a uniform scale of 2: the radius in the frame is 4, exactly
    float D[16];
    identity_frame(D);
    D[0] = D[5] = D[10] = 2.f;
    const RtObbFrame d = rt_obb_frame(D);
    CHECK(rt_obb_scale(d) == 2.f);
    CHECK(rt_obb_sphere(d, 2.f, rt_v3(4, -1, -1), rt_v3(5, 1, 1), rt_v3(0, 0, 0), 2.f) && !rt_obb_sphere(d, 2.f, rt_v3(4.5f, -1, -1), rt_v3(5, 1, 1), rt_v3(0, 0, 0), 2.f));
    CHECK(!rt_obb_sphere(d, 2.f, rt_v3(-2, -2, -2), rt_v3(2, 2, 2), rt_v3(0, 0, 0), 2.f));   // inside: the farthest corner at sqrt 12 < 4
    // the eighth turn: the first column (1,-1,0) has length fl(sqrt 2), the radius fl(2 sqrt 2) = 2.83: cases away from equality
    const RtObbFrame e = rt_obb_frame(E);
    CHECK(rt_obb_scale(e) == rt_sqrt(2.f));
    CHECK(!rt_obb_sphere(e, rt_obb_scale(e), rt_v3(3, -1, -1), rt_v3(4, 1, 1), rt_v3(0, 0, 0), 2.f) && rt_obb_sphere(e, rt_obb_scale(e), rt_v3(2, -1, -1), rt_v3(4, 1, 1), rt_v3(0, 0, 0), 2.f));
    CHECK(!rt_obb_sphere(e, rt_obb_scale(e), rt_v3(-1, -1, -1), rt_v3(1, 1, 1), rt_v3(0, 0, 0), 2.f));

    // frames that are not finite are not valid: each of the twelve numbers that are read, and none of the four that are not
    for (int at = 0; at < 16; at++)
        for (float bad : {nan, inf, -inf}) {
            float m[16];
            quarter_frame(m);
            m[at] = bad;
            CHECK(rt_obb_valid(rt_obb_frame(m), rt_v3(0, 0, 0), rt_v3(1, 1, 1)) == (at % 4 == 3), "m[%d]", at);
        }
    CHECK(rt_obb_valid(q, rt_v3(0, 0, 0), rt_v3(0, 0, 0)) && !rt_obb_valid(q, rt_v3(0, 2, 0), rt_v3(1, 1, 1)) && !rt_obb_valid(q, rt_v3(nan, 0, 0), rt_v3(1, 1, 1)));
    CHECK(!rt_obb_valid(q, rt_v3(0, 0, 0), rt_v3(1, inf, 1)));
    // singular frames are not refused: the rule applies as written. diag(1, 1, 0) flattens the world onto z' = 0
    float Z[16];
    identity_frame(Z);
    Z[10] = 0.f;
    const RtObbFrame z = rt_obb_frame(Z);
    CHECK(rt_obb_valid(z, rt_v3(0, 0, -1), rt_v3(1, 1, 1)));
    CHECK(rt_obb_triangle(z, rt_v3(0, 0, -1), rt_v3(1, 1, 1), A, B, Cc));
    CHECK(rt_obb_triangle(z, rt_v3(0, 0, -1), rt_v3(1, 1, 1), rt_v3(0, 0, 100), rt_v3(4, 0, 100), rt_v3(0, 4, 100)));   // any height lands in z' = 0
    CHECK(!rt_obb_triangle(z, rt_v3(0, 0, 0.5f), rt_v3(1, 1, 1), A, B, Cc));
    float N0[16];
    memset(N0, 0, sizeof N0);   // the zero frame: every point lands on its translation
    N0[12] = 0.5f;
    CHECK(rt_obb_valid(rt_obb_frame(N0), rt_v3(0, 0, 0), rt_v3(1, 1, 1)) && rt_obb_scale(rt_obb_frame(N0)) == 0.f);
    CHECK(rt_obb_triangle(rt_obb_frame(N0), rt_v3(0, 0, 0), rt_v3(1, 1, 1), rt_v3(9, 9, 9), rt_v3(-7, 8, 1e6f), rt_v3(3, 3, 3)));
    CHECK(!rt_obb_triangle(rt_obb_frame(N0), rt_v3(1, 0, 0), rt_v3(2, 1, 1), rt_v3(9, 9, 9), rt_v3(-7, 8, 1e6f), rt_v3(3, 3, 3)));

    // the identity frame against rt_box_triangle and rt_box_sphere themselves
    const RtObbFrame id = rt_obb_frame(I), id2 = rt_obb_identity();
    CHECK(memcmp(&id, &id2, sizeof id) == 0 && rt_obb_scale(id) == 1.f);
    int kept = 0;
    for (int round = 0; round < 4000; round++) {
        const rt_vec3 c = rt_v3(small_number() * 0.25f, small_number() * 0.25f, small_number() * 0.25f);
        const rt_vec3 h = rt_v3(rt_abs(small_number()) * 0.2f, rt_abs(small_number()) * 0.2f, rt_abs(small_number()) * 0.2f);
        const rt_vec3 lo = rt_sub(c, h), hi = rt_add(c, h);
        const rt_vec3 a = rt_v3(small_number() * 0.3f, small_number() * 0.3f, small_number() * 0.3f);
        const rt_vec3 b = rt_v3(a.x + small_number() * 0.1f, a.y + small_number() * 0.1f, a.z + small_number() * 0.1f);
        const rt_vec3 cc = rt_v3(a.x + small_number() * 0.1f, a.y + small_number() * 0.1f, a.z + small_number() * 0.1f);
        const bool want = rt_box_triangle(lo, hi, a, b, cc);
        kept += want;
        CHECK(rt_obb_triangle(id, lo, hi, a, b, cc) == want);
        const float r = rt_abs(small_number()) * 0.2f;
        CHECK(rt_obb_sphere(id, 1.f, lo, hi, a, r) == rt_box_sphere(lo, hi, a, r));
    }
    CHECK(kept > 200 && kept < 3800, "%d", kept);

    // the pruning's arithmetic: the pad, the magnitudes, the composed map
    CHECK(rt_obb_pad(0.f) > 0.f && rt_obb_pad(16.f) > rt_box_pad(16.f) && rt_obb_pad(16.f) < 1e-4f && rt_obb_pad(inf) == inf && rt_obb_pad(nan) != rt_obb_pad(nan));
    CHECK(rt_obb_mag(q, rt_v3(-1, -2, -3), rt_v3(0.5f, 1, 4)) == 4.f);            // rows (0,1,0) (-1,0,0) (0,0,1): 2, 1, 4
    float T[16];
    quarter_frame(T);
    T[12] = -10.f;
    CHECK(rt_obb_mag(rt_obb_frame(T), rt_v3(-1, -2, -3), rt_v3(0.5f, 1, 4)) == 12.f);   // 2 + |-10|
    CHECK(rt_obb_mag_placed(rt_obb_frame(T), 3.f) == 13.f && rt_obb_mag_placed(e, 3.f) == 6.f);
    // M: scale by 2 and move by (1, 0, 5); F the quarter turn moved by (-10, 0, 0): G v + g = F (M v + t) + s
    const RtObbFrame g = rt_obb_compose(rt_obb_frame(T), rt_v3(2, 0, 0), rt_v3(0, 2, 0), rt_v3(0, 0, 2), rt_v3(1, 0, 5));
    const rt_vec3 v = rt_v3(3, -1, 0.5f), w = rt_v3(7, -2, 6);
    const rt_vec3 direct = rt_obb_point(rt_obb_frame(T), w), composed = rt_obb_point(g, v);
    CHECK(direct.x == -12.f && direct.y == -7.f && direct.z == 6.f && memcmp(&direct, &composed, sizeof direct) == 0);
    // the node box [1,2] x [3,5] x [0,1] under the quarter turn is [3,5] x [-2,-1] x [0,1]
    const float pad = rt_obb_pad(8.f);
    CHECK(!rt_obb_apart(rt_v3(5, -1, 1), rt_v3(6, 0, 2), q, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));     // touching at a corner
    CHECK(rt_obb_apart(rt_v3(5.5f, -2, 0), rt_v3(6, -1, 1), q, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));
    CHECK(rt_obb_apart(rt_v3(3, -0.5f, 0), rt_v3(5, 0, 1), q, rt_v3(1, 3, 0), rt_v3(2, 5, 1), pad));
    CHECK(!rt_obb_apart(rt_v3(5.5f, -2, 0), rt_v3(6, -1, 1), q, rt_v3(1, 3, 0), rt_v3(2, 5, 1), rt_obb_pad(inf)));   // an unbounded object: never
    CHECK(!rt_obb_apart(rt_v3(5.5f, -2, 0), rt_v3(6, -1, 1), q, rt_v3(1, 3, 0), rt_v3(2, 5, 1), nan));
    CHECK(!rt_obb_apart(rt_v3(5.5f, -2, 0), rt_v3(6, -1, 1), q, rt_v3(-inf, -inf, -inf), rt_v3(inf, inf, inf), pad));
}

// What the descent relies on, tried on seeded numbers: a corner v of a node's box, placed as the kernel places it (fp32 through M,
// then fp32 through F), is never apart from the node's box as the kernel projects it: through F with the pad of rt_obb_mag over the
// object's box for an identity object, through fl(F M) with the pad of rt_obb_mag_placed of the object's scale for a placed one.
// The point box [z, z] is the tightest query box that has the corner as a member.
float seeded(float lo, float hi) {
    g_lcg = g_lcg * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(g_lcg >> 8) * (1.f / 16777216.f);
}
void pruning_keeps_every_corner() {
    const float far[4] = {0.f, 1.f, 30.f, 1000.f};
    for (int round = 0; round < 20000; round++) {
        float fm[16], mm[16];
        identity_frame(fm); identity_frame(mm);
        const float fs = far[round % 4], ms = far[(round / 4) % 4], gain = round % 3 ? 1.f : seeded(0.25f, 4.f);
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < 3; r++) { fm[4 * c + r] = seeded(-1.f, 1.f) * gain; mm[4 * c + r] = seeded(-1.5f, 1.5f); }
        for (int r = 0; r < 3; r++) { fm[12 + r] = seeded(-1.f, 1.f) * fs; mm[12 + r] = seeded(-1.f, 1.f) * ms; }
        const RtObbFrame f = rt_obb_frame(fm);
        // the object's root box, a node's box inside it, and corners of the node's box and points within it
        const rt_vec3 c0 = rt_v3(seeded(-2.f, 2.f), seeded(-2.f, 2.f), seeded(-2.f, 2.f)), e0 = rt_v3(seeded(0.f, 2.f), seeded(0.f, 2.f), seeded(0.f, 2.f));
        const rt_vec3 rlo = rt_sub(c0, e0), rhi = rt_add(c0, e0);
        const rt_vec3 blo = rt_v3(seeded(rlo.x, rhi.x), seeded(rlo.y, rhi.y), seeded(rlo.z, rhi.z));
        const rt_vec3 bhi = rt_v3(seeded(blo.x, rhi.x), seeded(blo.y, rhi.y), seeded(blo.z, rhi.z));
        const rt_vec3 a = rt_v3(rt_max(rt_abs(rlo.x), rt_abs(rhi.x)), rt_max(rt_abs(rlo.y), rt_abs(rhi.y)), rt_max(rt_abs(rlo.z), rt_abs(rhi.z)));
        float objMag = 0.f;   // |M| |[v; 1]| over the root box, the largest component (what layout_nearest records, at least)
        for (int r = 0; r < 3; r++) objMag = rt_max(objMag, ((rt_abs(mm[r]) * a.x + rt_abs(mm[4 + r]) * a.y) + rt_abs(mm[8 + r]) * a.z) + rt_abs(mm[12 + r]));
        const RtObbFrame g = rt_obb_compose(f, rt_v3(mm[0], mm[4], mm[8]), rt_v3(mm[1], mm[5], mm[9]), rt_v3(mm[2], mm[6], mm[10]), rt_v3(mm[12], mm[13], mm[14]));
        const float padPlaced = rt_obb_pad(rt_obb_mag_placed(f, objMag)), padIdentity = rt_obb_pad(rt_obb_mag(f, rlo, rhi));
        for (int corner = 0; corner < 12; corner++) {
            const rt_vec3 v = corner < 8 ? rt_v3(corner & 1 ? bhi.x : blo.x, corner & 2 ? bhi.y : blo.y, corner & 4 ? bhi.z : blo.z)
                                         : rt_v3(seeded(blo.x, bhi.x), seeded(blo.y, bhi.y), seeded(blo.z, bhi.z));
            if (!(v.x >= blo.x && v.x <= bhi.x && v.y >= blo.y && v.y <= bhi.y && v.z >= blo.z && v.z <= bhi.z)) continue;   // (seeded() rounds)
            const rt_vec3 zi = rt_obb_point(f, v), zp = rt_obb_point(f, rt_xform_point(mm, v));
            CHECK(!rt_obb_apart(zi, zi, f, blo, bhi, padIdentity), "round %d corner %d: an identity object's corner is pruned", round, corner);
            CHECK(!rt_obb_apart(zp, zp, g, blo, bhi, padPlaced), "round %d corner %d: a placed object's corner is pruned", round, corner);
        }
    }
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
    // the boxes of box_queries_check.cpp under identity frames: rt_boxes_exhaustive_host's bytes
    const float lo[7][3] = {{-20, -20, -20}, {0, 0, 0}, {-0.5f, -0.5f, 3.5f}, {1, 1, 8}, {nan, 0, 0}, {0, 2, 0}, {0, 0, 0}};
    const float hi[7][3] = {{20, 20, 20}, {1, 1, 2}, {0.5f, 0.5f, 4.5f}, {2, 2, 8}, {1, 1, 1}, {1, 1, 1}, {1, inf, 1}};
    float frames[7][16];
    for (auto& f : frames) identity_frame(f);
    const RtBoxBatch plain{&lo[0][0], &hi[0][0], 7};
    const RtObbBatch all{&frames[0][0], &lo[0][0], &hi[0][0], 7, 0}, shared{&frames[0][0], &lo[0][0], &hi[0][0], 7, 1};
    for (uint32_t k : {0u, 1u, 2u, 8u}) {
        RtOverlap want[7 * 8], got[7 * 8], got1[7 * 8];
        uint32_t wc[7], gc[7], gc1[7];
        memset(want, 0x11, sizeof want); memset(got, 0x22, sizeof got); memset(got1, 0x33, sizeof got1);
        CHECK(rt_boxes_exhaustive_host(&s, &plain, k, k ? want : nullptr, wc) == 0);
        CHECK(rt_obbs_exhaustive_host(&s, &all, k, k ? got : nullptr, gc) == 0 && rt_obbs_exhaustive_host(&s, &shared, k, k ? got1 : nullptr, gc1) == 0);
        CHECK(memcmp(wc, gc, sizeof wc) == 0 && memcmp(wc, gc1, sizeof wc) == 0, "k %u", k);
        CHECK(memcmp(want, got, 7 * k * sizeof(RtOverlap)) == 0 && memcmp(want, got1, 7 * k * sizeof(RtOverlap)) == 0, "k %u", k);
        CHECK(wc[0] == 5 && wc[1] == 2 && wc[3] == 1);
    }
    // placed boxes. 0: about everything, turned by 45 degrees; 1: the quarter turn about z: local [3.5, -1, 15] .. [5, 1, 17] is the
    // world box [-1, 3.5, 15] .. [1, 5, 17]: it holds the corner (0,4,16) of object 1's triangle 0 and nothing else; 2: the identity,
    // [3.5, 1, 15] .. [5, 2, 17], beyond that triangle's hypotenuse: nothing; 3: the quarter turn, a local box about (0,-2,4)... the sphere's centre under it is (0,0,4), so
    // [1.5, -0.5, 3.5] .. [2.5, 0.5, 4.5] straddles its shell; 4: a frame with a NaN translation; 5: a frame with an infinite entry;
    // 6: a NaN among the four floats that are not read: as box 1
    float pf[7][16];
    eighth_frame(pf[0]); quarter_frame(pf[1]); identity_frame(pf[2]); quarter_frame(pf[3]); quarter_frame(pf[4]); quarter_frame(pf[5]); quarter_frame(pf[6]);
    pf[4][13] = nan; pf[5][4] = inf; pf[6][3] = nan; pf[6][15] = inf;
    const float plo[7][3] = {{-60, -60, -20}, {3.5f, -1, 15}, {3.5f, 1, 15}, {1.5f, -0.5f, 3.5f}, {3.5f, -1, 15}, {3.5f, -1, 15}, {3.5f, -1, 15}};
    const float phi[7][3] = {{60, 60, 20}, {5, 1, 17}, {5, 2, 17}, {2.5f, 0.5f, 4.5f}, {5, 1, 17}, {5, 1, 17}, {5, 1, 17}};
    const RtObbBatch placed{&pf[0][0], &plo[0][0], &phi[0][0], 7, 0};
    RtOverlap out[7 * 8];
    uint32_t counts[7];
    memset(counts, 0x77, sizeof counts);
    CHECK(rt_obbs_exhaustive_host(&s, &placed, 8, out, counts) == 0);
    const uint32_t want[7] = {5, 1, 0, 1, 0, 0, 1};
    for (int i = 0; i < 7; i++) CHECK(counts[i] == want[i], "placed box %d: %u", i, counts[i]);
    const RtOverlap none = rt_box_no_member();
    CHECK(out[0].found == 1 && out[0].isSphere == 1 && out[0].objectIndex == 0);
    for (uint32_t e = 1; e < 5; e++) CHECK(out[e].found == 1 && out[e].isSphere == 0 && out[e].objectIndex == (e - 1) / 2 && out[e].triIndex == (e - 1) % 2, "entry %u", e);
    for (uint32_t e = 5; e < 8; e++) CHECK(memcmp(&out[e], &none, sizeof none) == 0);
    CHECK(out[8].found == 1 && out[8].isSphere == 0 && out[8].objectIndex == 1 && out[8].triIndex == 0 && out[9].found == 0);
    CHECK(out[24].found == 1 && out[24].isSphere == 1 && out[24].objectIndex == 0 && out[25].found == 0);
    CHECK(memcmp(&out[48], &out[8], 8 * sizeof(RtOverlap)) == 0);
    for (int i : {2, 4, 5})
        for (uint32_t e = 0; e < 8; e++) CHECK(memcmp(&out[i * 8 + e], &none, sizeof none) == 0);
    // a shared frame is the first matrix for every box: the repeated matrix's bytes
    float rep[7][16];
    for (auto& f : rep) quarter_frame(f);
    const RtObbBatch repeated{&rep[0][0], &plo[0][0], &phi[0][0], 7, 0}, one{&rep[0][0], &plo[0][0], &phi[0][0], 7, 1};
    RtOverlap a[7 * 8], b[7 * 8];
    uint32_t ca[7], cb[7];
    CHECK(rt_obbs_exhaustive_host(&s, &repeated, 8, a, ca) == 0 && rt_obbs_exhaustive_host(&s, &one, 8, b, cb) == 0);
    CHECK(memcmp(a, b, sizeof a) == 0 && memcmp(ca, cb, sizeof ca) == 0 && ca[1] == 1 && ca[0] == 5);
    // counts are the same for every k, and a smaller k is the head of the same list
    for (uint32_t k : {0u, 1u, 2u}) {
        RtOverlap fewer[7 * 2];
        uint32_t c2[7];
        CHECK(rt_obbs_exhaustive_host(&s, &placed, k, k ? fewer : nullptr, c2) == 0 && memcmp(c2, counts, sizeof counts) == 0);
        for (int i = 0; i < 7; i++) CHECK(memcmp(&fewer[i * k], &out[i * 8], k * sizeof(RtOverlap)) == 0, "k %u box %d", k, i);
    }

    // refusals of the loop itself
    CHECK(rt_obbs_exhaustive_host(nullptr, &placed, 1, out, counts) == -1);
    CHECK(rt_obbs_exhaustive_host(&s, nullptr, 1, out, counts) == -1);
    CHECK(rt_obbs_exhaustive_host(&s, &placed, 9, out, counts) == -1);
    CHECK(rt_obbs_exhaustive_host(&s, &placed, 1, nullptr, counts) == -1);
    CHECK(rt_obbs_exhaustive_host(&s, &placed, 1, out, nullptr) == -1);
    const RtObbBatch noF{nullptr, &plo[0][0], &phi[0][0], 1, 0}, noLo{&pf[0][0], nullptr, &phi[0][0], 1, 0}, noHi{&pf[0][0], &plo[0][0], nullptr, 1, 0};
    const RtObbBatch big{&pf[0][0], &plo[0][0], &phi[0][0], 1u << 30, 0}, two{&pf[0][0], &plo[0][0], &phi[0][0], 7, 2}, empty{nullptr, nullptr, nullptr, 0, 9};
    for (const RtObbBatch* bad : {&noF, &noLo, &noHi, &big, &two}) CHECK(rt_obbs_exhaustive_host(&s, bad, 1, out, counts) == -1);
    CHECK(rt_obbs_exhaustive_host(&s, &empty, 8, nullptr, nullptr) == 0);
    CHECK(rt_obbs_exhaustive_host(&s, &empty, 9, nullptr, nullptr) == -1);

    // rt_object_frames_host: the inverse matrices; under object 1's the box [0,0,0] .. [1,1,0] is at z = 16 in the world
    const uint32_t which[2] = {1, 0};
    float inv[2][16];
    CHECK(rt_object_frames_host(&s, which, 2, &inv[0][0]) == 0);
    CHECK(inv[0][14] == -16.f && inv[0][0] == 1.f && inv[0][5] == 1.f && inv[0][10] == 1.f && inv[1][14] == 0.f && inv[1][10] == 1.f);
    const float olo[3] = {0, 0, 0}, ohi[3] = {1, 1, 0};
    const RtObbBatch own{&inv[0][0], olo, ohi, 1, 0};
    CHECK(rt_obbs_exhaustive_host(&s, &own, 8, out, counts) == 0 && counts[0] == 1 && out[0].objectIndex == 1 && out[0].triIndex == 0);
    const uint32_t past[1] = {2};
    CHECK(rt_object_frames_host(&s, past, 1, &inv[0][0]) == -1 && rt_object_frames_host(nullptr, which, 1, &inv[0][0]) == -1);
    CHECK(rt_object_frames_host(&s, nullptr, 0, nullptr) == 0);

    nodes[2].index = 2;   // a leaf range past the triangles
    CHECK(rt_obbs_exhaustive_host(&s, &placed, 1, out, counts) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    staging();
    rule_table();
    pruning_keeps_every_corner();
    hand_made_scene();
    return check_finish("obb queries ok");
}
