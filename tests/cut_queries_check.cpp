// cut_queries_check.cpp — what the cut queries refuse (check_tris_query under their names), in its order and with its messages,
// the block and byte arithmetic of a batch (ray_tracer_amd/csrc/cut_queries.h: cuts_shape) at n = 0, 1, ... 2^30 - 1 and
// k = 0, 1, 8, the stack choice (cuts_stack), the part layout of the _host form for 65 triangles (stage_layout), the rule
// (include/rt_tri_cut.h) on hand-made cases in small integers and halves, where every fp32 operation is exact so that the end
// points, the features and the a / b order can be given as literals, the bit-equality of the end on an edge that two scene
// triangles share, whatever their windings, and rt_cuts_exhaustive_host on a hand-made scene, on the CPU, built with plain g++ by
// tests/test_cuts_host.py. No array of a batch is ever dereferenced by the checks: the addresses are made up.
// Prints "cut queries ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "cut_queries.h"
#include "host_staging.h"
#include "rt_tri_cut.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const P = at<float>(0x10000000u);
    void* const O = at<void>(0x40000000u);
    void* const C = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_cuts", "rt_query_cuts_host"}) {
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
    CHECK(sizeof(RtCut) == 48 && offsetof(RtCut, featA) == 12 && offsetof(RtCut, b) == 16 && offsetof(RtCut, featB) == 28 && offsetof(RtCut, found) == 32 && offsetof(RtCut, reserved) == 44);
    for (uint32_t k : {0u, 1u, 8u}) {
        const CutsShape zero = cuts_shape(0, k, 256);
        CHECK(zero.blocks == 0 && zero.cornerBytes == 0 && zero.outBytes == 0 && zero.countBytes == 0 && zero.listBytes == 0);
        struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
        for (const Row& r : rows) {
            const CutsShape s = cuts_shape(r.n, k, 256);
            CHECK(s.blocks == r.blocks);
            CHECK(s.cornerBytes == (size_t)36 * r.n && s.countBytes == (size_t)4 * r.n);
            CHECK(s.outBytes == (size_t)48 * r.n * k);
            CHECK(s.listBytes == (size_t)r.blocks * 256 * 64);   // 8 keys of 2 words for every lane of the grid
            CHECK(s.listBytes == tris_shape(r.n, k, 256).listBytes);   // the buffer is the box and triangle queries'
        }
    }
    CHECK(cuts_shape((1u << 30) - 1u, 8, 256).outBytes == 412316860032ull);   // past 32 bits: size_t arithmetic
    CHECK(cuts_shape((1u << 30) - 1u, 8, 256).cornerBytes == 38654705628ull);

    std::string e;
    CHECK(cuts_stack("f", 0, &e) == 24 && cuts_stack("f", 24, &e) == 24 && cuts_stack("f", 25, &e) == 64 && cuts_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(cuts_stack("rt_query_cuts", 65, &e) == 0);
    CHECK(e == "rt_query_cuts: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_tris_cut", "%s", e.c_str());
}

// corners, out, counts of the _host form for 65 triangles, by the one rule of host_staging.h
void staging() {
    struct Case { uint32_t k; size_t offset[3], total; } const cases[] = {
        {8, {0, 2560, 27648}, 28160},   // 2340, 24960, 260 bytes, each from a multiple of 256
        {0, {0, 2560, 2560}, 3072},     // counts only: no records
        {1, {0, 2560, 5888}, 6400}};    // 3120 bytes of records
    for (const Case& c : cases) {
        const CutsShape s = cuts_shape(65, c.k, 256);
        const size_t bytes[3] = {s.cornerBytes, s.outBytes, s.countBytes};
        CHECK(bytes[0] == 2340 && bytes[2] == 260 && bytes[1] == (size_t)3120 * c.k);
        const StageLayout g = stage_layout(bytes, 3);
        CHECK(g.ok && g.bytes == c.total, "k %u: %zu", c.k, g.bytes);
        for (int p = 0; p < 3; p++) CHECK(g.offset[p] == c.offset[p], "k %u part %d: %zu", c.k, p, g.offset[p]);
    }
}

struct V { float x, y, z; };
rt_vec3 v3(const V& v) { return rt_v3(v.x, v.y, v.z); }
bool same(rt_vec3 u, const V& v) { return u.x == v.x && u.y == v.y && u.z == v.z; }
bool same_bits(rt_vec3 u, rt_vec3 v) { return memcmp(&u, &v, sizeof u) == 0; }

struct CutCase { const char* what; V a, b, c; bool touch, cut; V ea; uint32_t fa; V eb; uint32_t fb; };

void rule_table() {
    // the query (0,0,0) (4,0,0) (0,4,0) in the plane z = 0, m = (2, 2, 0), nQ = (0, 0, 16): small integers and halves, every
    // operation of the rule is exact
    const V Q0[3] = {{0, 0, 0}, {4, 0, 0}, {0, 4, 0}};
    const CutCase cases[] = {
        // two triangles crossing at right angles: the scene's in the plane x = 1, nT = (16, 0, 0), D = (0, 256, 0): a is the end
        // of lower y. The query's chord on x = 1 is y in [0, 3], the scene triangle's on z = 0 is y in [-0.5, 2.5]
        {"crossing at right angles", {1, -1, -1}, {1, 3, -1}, {1, 1, 3}, true, true, {1, 0, 0}, 0, {1, 2.5f, 0}, 4},
        // ... the same triangle wound the other way: nT and D turn round, and so do a and b; the edge b c is now edge 0 (c b)
        {"crossing at right angles, wound the other way", {1, 1, 3}, {1, 3, -1}, {1, -1, -1}, true, true, {1, 2.5f, 0}, 3, {1, 0, 0}, 0},
        // DESIGN.md's coplanar pair, apart by nQ x eQ1 alone: no member of the triangle query, no cut
        {"coplanar, beyond the hypotenuse", {3, 3, 0}, {6, 3, 0}, {3, 6, 0}, false, false, {0, 0, 0}, 0, {0, 0, 0}, 0},
        // coplanar and touching: members of the triangle query, no cut
        {"coplanar, touching the hypotenuse with a corner", {2, 2, 0}, {6, 2, 0}, {2, 6, 0}, true, false, {0, 0, 0}, 0, {0, 0, 0}, 0},
        {"coplanar, inside the query", {0.5f, 0.5f, 0}, {1.5f, 0.5f, 0}, {0.5f, 1.5f, 0}, true, false, {0, 0, 0}, 0, {0, 0, 0}, 0},
        {"the same triangle", {0, 0, 0}, {4, 0, 0}, {0, 4, 0}, true, false, {0, 0, 0}, 0, {0, 0, 0}, 0},
        // a corner exactly on the query's plane, the other two on either side: nT = (-16, 0, 0), D = (0, -256, 0), a is the end of
        // higher y. (1, 3, 0) is where the scene edge b c crosses z = 0 AND where the hypotenuse crosses x = 1: equal projections,
        // the query's candidate wins. The other end is the corner: the feature of the edge that starts at it
        {"a corner on the plane", {1, 1, 0}, {1, 3, 4}, {1, 3, -4}, true, true, {1, 3, 0}, 1, {1, 1, 0}, 3},
        // a point touch: a corner resting on the face, the rest above. The scene triangle's one candidate lies within the query's
        // chord (y = 1, x in [0, 3]) and is both ends
        {"a corner resting on the face", {1, 1, 0}, {1, 1, 4}, {2, 1, 4}, true, true, {1, 1, 0}, 3, {1, 1, 0}, 3},
        {"the resting corner as the second corner", {2, 1, 4}, {1, 1, 0}, {1, 1, 4}, true, true, {1, 1, 0}, 4, {1, 1, 0}, 4},
        // an edge resting on the face: two corners on the plane, the cut is that edge; nT = (0, -4, 0), D = (64, 0, 0)
        {"an edge resting on the face", {1, 1, 0}, {2, 1, 0}, {1, 1, 4}, true, true, {1, 1, 0}, 3, {2, 1, 0}, 4},
        // apart
        {"parallel planes one unit apart", {0, 0, 1}, {4, 0, 1}, {0, 4, 1}, false, false, {0, 0, 0}, 0, {0, 0, 0}, 0},
        {"crossing planes, the triangle beside the query", {5, -1, -1}, {5, 1, 1}, {5, 3, -1}, false, false, {0, 0, 0}, 0, {0, 0, 0}, 0},
    };
    for (const CutCase& c : cases) {
        RtCutSeg seg;
        memset(&seg, 0, sizeof seg);
        CHECK(rt_tri_triangle(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), v3(c.a), v3(c.b), v3(c.c)) == c.touch, "%s", c.what);
        const bool cut = rt_tri_cut(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), v3(c.a), v3(c.b), v3(c.c), &seg);
        CHECK(cut == c.cut, "%s", c.what);
        if (cut && c.cut) {
            CHECK(same(seg.a, c.ea) && seg.featA == c.fa, "%s: a = (%g, %g, %g) on %u", c.what, seg.a.x, seg.a.y, seg.a.z, seg.featA);
            CHECK(same(seg.b, c.eb) && seg.featB == c.fb, "%s: b = (%g, %g, %g) on %u", c.what, seg.b.x, seg.b.y, seg.b.z, seg.featB);
        }
    }
    // the record of a cut and of none
    RtCutSeg seg;
    CHECK(rt_tri_cut(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), rt_v3(1, -1, -1), rt_v3(1, 3, -1), rt_v3(1, 1, 3), &seg));
    const RtCut rec = rt_cut_record(&seg, 7, 9), none = rt_cut_no_member();
    CHECK(rec.a[0] == 1 && rec.a[1] == 0 && rec.a[2] == 0 && rec.featA == 0 && rec.b[0] == 1 && rec.b[1] == 2.5f && rec.b[2] == 0 && rec.featB == 4);
    CHECK(rec.found == 1 && rec.objectIndex == 7 && rec.triIndex == 9 && rec.reserved == 0);
    const unsigned char zeros[48] = {0};
    CHECK(memcmp(&none, zeros, 48) == 0);

    // degenerate queries are coplanar with everything: the segment through the face and the point on it touch, and have no cut
    const rt_vec3 a = rt_v3(2, 0, -2), b = rt_v3(2, 4, -2), c = rt_v3(2, 2, 2);
    CHECK(rt_tri_triangle(rt_v3(0, 2, 0), rt_v3(0, 2, 0), rt_v3(4, 2, 0), a, b, c) && !rt_tri_cut(rt_v3(0, 2, 0), rt_v3(0, 2, 0), rt_v3(4, 2, 0), a, b, c, &seg));
    CHECK(rt_tri_triangle(rt_v3(0, 2, 0), rt_v3(4, 2, 0), rt_v3(4, 2, 0), a, b, c) && !rt_tri_cut(rt_v3(0, 2, 0), rt_v3(4, 2, 0), rt_v3(4, 2, 0), a, b, c, &seg));
    CHECK(rt_tri_triangle(rt_v3(2, 2, 0), rt_v3(2, 2, 0), rt_v3(2, 2, 0), a, b, c) && !rt_tri_cut(rt_v3(2, 2, 0), rt_v3(2, 2, 0), rt_v3(2, 2, 0), a, b, c, &seg));
    // a scene triangle of NaN corners is a member of the triangle query (NaN separates nothing) and has no cut
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const rt_vec3 N = rt_v3(nan, nan, nan);
    CHECK(rt_tri_triangle(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), N, N, N) && !rt_tri_cut(v3(Q0[0]), v3(Q0[1]), v3(Q0[2]), N, N, N, &seg));

    // the canonical order of an edge's ends
    CHECK(rt_cut_before(rt_v3(0, 5, 5), rt_v3(1, 0, 0)) && rt_cut_before(rt_v3(1, 0, 5), rt_v3(1, 1, 0)) && rt_cut_before(rt_v3(1, 1, 0), rt_v3(1, 1, 1)));
    CHECK(!rt_cut_before(rt_v3(1, 1, 1), rt_v3(1, 1, 1)) && !rt_cut_before(rt_v3(1, 0, 0), rt_v3(0, 5, 5)) && !rt_cut_before(rt_v3(nan, 0, 0), rt_v3(1, 0, 0)));
}

// the end of a cut that lies on the scene triangle's edge `feat`
bool end_on(const RtCutSeg& s, uint32_t feat, rt_vec3* x) {
    if (s.featA == feat) { *x = s.a; return true; }
    if (s.featB == feat) { *x = s.b; return true; }
    return false;
}

// Two scene triangles that share the edge u v, cut by one query whose plane crosses that edge well inside the query: the end on
// the shared edge is the same bits in both cuts, for either winding of either triangle and every rotation of their corners, on
// numbers where nothing is exact
void shared_edge() {
    const rt_vec3 u = rt_v3(0.3f, 0.1f, -0.7f), v = rt_v3(0.2f, 0.9f, 0.6f), c = rt_v3(1.1f, 0.4f, 0.05f), d = rt_v3(-0.9f, 0.5f, -0.1f);
    const rt_vec3 q[3] = {rt_v3(-2.1f, -1.3f, 0.05f), rt_v3(2.3f, -1.1f, -0.1f), rt_v3(0.1f, 2.7f, 0.15f)};
    // every way to write a triangle that has the edge u v: (corners, the index of the shared edge)
    struct Tri { rt_vec3 a, b, c; uint32_t edge; };
    auto ways = [](rt_vec3 u, rt_vec3 v, rt_vec3 w, Tri out[6]) {
        out[0] = {u, v, w, 0}; out[1] = {v, w, u, 2}; out[2] = {w, u, v, 1};
        out[3] = {v, u, w, 0}; out[4] = {u, w, v, 2}; out[5] = {w, v, u, 1};
    };
    Tri one[6], two[6];
    ways(u, v, c, one);
    ways(u, v, d, two);
    for (int rot = 0; rot < 3; rot++) {
        const rt_vec3 p0 = q[rot], p1 = q[(rot + 1) % 3], p2 = q[(rot + 2) % 3];
        rt_vec3 first = rt_v3(0, 0, 0);
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) {
                RtCutSeg s1, s2;
                rt_vec3 x1, x2;
                CHECK(rt_tri_cut(p0, p1, p2, one[i].a, one[i].b, one[i].c, &s1) && rt_tri_cut(p0, p1, p2, two[j].a, two[j].b, two[j].c, &s2), "rot %d ways %d %d", rot, i, j);
                CHECK(end_on(s1, 3 + one[i].edge, &x1) && end_on(s2, 3 + two[j].edge, &x2), "rot %d ways %d %d: no end on the shared edge", rot, i, j);
                CHECK(same_bits(x1, x2), "rot %d ways %d %d: (%.9g, %.9g, %.9g) against (%.9g, %.9g, %.9g)", rot, i, j, x1.x, x1.y, x1.z, x2.x, x2.y, x2.z);
                if (i == 0 && j == 0) first = x1;
                CHECK(same_bits(x1, first));
                CHECK(s1.featA >= 3 && s1.featB >= 3 && s2.featA >= 3 && s2.featB >= 3);   // the cuts end inside the query
            }
        CHECK(std::fabs(first.x - 0.242395f) < 1e-5f && std::fabs(first.y - 0.560841f) < 1e-5f && std::fabs(first.z - 0.048867f) < 1e-5f);   // where u v meets the query's plane (float64: 0.24239482, 0.56084142, 0.04886731)
    }
}

// tri_queries_check.cpp's hand-made scene: one mesh of two triangles (the triangle (0,0,0) (4,0,0) (0,4,0), and a copy of it at
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
    // 0: an upright triangle in the plane x = 1 through all four triangles and the ball, its third corner exactly on z = 0;
    // 1: a small triangle in the plane z = 0, inside object 0's triangle 0: coplanar; 2: inside the ball: nothing; 3, 4: invalid;
    // 5: a point on object 1's triangle 1: degenerate; 6: a segment through it: degenerate
    const float q[7][9] = {{1, 1, -20, 1, 1, 20, 1, 2, 0}, {1, 1, 0, 2, 1, 0, 1, 2, 0}, {0, 0, 4, 0.5f, 0, 4, 0, 0.5f, 4},
                           {1, 1, 0, 2, nan, 0, 1, 2, 0}, {1, 1, 0, 2, 1, 0, 1, 2, inf}, {1, 1, 8, 1, 1, 8, 1, 1, 8}, {1, 1, 7, 1, 1, 7, 1, 1, 9}};
    const RtTriangleBatch all{&q[0][0], 7};
    RtCut out[7 * 8];
    uint32_t counts[7];
    memset(counts, 0x77, sizeof counts);
    memset(out, 0x77, sizeof out);
    CHECK(rt_cuts_exhaustive_host(&s, &all, 8, out, counts) == 0);
    const uint32_t want[7] = {4, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 7; i++) CHECK(counts[i] == want[i], "triangle %d: %u", i, counts[i]);
    const unsigned char zeros[48] = {0};
    // query 0: object 0's triangles 0 and 1 (z = 0, -8), then object 1's (z = 16, 8); never the sphere
    const float z[4] = {0, -8, 16, 8};
    for (uint32_t e = 0; e < 4; e++) {
        const RtCut& r = out[e];
        CHECK(r.found == 1 && r.objectIndex == e / 2 && r.triIndex == e % 2 && r.reserved == 0, "entry %u", e);
        CHECK(r.a[0] == 1 && r.b[0] == 1 && r.a[2] == z[e] && r.b[2] == z[e], "entry %u: (%g %g %g) (%g %g %g)", e, r.a[0], r.a[1], r.a[2], r.b[0], r.b[1], r.b[2]);
        CHECK(r.featA < 3 && r.featB < 3, "entry %u: the query's chord lies inside the scene triangle's", e);
    }
    // nQ = (-40, 0, 0), nT = (0, 0, 16), D = (0, 640, 0): a is the end of lower y, where the edge p q crosses; b is the corner r
    CHECK(out[0].a[1] == 1 && out[0].featA == 0 && out[0].b[1] == 2 && out[0].featB == 2);
    for (uint32_t e = 4; e < 8; e++) CHECK(memcmp(&out[e], zeros, 48) == 0);
    for (int i = 1; i < 7; i++)
        for (uint32_t e = 0; e < 8; e++) CHECK(memcmp(&out[i * 8 + e], zeros, 48) == 0, "triangle %d entry %u", i, e);
    // counts are the same for every k, and a smaller k is the head of the same list
    for (uint32_t k : {0u, 1u, 2u}) {
        RtCut fewer[7 * 2];
        uint32_t c2[7];
        CHECK(rt_cuts_exhaustive_host(&s, &all, k, k ? fewer : nullptr, c2) == 0 && memcmp(c2, counts, sizeof counts) == 0);
        for (int i = 0; i < 7; i++) CHECK(memcmp(&fewer[i * k], &out[i * 8], k * sizeof(RtCut)) == 0, "k %u triangle %d", k, i);
    }

    // refusals of the loop itself
    CHECK(rt_cuts_exhaustive_host(nullptr, &all, 1, out, counts) == -1);
    CHECK(rt_cuts_exhaustive_host(&s, nullptr, 1, out, counts) == -1);
    CHECK(rt_cuts_exhaustive_host(&s, &all, 9, out, counts) == -1);
    CHECK(rt_cuts_exhaustive_host(&s, &all, 1, nullptr, counts) == -1);
    CHECK(rt_cuts_exhaustive_host(&s, &all, 1, out, nullptr) == -1);
    const RtTriangleBatch noCorners{nullptr, 1}, big{&q[0][0], 1u << 30}, empty{nullptr, 0};
    CHECK(rt_cuts_exhaustive_host(&s, &noCorners, 1, out, counts) == -1);
    CHECK(rt_cuts_exhaustive_host(&s, &big, 1, out, counts) == -1);
    CHECK(rt_cuts_exhaustive_host(&s, &empty, 8, nullptr, nullptr) == 0);
    CHECK(rt_cuts_exhaustive_host(&s, &empty, 9, nullptr, nullptr) == -1);
    nodes[2].index = 2;   // a leaf range past the triangles
    CHECK(rt_cuts_exhaustive_host(&s, &all, 1, out, counts) == -1);
    nodes[2].index = 1;
    objs[1].bvhIndex = 3;   // a root past the nodes
    CHECK(rt_cuts_exhaustive_host(&s, &all, 1, out, counts) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    staging();
    rule_table();
    shared_edge();
    hand_made_scene();
    return check_finish("cut queries ok");
}
