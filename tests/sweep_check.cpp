// sweep_check.cpp — what the sphere sweeps refuse (ray_tracer_amd/csrc/sweep_queries.h: check_sweep_query), in their order and with
// their messages, the block and byte arithmetic of a batch (sweep_shape) at n = 0, 1, ... 2^30 - 1, the stack choice (sweep_stack)
// at depths 24, 25, 64 and 65, the part layout of the _host form for 65 rays (stage_layout), the rule (include/rt_sweep.h) on
// hand cases, each against its closed form, and rt_sweep_exhaustive_host on a hand-made scene, on the CPU, built with plain g++ by
// tests/test_sweep_host.py. No array of a batch is ever dereferenced by the checks: the addresses are made up. Prints "sweep ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "host_staging.h"
#include "sweep_queries.h"
#include "rt_sweep.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }
const float INF = std::numeric_limits<float>::infinity(), NaN = std::numeric_limits<float>::quiet_NaN();

void refusals() {
    float* const O = at<float>(0x10000000u);
    float* const D = at<float>(0x20000000u);
    float* const R = at<float>(0x30000000u);
    float* const T = at<float>(0x40000000u);
    void* const out = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_sweep", "rt_query_sweep_host"}) {
        const std::string f(fn);
        const RtSweepBatch ok{O, D, R, T, 1000}, noLimit{O, D, R, nullptr, 1000};
        CHECK(check_sweep_query(fn, true, &ok, out).empty());
        CHECK(check_sweep_query(fn, true, &noLimit, out).empty());
        CHECK(check_sweep_query(fn, false, &ok, out) == f + " before rt_upload_scene");
        CHECK(check_sweep_query(fn, true, nullptr, out) == f + ": the batch is NULL");
        const std::string required = f + ": origins, dirs, radius and the output are required";
        const RtSweepBatch noO{nullptr, D, R, T, 5}, noD{O, nullptr, R, T, 5}, noR{O, D, nullptr, T, 5};
        CHECK(check_sweep_query(fn, true, &noO, out) == required);
        CHECK(check_sweep_query(fn, true, &noD, out) == required);
        CHECK(check_sweep_query(fn, true, &noR, out) == required);
        CHECK(check_sweep_query(fn, true, &ok, nullptr) == required);
        const RtSweepBatch big{O, D, R, T, 1u << 30}, most{O, D, R, T, (1u << 30) - 1u}, huge{O, D, R, T, 0xffffffffu};
        CHECK(check_sweep_query(fn, true, &big, out) == f + ": a batch of 1073741824 rays does not fit the 30 bits of a slot id");
        CHECK(check_sweep_query(fn, true, &huge, out) == f + ": a batch of 4294967295 rays does not fit the 30 bits of a slot id");
        CHECK(check_sweep_query(fn, true, &most, out).empty());
        // n == 0 succeeds whatever the pointers are, but not without a scene or a batch
        const RtSweepBatch none{nullptr, nullptr, nullptr, nullptr, 0};
        CHECK(check_sweep_query(fn, true, &none, nullptr).empty());
        CHECK(check_sweep_query(fn, false, &none, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, the pointers, the size
        const RtSweepBatch bigNoR{O, D, nullptr, T, 1u << 30};
        CHECK(check_sweep_query(fn, false, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_sweep_query(fn, true, nullptr, nullptr) == f + ": the batch is NULL");
        CHECK(check_sweep_query(fn, true, &bigNoR, out) == required);
        CHECK(check_sweep_query(fn, true, &big, nullptr) == required);
    }
}

void arithmetic() {
    CHECK(sizeof(RtSweep) == 64 && offsetof(RtSweep, triIndex) == 16 && offsetof(RtSweep, gap) == 28 && offsetof(RtSweep, point) == 32);
    CHECK(offsetof(RtSweep, startsInContact) == 44 && offsetof(RtSweep, normal) == 48 && offsetof(RtSweep, _pad) == 60);
    const SweepShape zero = sweep_shape(0, 256);
    CHECK(zero.blocks == 0 && zero.vecBytes == 0 && zero.scalarBytes == 0 && zero.outBytes == 0);
    struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
    for (const Row& r : rows) {
        const SweepShape s = sweep_shape(r.n, 256);
        CHECK(s.blocks == r.blocks && s.vecBytes == (size_t)12 * r.n && s.scalarBytes == (size_t)4 * r.n && s.outBytes == (size_t)64 * r.n);
    }
    CHECK(sweep_shape((1u << 30) - 1u, 256).outBytes == 68719476672ull);   // past 32 bits: size_t arithmetic

    std::string e;
    CHECK(sweep_stack("f", 0, &e) == 24 && sweep_stack("f", 24, &e) == 24 && sweep_stack("f", 25, &e) == 64 && sweep_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(sweep_stack("rt_query_sweep", 65, &e) == 0);
    CHECK(e == "rt_query_sweep: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_sweep_spheres");
}

// origins, dirs, radius, tmax, out of the _host form for 65 rays, by the one rule of host_staging.h
void staging() {
    struct Case { bool limits; size_t offset[5], total; } const cases[] = {
        {true, {0, 1024, 2048, 2560, 3072}, 7424},     // 780, 780, 260, 260, 4160 bytes, each from a multiple of 256
        {false, {0, 1024, 2048, 2560, 2560}, 6912}};   // no tmax: the part is absent, its offset the next one's
    for (const Case& c : cases) {
        const SweepShape s = sweep_shape(65, 256);
        const size_t bytes[5] = {s.vecBytes, s.vecBytes, s.scalarBytes, c.limits ? s.scalarBytes : 0, s.outBytes};
        CHECK(bytes[0] == 780 && bytes[2] == 260 && bytes[4] == 4160);
        const StageLayout g = stage_layout(bytes, 5);
        CHECK(g.ok && g.bytes == c.total, "%zu", g.bytes);
        for (int p = 0; p < 5; p++) CHECK(g.offset[p] == c.offset[p], "part %d: %zu", p, g.offset[p]);
    }
}

bool near(float got, double want, double tol) { return std::fabs((double)got - want) <= tol; }

struct Tri { rt_vec3 a, b, c; };
// the time of a triangle, or -1
float tri_time(rt_vec3 o, rt_vec3 d, float R, const Tri& t, float* d2 = nullptr, float* u = nullptr, float* v = nullptr) {
    float tt, dd2, uu, vv;
    if (!rt_sweep_triangle(o, d, rt_dot(d, d), R, t.a, t.b, t.c, &tt, &dd2, &uu, &vv)) return -1.f;
    if (d2) *d2 = dd2;
    if (u) *u = uu;
    if (v) *v = vv;
    return tt;
}

void rule_start_and_key() {
    bool s;
    CHECK(rt_sweep_start(rt_v3(0, 0, 1), 1.f, false, 0.f, &s) == INF && s);
    CHECK(rt_sweep_start(rt_v3(0, 0, 1), 1.f, true, 2.f, &s) == 2.f && s);
    for (float bad : {0.f, -0.f, -1.f, NaN, INF}) { rt_sweep_start(rt_v3(0, 0, 1), bad, false, 0.f, &s); CHECK(!s, "radius %g", (double)bad); }
    for (float bad : {0.f, -0.f, -1.f, NaN}) { rt_sweep_start(rt_v3(0, 0, 1), 1.f, true, bad, &s); CHECK(!s, "limit %g", (double)bad); }
    rt_sweep_start(rt_v3(0, 0, 1), 1.f, true, INF, &s); CHECK(s);
    rt_sweep_start(rt_v3(0, 0, 0), 1.f, false, 0.f, &s); CHECK(!s);
    rt_sweep_start(rt_v3(0, -0.f, 0), 1.f, false, 0.f, &s); CHECK(!s);
    rt_sweep_start(rt_v3(INF, 0, 0), 1.f, false, 0.f, &s); CHECK(!s);
    rt_sweep_start(rt_v3(NaN, 0, 1), 1.f, false, 0.f, &s); CHECK(!s);
    rt_sweep_start(rt_v3(3e19f, 3e19f, 0), 1.f, false, 0.f, &s); CHECK(!s);   // dot(d, d) overflows
    // the key: t below the limit, then the lower time, spheres before triangles, the lower index
    const uint32_t s0 = rt_hits_sphere_word(0, false), s5 = rt_hits_sphere_word(5, false);
    CHECK(rt_sweep_replaces(1.f, 3, 7, INF, INF, RT_HITS_EMPTY, 0) && rt_sweep_replaces(1.f, s5, 0, 2.f, 2.f, RT_HITS_EMPTY, 0));
    CHECK(!rt_sweep_replaces(2.f, 3, 7, 2.f, 2.f, RT_HITS_EMPTY, 0) && !rt_sweep_replaces(2.f, s0, 0, 2.f, 2.f, RT_HITS_EMPTY, 0));   // [0, T): T itself is out
    CHECK(!rt_sweep_replaces(NaN, 3, 7, INF, INF, RT_HITS_EMPTY, 0));
    CHECK(rt_sweep_replaces(1.f, s5, 0, INF, 1.f, 0, 0) && !rt_sweep_replaces(1.f, 0, 0, INF, 1.f, s5, 0));
    CHECK(rt_sweep_replaces(1.f, s0, 0, INF, 1.f, s5, 0) && rt_sweep_replaces(1.f, 2, 9, INF, 1.f, 3, 1) && rt_sweep_replaces(1.f, 3, 1, INF, 1.f, 3, 9));
    CHECK(!rt_sweep_replaces(1.f, 3, 1, INF, 1.f, 3, 1) && rt_sweep_replaces(0.5f, 9, 9, INF, 1.f, s0, 0) && !rt_sweep_replaces(1.5f, s0, 0, INF, 1.f, 9, 9));
    const RtSweep none = rt_sweep_not_found();
    RtSweep zero;
    memset(&zero, 0, sizeof zero);
    zero.t = RT_MISS_DST;
    CHECK(memcmp(&none, &zero, sizeof zero) == 0);
}

void rule_triangle() {
    const Tri T{rt_v3(0, 0, 0), rt_v3(4, 0, 0), rt_v3(0, 4, 0)};
    float d2, u, v;
    // face: straight down on (1, 1): the plane z = 0 less the radius
    CHECK(tri_time(rt_v3(1, 1, 5), rt_v3(0, 0, -1), 1.f, T, &d2, &u, &v) == 4.f && d2 == 1.f && u == 0.25f && v == 0.25f);
    CHECK(tri_time(rt_v3(1, 1, 5), rt_v3(0, 0, -2), 1.f, T) == 2.f);            // t in units of |d|
    CHECK(tri_time(rt_v3(1, 1, -5), rt_v3(0, 0, 1), 1.f, T) == 4.f);            // no front or back
    CHECK(tri_time(rt_v3(1, 1, 5), rt_v3(0, 0, 1), 1.f, T) == -1.f);            // outside the slab and leaving
    CHECK(tri_time(rt_v3(1, 1, 5), rt_v3(1, 0, 0), 1.f, T) == -1.f);            // outside the slab and level with it
    CHECK(tri_time(rt_v3(1, 1, 0.5f), rt_v3(1, 0, 0), 1.f, T, &d2) == 0.f && d2 == 0.25f);   // starts in contact
    CHECK(tri_time(rt_v3(1, 1, 1), rt_v3(0, 0, 1), 1.f, T) == 0.f);             // touching at t = 0, leaving
    // oblique on the face: (1, 1, 5) + t (0.25, 0.25, -1) reaches z = 1 at t = 4 over (2, 2), which is the hypotenuse's midpoint
    CHECK(tri_time(rt_v3(1, 1, 5), rt_v3(0.25f, 0.25f, -1), 1.f, T, &d2, &u, &v) == 4.f && u == 0.5f && v == 0.5f);
    // edge ab from the side, in the triangle's plane: y = -1 at t = 2
    CHECK(tri_time(rt_v3(2, -3, 0), rt_v3(0, 1, 0), 1.f, T, &d2, &u, &v) == 2.f && d2 == 1.f && u == 0.5f && v == 0.f);
    // edge ab from below and outside, 45 degrees: the centre (2, -3 + t, -3 + t) is at sqrt(2) (3 - t) from the edge: t = 3 - 1 / sqrt(2)
    CHECK(near(tri_time(rt_v3(2, -3, -3), rt_v3(0, 1, 1), 1.f, T), 3.0 - std::sqrt(0.5), 1e-6));
    // vertex a along (3, 4, 0): the centre reaches distance 1 of the corner at t = 1 - 1 / 5
    CHECK(near(tri_time(rt_v3(-3, -4, 0), rt_v3(3, 4, 0), 1.f, T, &d2, &u, &v), 0.8, 1e-6) && u == 0.f && v == 0.f && near(d2, 1.0, 1e-5));
    // vertex b from beyond it
    CHECK(near(tri_time(rt_v3(10, -3, 0), rt_v3(-1, 0.5f, 0), 0.5f, T, &d2, &u, &v), 6.0 - std::sqrt(0.2), 2e-6) && u == 1.f && v == 0.f);
    // inside the slab but off the triangle: at height 0.5 towards the hypotenuse x + y = 4 along (-1, -1, 0):
    // ((16 - 2 t) / sqrt(2))^2 + 0.25 = 1, t = 8 - sqrt(0.375)
    CHECK(near(tri_time(rt_v3(10, 10, 0.5f), rt_v3(-1, -1, 0), 1.f, T, &d2, &u, &v), 8.0 - std::sqrt(0.375), 2e-6) && near(u, 0.5, 1e-6) && near(v, 0.5, 1e-6));
    // a ray along edge ab at y = -0.5: the cylinder is left out, edge ac's entry at t = 4 lies off the edge, vertex a decides:
    // (t - 5)^2 + 0.25 = 1
    CHECK(near(tri_time(rt_v3(-5, -0.5f, 0), rt_v3(1, 0, 0), 1.f, T, &d2, &u, &v), 5.0 - std::sqrt(0.75), 1e-6) && u == 0.f && v == 0.f);
    // ... and at y = -2 it passes
    CHECK(tri_time(rt_v3(-5, -2, 0), rt_v3(1, 0, 0), 1.f, T) == -1.f);
    // passes the corner b by more than R
    CHECK(tri_time(rt_v3(6, -3, 0), rt_v3(0, 1, 0), 1.f, T) == -1.f);
    // behind the origin: no contact ahead
    CHECK(tri_time(rt_v3(2, -3, 0), rt_v3(0, -1, 0), 1.f, T) == -1.f);
    // an origin 1e3 away: the same contact to the step's rounding (u t ~ 6e-5), not to R^2's cancellation
    CHECK(near(tri_time(rt_v3(2, -1003, 0), rt_v3(0, 1, 0), 1.f, T), 1002.0, 3e-4));
    CHECK(near(tri_time(rt_v3(1, 1, 1000), rt_v3(0, 0, -1), 0.01f, T), 999.99, 3e-4));

    // degenerate triangles: a point is its vertex ball, a segment its capsule
    const Tri P{rt_v3(1, 2, 3), rt_v3(1, 2, 3), rt_v3(1, 2, 3)};
    CHECK(tri_time(rt_v3(1, 2, 8), rt_v3(0, 0, -1), 1.f, P, &d2, &u, &v) == 4.f && d2 == 1.f);
    CHECK(tri_time(rt_v3(3, 2, 8), rt_v3(0, 0, -1), 1.f, P) == -1.f);
    const Tri S{rt_v3(0, 0, 0), rt_v3(4, 0, 0), rt_v3(4, 0, 0)};
    CHECK(tri_time(rt_v3(2, -3, 0), rt_v3(0, 1, 0), 1.f, S, &d2) == 2.f && d2 == 1.f);
    CHECK(near(tri_time(rt_v3(-3, -4, 0), rt_v3(3, 4, 0), 1.f, S), 0.8, 1e-6));
    const Tri L{rt_v3(0, 0, 0), rt_v3(2, 0, 0), rt_v3(4, 0, 0)};   // collinear
    CHECK(tri_time(rt_v3(3, -3, 0), rt_v3(0, 1, 0), 1.f, L) == 2.f);
}

void rule_sphere() {
    const rt_vec3 c = rt_v3(0, 0, 0);
    float t, d2;
    // from outside: the ball r + R
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 10), rt_v3(0, 0, -1), 1.f, 1.f, c, 2.f, &t, &d2) && t == 7.f && d2 == 1.f);
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 10), rt_v3(0, 0, -2), 4.f, 1.f, c, 2.f, &t, &d2) && t == 3.5f);
    CHECK(!rt_sweep_sphere(rt_v3(0, 0, 10), rt_v3(0, 0, 1), 1.f, 1.f, c, 2.f, &t, &d2));       // leaving
    CHECK(!rt_sweep_sphere(rt_v3(3.5f, 0, 10), rt_v3(0, 0, -1), 1.f, 1.f, c, 2.f, &t, &d2));   // passes
    CHECK(rt_sweep_sphere(rt_v3(3, 0, 10), rt_v3(0, 0, -1), 1.f, 1.f, c, 2.f, &t, &d2) && t == 10.f);   // tangent to r + R
    // from inside the shell r - R: its exit; the surface is met from inside
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 0), rt_v3(0, 0, 1), 1.f, 1.f, c, 2.f, &t, &d2) && t == 1.f && d2 == 1.f);
    CHECK(rt_sweep_sphere(rt_v3(0, 0, -0.5f), rt_v3(0, 0, 1), 1.f, 1.f, c, 2.f, &t, &d2) && t == 1.5f);
    // between the two: already touching
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 1.5f), rt_v3(0, 0, 1), 1.f, 1.f, c, 2.f, &t, &d2) && t == 0.f && d2 == 0.25f);
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 2.5f), rt_v3(1, 0, 0), 1.f, 1.f, c, 2.f, &t, &d2) && t == 0.f && d2 == 0.25f);
    // a sphere no larger than the ball has no inside
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 0), rt_v3(0, 0, 1), 1.f, 1.f, c, 0.5f, &t, &d2) && t == 0.f && d2 == 0.25f);
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 0), rt_v3(0, 0, 1), 1.f, 1.f, c, 1.f, &t, &d2) && t == 0.f && d2 == 1.f);
    // far away
    CHECK(rt_sweep_sphere(rt_v3(0, 0, 1000), rt_v3(0, 0, -1), 1.f, 0.01f, c, 2.f, &t, &d2) && near(t, 997.99, 3e-4));
    // the records
    const RtSweep out = rt_sweep_sphere_record(rt_v3(0, 0, 10), rt_v3(0, 0, -1), 7.f, c, 2.f, 3);
    CHECK(out.t == 7.f && out.found == 1 && out.isSphere == 1 && out.objectIndex == 3 && out.triIndex == 0 && out.uv[0] == 0.f && out.uv[1] == 0.f && out.gap == 1.f);
    CHECK(out.point[0] == 0.f && out.point[1] == 0.f && out.point[2] == 2.f && out.startsInContact == 0 && out.normal[2] == 1.f && out.normal[0] == 0.f && out._pad == 0);
    const RtSweep in = rt_sweep_sphere_record(rt_v3(0, 0, 0), rt_v3(0, 0, 1), 1.f, c, 2.f, 0);
    CHECK(in.point[2] == 2.f && in.normal[2] == -1.f && in.gap == 1.f);         // from the point towards the centre: inwards
    const Tri T{rt_v3(0, 0, 0), rt_v3(4, 0, 0), rt_v3(0, 4, 0)};
    const RtSweep tr = rt_sweep_triangle_record(rt_v3(1, 1, 5), rt_v3(0, 0, -1), 4.f, T.a, T.b, T.c, 2, 11);
    CHECK(tr.t == 4.f && tr.found == 1 && tr.isSphere == 0 && tr.objectIndex == 2 && tr.triIndex == 11 && tr.uv[0] == 0.25f && tr.uv[1] == 0.25f && tr.gap == 1.f);
    CHECK(tr.point[0] == 1.f && tr.point[1] == 1.f && tr.point[2] == 0.f && tr.normal[2] == 1.f && tr.startsInContact == 0 && tr._pad == 0);
    const RtSweep on = rt_sweep_triangle_record(rt_v3(1, 1, 0), rt_v3(0, 3, -4), 0.f, T.a, T.b, T.c, 0, 0);   // the centre on the surface
    CHECK(on.gap == 0.f && on.startsInContact == 1 && near(on.normal[1], -0.6, 1e-7) && near(on.normal[2], 0.8, 1e-7) && on.normal[0] == 0.f);
}

void rule_boxes() {
    const rt_vec3 lo = rt_v3(-1, -1, -1), hi = rt_v3(1, 1, 1);
    float e, x;
    rt_sweep_box(lo, hi, rt_v3(0, 0, 10), rt_sweep_inv(rt_v3(0, 0, -1)), 0.5f, &e, &x);
    CHECK(e == 8.5f && x == 11.5f && rt_sweep_box_open(e, x, INF) && rt_sweep_box_open(e, x, 8.5f) && !rt_sweep_box_open(e, x, 8.4f));
    rt_sweep_box(lo, hi, rt_v3(1.4f, 0, 10), rt_sweep_inv(rt_v3(0, 0, -1)), 0.5f, &e, &x);   // an axis it does not move along, inside the grown slab
    CHECK(e == 8.5f && x == 11.5f);
    rt_sweep_box(lo, hi, rt_v3(1.6f, 0, 10), rt_sweep_inv(rt_v3(0, 0, -1)), 0.5f, &e, &x);   // ... and outside it
    CHECK(!rt_sweep_box_open(e, x, INF));
    rt_sweep_box(lo, hi, rt_v3(0, 0, 10), rt_sweep_inv(rt_v3(0, 0, 1)), 0.5f, &e, &x);       // behind
    CHECK(x < 0.f && !rt_sweep_box_open(e, x, INF));
    rt_sweep_box(lo, hi, rt_v3(0, 0, 0), rt_sweep_inv(rt_v3(1, 1, 1)), 0.5f, &e, &x);        // inside
    CHECK(e == -1.5f && x == 1.5f && rt_sweep_box_open(e, x, 0.f));
    rt_sweep_box(lo, hi, rt_v3(0, 0, 10), rt_sweep_inv(rt_v3(0, 0, -1)), INF, &e, &x);       // sMin == 0: nothing is discarded
    CHECK(rt_sweep_box_open(e, x, 0.f));
    rt_sweep_box(lo, hi, rt_v3(5, 0, 10), rt_sweep_inv(rt_v3(0, 0, -1)), NaN, &e, &x);       // an unbounded object: likewise
    CHECK(rt_sweep_box_open(e, x, 0.f));
    rt_sweep_box(rt_v3(-INF, -INF, -INF), rt_v3(INF, INF, INF), rt_v3(5, 0, 10), rt_sweep_inv(rt_v3(0, 0, -1)), 0.5f, &e, &x);   // the world box of an object without one
    CHECK(rt_sweep_box_open(e, x, 0.f));
    // the pad: R + sigma + eta over sMin and the ray's own rounding; never below R / sMin
    CHECK(rt_sweep_pad(0.5f, 3.f, 2.f, 1.f, 0.f, 1.f) > 0.5f && rt_sweep_pad(0.5f, 3.f, 2.f, 1.f, 0.f, 1.f) < 0.5001f);
    CHECK(rt_sweep_pad(0.5f, 3.f, 2.f, 0.25f, 0.f, 0.25f) > 2.f && rt_sweep_pad(0.5f, 3.f, 2.f, 0.25f, 1e-6f, 0.25f) > rt_sweep_pad(0.5f, 3.f, 2.f, 0.25f, 0.f, 0.25f));
    CHECK(rt_sweep_pad(0.5f, 3.f, 2.f, 0.f, 0.f, 0.f) == INF);
}

// A hand-made scene: one mesh of two triangles (the unit right triangle in z = 0, and a copy of it at z = -5) under an interior
// root with two leaves, placed twice by the identity, so the two objects' triangles coincide; a sphere of radius 1 about
// (0.25, 0.25, 3); and a zeroed sphere slot.
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

    // four rays down the line x = y = 0.25 and one that moves away from everything
    const float o[5][3] = {{0.25f, 0.25f, 1.25f}, {0.25f, 0.25f, 1.75f}, {0.25f, 0.25f, -1.f}, {0.25f, 0.25f, 3.f}, {5, 5, 1}};
    const float d[5][3] = {{0, 0, -1}, {0, 0, -1}, {0, 0, -2}, {0, 0, 1}, {1, 0, 0}};
    const float R[5] = {0.25f, 0.5f, 0.5f, 0.25f, 0.5f};
    RtSweep out[5];
    const RtSweepBatch all{&o[0][0], &d[0][0], R, nullptr, 5};
    CHECK(rt_sweep_exhaustive_host(&s, &all, out) == 0);
    // 0: the sphere is 0.75 away and behind; the coincident triangles of objects 0 and 1 tie at t = 1: the lower object
    CHECK(out[0].found == 1 && out[0].t == 1.f && out[0].isSphere == 0 && out[0].objectIndex == 0 && out[0].triIndex == 0 && out[0].gap == 0.25f);
    CHECK(out[0].uv[0] == 0.25f && out[0].uv[1] == 0.25f && out[0].point[2] == 0.f && out[0].normal[2] == 1.f && out[0].startsInContact == 0);
    // 1: starts within 0.5 of the sphere's lowest point: t = 0, the sphere, whatever lies ahead
    CHECK(out[1].found == 1 && out[1].t == 0.f && out[1].isSphere == 1 && out[1].objectIndex == 0 && out[1].startsInContact == 1 && out[1].gap == 0.25f);
    CHECK(out[1].point[2] == 2.f && out[1].normal[2] == -1.f);
    // 2: between the two sheets, going down at speed 2: z = -4.5 at t = 1.75, triangle 1 of object 0
    CHECK(out[2].found == 1 && out[2].t == 1.75f && out[2].objectIndex == 0 && out[2].triIndex == 1 && out[2].point[2] == -5.f);
    // 3: at the sphere's centre: inside the shell 1 - 0.25, out through it at t = 0.75
    CHECK(out[3].found == 1 && out[3].t == 0.75f && out[3].isSphere == 1 && out[3].point[2] == 4.f && out[3].normal[2] == -1.f && out[3].gap == 0.25f);
    const RtSweep none = rt_sweep_not_found();
    CHECK(memcmp(&out[4], &none, sizeof none) == 0);

    // limits: [0, T)
    struct Limit { float T; bool found; } const limits[] = {{1.f, false}, {1.5f, true}, {0.5f, false}, {INF, true}, {0.f, false}, {-1.f, false}, {NaN, false}};
    for (const Limit& l : limits) {
        const RtSweepBatch one{&o[0][0], &d[0][0], R, &l.T, 1};
        RtSweep got;
        CHECK(rt_sweep_exhaustive_host(&s, &one, &got) == 0);
        CHECK(memcmp(&got, l.found ? &out[0] : &none, sizeof got) == 0, "limit %g", (double)l.T);
    }
    // radii that mean no search
    for (float bad : {0.f, -0.f, -1.f, NaN}) {
        const RtSweepBatch one{&o[1][0], &d[1][0], &bad, nullptr, 1};
        RtSweep got;
        CHECK(rt_sweep_exhaustive_host(&s, &one, &got) == 0 && memcmp(&got, &none, sizeof got) == 0, "radius %g", (double)bad);
    }
    const float still[3] = {0, 0, 0};
    const RtSweepBatch noDir{&o[1][0], still, R, nullptr, 1};
    RtSweep got;
    CHECK(rt_sweep_exhaustive_host(&s, &noDir, &got) == 0 && memcmp(&got, &none, sizeof got) == 0);

    // refusals of the loop itself
    CHECK(rt_sweep_exhaustive_host(nullptr, &all, out) == -1);
    CHECK(rt_sweep_exhaustive_host(&s, nullptr, out) == -1);
    CHECK(rt_sweep_exhaustive_host(&s, &all, nullptr) == -1);
    const RtSweepBatch noO{nullptr, &d[0][0], R, nullptr, 1}, noD{&o[0][0], nullptr, R, nullptr, 1}, noR{&o[0][0], &d[0][0], nullptr, nullptr, 1};
    const RtSweepBatch big{&o[0][0], &d[0][0], R, nullptr, 1u << 30}, empty{nullptr, nullptr, nullptr, nullptr, 0};
    CHECK(rt_sweep_exhaustive_host(&s, &noO, out) == -1 && rt_sweep_exhaustive_host(&s, &noD, out) == -1 && rt_sweep_exhaustive_host(&s, &noR, out) == -1);
    CHECK(rt_sweep_exhaustive_host(&s, &big, out) == -1);
    CHECK(rt_sweep_exhaustive_host(&s, &empty, nullptr) == 0);
    nodes[2].index = 2;   // a leaf range past the triangles
    CHECK(rt_sweep_exhaustive_host(&s, &all, out) == -1);
    nodes[2].index = 1;
    objs[1].bvhIndex = 3;   // a root past the nodes
    CHECK(rt_sweep_exhaustive_host(&s, &all, out) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    staging();
    rule_start_and_key();
    rule_triangle();
    rule_sphere();
    rule_boxes();
    hand_made_scene();
    return check_finish("sweep ok");
}
