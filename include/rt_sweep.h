/*
 * rt_sweep.h — the rule of the sphere sweeps (rt_query_sweep, rt_sweep_exhaustive_host): when a ball of radius R whose centre
 * moves along o + t d first touches a triangle or a sphere, and the record of that contact. One text for both sides, under
 * rt_det_math.h's discipline (RT_HD, -ffp-contract=off, rt_* math only), the way rt_point_query.h and rt_ray_hits.h are shared:
 * the device kernel (k_sweep_spheres) and the exhaustive host loop compile these very functions, so a primitive's contact time
 * has the same 32 bits on both.
 *
 * Declared semantics ("Sphere sweeps"). The surfaces are rt_query_nearest's: every sphere with
 * rt_sphere_is_surface(r) and every triangle of every object, its world corners placed as k_nearest_points places them. They are
 * surfaces, not solids. Ray i asks for the least t in [0, T) at which the centre is within R of a surface; T = tmax[i], +inf when
 * tmax is NULL. R NaN or <= 0, T NaN or <= 0, dot(d, d) not finite or not > 0: no search (rt_sweep_start).
 *
 * Per primitive the rule gives a time or none, as a function of the ray, the radius and the primitive alone:
 *  - Triangle. The slab of half-thickness R about its plane: a centre outside it and not approaching never touches: none. Else
 *    the slab entry time (0 inside) is the face candidate, and the answer when it is accepted. Else the entry times of the three
 *    vertex balls and of the three edge cylinders (each valid when the segment parameter at contact lies within the edge; an edge
 *    the ray runs along, or of no length, leaves it to the vertices) are tried in ascending order, and the first accepted one is
 *    the answer. An entry below 0 with an exit >= 0 counts as 0.
 *  - Sphere of radius r. From outside the ball r + R: its entry. Inside the ball r - R (r > R): its exit. Between: 0.
 *  - Every quadratic is solved about the point of the line nearest the primitive (rt_sweep_ball, rt_sweep_edge_time), not about o:
 *    with coefficients taken at an origin 1e3 away the cancellation in |m|^2 - R^2 alone is of the size of R^2.
 *  - Acceptance. A candidate t counts only if the point queries' own distance from the centre fl(o + t d) to the primitive,
 *    rt_point_triangle or rt_point_sphere, is <= fl((R + sigma)^2), sigma = RT_SWEEP_SIGMA x the scale of the contact: the largest
 *    |coordinate| of that centre, of the corners (|c| + r of a sphere) and of the step t d itself (the rounding of t moves the
 *    centre by u |t d|, which the centre's own coordinates do not bound when the origin is far). That call yields the record's
 *    uv, point and gap, and it is what the pruning of the device descent is derived from.
 * Ray i keeps (best, key), started at T. A primitive replaces the answer when its t is < T and rt_hits_before of
 * {t, primitive word, triangle} against the answer so far: the lower time, then spheres before triangles, then the lower index.
 * The key is total, so the answer does not depend on the visiting order.
 */
#ifndef RT_SWEEP_H
#define RT_SWEEP_H

#include "rt_amd.h"
#include "rt_point_query.h"
#include "rt_ray_hits.h"

/* 48 u, u = 2^-24, in units of the contact's scale ("Sphere sweeps", counts them): what separates the candidate's
 * solve from the measurement at the same fp32 centre and corners once the barycentrics name the right point: 27.7 u
 * rt_point_triangle's own roundings, 7 u the centre fl(o + t d) as a vector where the candidate was solved and where it is
 * measured, 12 u the candidate's chain (the line parameter of the nearest point, that point, its offset from the primitive, the
 * half chord, t): 46.7. The conditioning of the barycentrics themselves is not in it; the tests' delta carries that. */
#define RT_SWEEP_SIGMA 2.86102294921875e-06f
/* an edge counts as parallel to the ray when sin^2 of their angle is at most 2^-20: the cylinder's time is then worse than the
 * vertex balls' by more than the rule can use, and an edge the ray runs along exactly leaves rounding noise for a direction */
#define RT_SWEEP_PARALLEL 9.5367431640625e-07f
/* box times carry 5 roundings: a box is entered when entry * RT_SWEEP_TDOWN <= best (entry > 0) */
#define RT_SWEEP_TDOWN 0.999999523162841796875f   /* 1 - 2^-21 */
#define RT_SWEEP_GROW 1.00000095367431640625f     /* 1 + 2^-20: the pad's own roundings */
#define RT_SWEEP_HUGE 3.0e38f

RT_HD float rt_sweep_inf(void) { return rt_u2f(0x7f800000u); }
RT_HD float rt_max3abs(rt_vec3 v) { return rt_max(rt_max(rt_abs(v.x), rt_abs(v.y)), rt_abs(v.z)); }

/* the bound a search starts with; *search = false: the not-found record without a search */
RT_HD float rt_sweep_start(rt_vec3 d, float R, bool hasLimit, float tmax, bool* search) {
    float dd = rt_dot(d, d);
    float T = hasLimit ? tmax : rt_sweep_inf();
    *search = (R > 0.f) && (T > 0.f) && (dd > 0.f) && !rt_isinf(dd) && !rt_isinf(R);
    return T;
}

RT_HD rt_vec3 rt_sweep_centre(rt_vec3 o, rt_vec3 d, float t) { return rt_add(o, rt_scale(d, t)); }

/* sigma of a contact: centre at t, the largest |coordinate| of the primitive (cmax), the step t d */
RT_HD float rt_sweep_sigma(rt_vec3 centre, rt_vec3 d, float t, float cmax) {
    return RT_SWEEP_SIGMA * rt_max(rt_max(rt_max3abs(centre), cmax), rt_abs(t) * rt_max3abs(d));
}
RT_HD bool rt_sweep_accepts(float d2, float R, float sigma) {
    float reach = R + sigma;
    return d2 <= reach * reach;
}

/* [t0, t1]: the times the line is within sqrt(rho2) of c. Solved about p = o + s d, the point of the line nearest c. Both times
 * are always written (selects, no branches: the device runs this seven times a triangle); false: there are none. */
RT_HD bool rt_sweep_ball(rt_vec3 o, rt_vec3 d, float dd, rt_vec3 c, float rho2, float* t0, float* t1) {
    float s = rt_dot(rt_sub(c, o), d) / dd;
    rt_vec3 w = rt_sub(c, rt_sweep_centre(o, d, s));
    float h2 = rho2 - rt_dot(w, w);
    float half = rt_sqrt(rt_max(h2, 0.f) / dd);
    *t0 = s - half; *t1 = s + half;
    return h2 >= 0.f;
}
/* an interval as a candidate: none when there is none, or it ends before 0 (or is NaN); an entry below 0 counts as 0 */
RT_HD float rt_sweep_clip(bool has, float t0, float t1) {
    return (has && t1 >= 0.f) ? (t0 > 0.f ? t0 : 0.f) : rt_sweep_inf();
}
RT_HD float rt_sweep_ball_time(rt_vec3 o, rt_vec3 d, float dd, rt_vec3 c, float rho2) {
    float t0, t1;
    bool has = rt_sweep_ball(o, d, dd, c, rho2, &t0, &t1);
    return rt_sweep_clip(has, t0, t1);
}
/* The candidate of the edge a + x e, x in [0, 1]: the entry of the line into the cylinder of radius sqrt(rho2) about the axis,
 * solved about the point of the line nearest the axis, valid when the centre at that time projects into the edge. +inf: no such
 * time, an edge of no length (every comparison with the NaN it makes is false), or an edge the ray runs along
 * (RT_SWEEP_PARALLEL). */
RT_HD float rt_sweep_edge_time(rt_vec3 o, rt_vec3 d, float dd, rt_vec3 a, rt_vec3 e, float rho2) {
    float ee = rt_dot(e, e);
    rt_vec3 dp = rt_sub(d, rt_scale(e, rt_dot(d, e) / ee));       /* d less its part along the axis */
    float A = rt_dot(dp, dp);
    rt_vec3 m = rt_sub(o, a);
    rt_vec3 mp = rt_sub(m, rt_scale(e, rt_dot(m, e) / ee));
    float s = -rt_dot(mp, dp) / A;
    rt_vec3 wp = rt_sub(rt_sweep_centre(o, d, s), a);
    rt_vec3 w = rt_sub(wp, rt_scale(e, rt_dot(wp, e) / ee));
    float h2 = rho2 - rt_dot(w, w);
    float half = rt_sqrt(rt_max(h2, 0.f) / A);
    float t = rt_sweep_clip(ee > 0.f && A > RT_SWEEP_PARALLEL * dd && h2 >= 0.f, s - half, s + half);
    float x = rt_dot(rt_sub(rt_sweep_centre(o, d, t), a), e) / ee;
    return (x >= 0.f && x <= 1.f) ? t : rt_sweep_inf();
}

/* the acceptance of one candidate time of a triangle */
RT_HD bool rt_sweep_try(rt_vec3 o, rt_vec3 d, float R, rt_vec3 a, rt_vec3 b, rt_vec3 c, float cmax, float t, float* d2, float* u, float* v) {
    rt_vec3 q = rt_sweep_centre(o, d, t);
    *d2 = rt_point_triangle(q, a, b, c, u, v);
    return rt_sweep_accepts(*d2, R, rt_sweep_sigma(q, d, t, cmax));
}

/* The time of a triangle, world corners a b c. true: *t, and *d2, *u, *v as rt_point_triangle gives them at the centre fl(o + t d). */
RT_HD bool rt_sweep_triangle(rt_vec3 o, rt_vec3 d, float dd, float R, rt_vec3 a, rt_vec3 b, rt_vec3 c, float* t, float* d2, float* u, float* v) {
    const float inf = rt_sweep_inf();
    float cmax = rt_max(rt_max(rt_max3abs(a), rt_max3abs(b)), rt_max3abs(c));
    float R2 = R * R;
    rt_vec3 ab = rt_sub(b, a), ac = rt_sub(c, a);
    rt_vec3 n = rt_cross(ab, ac);
    float nn = rt_dot(n, n);
    if (nn > 0.f) {
        float ln = rt_sqrt(nn);
        float h = rt_dot(rt_sub(o, a), n) / ln;             /* the signed distance of the plane at t = 0 */
        float approach = (h > 0.f ? -rt_dot(d, n) : rt_dot(d, n)) / ln;
        bool outside = rt_abs(h) > R;
        if (outside && !(approach > 0.f)) return false;
        float tf = outside ? (rt_abs(h) - R) / approach : 0.f;
        if (rt_sweep_try(o, d, R, a, b, c, cmax, tf, d2, u, v)) { *t = tf; return true; }
    }
    /* the vertex balls and the edge cylinders */
    float ta = rt_sweep_ball_time(o, d, dd, a, R2), tb = rt_sweep_ball_time(o, d, dd, b, R2), tc = rt_sweep_ball_time(o, d, dd, c, R2);
    float tab = rt_sweep_edge_time(o, d, dd, a, ab, R2), tac = rt_sweep_edge_time(o, d, dd, a, ac, R2);
    float tbc = rt_sweep_edge_time(o, d, dd, b, rt_sub(c, b), R2);
    float below = -1.f;
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int k = 0; k < 6; k++) {
        /* ascending: the least above the one tried last */
        float m = inf;
        m = (ta > below && ta < m) ? ta : m;
        m = (tb > below && tb < m) ? tb : m;
        m = (tc > below && tc < m) ? tc : m;
        m = (tab > below && tab < m) ? tab : m;
        m = (tac > below && tac < m) ? tac : m;
        m = (tbc > below && tbc < m) ? tbc : m;
        if (!(m < inf)) return false;
        if (rt_sweep_try(o, d, R, a, b, c, cmax, m, d2, u, v)) { *t = m; return true; }
        below = m;
    }
    return false;
}

/* The time of a sphere that is a surface. true: *t, and *d2 as rt_point_sphere gives it at the centre fl(o + t d). */
RT_HD bool rt_sweep_sphere(rt_vec3 o, rt_vec3 d, float dd, float R, rt_vec3 c, float r, float* t, float* d2) {
    float outer = r + R, t0, t1;
    if (!rt_sweep_ball(o, d, dd, c, outer * outer, &t0, &t1)) return false;
    if (!(t1 >= 0.f)) return false;
    float tc = t0;
    if (!(t0 > 0.f)) {
        tc = 0.f;                                           /* within the outer ball at t = 0: in the shell, unless inside the inner one */
        float inner = r - R, i0, i1;
        if (inner > 0.f && rt_sweep_ball(o, d, dd, c, inner * inner, &i0, &i1) && i0 < 0.f && i1 > 0.f) tc = i1;
    }
    rt_vec3 q = rt_sweep_centre(o, d, tc), p;
    float f2 = rt_point_sphere(q, c, r, &p);
    if (!rt_sweep_accepts(f2, R, rt_sweep_sigma(q, d, tc, rt_max3abs(c) + r))) return false;
    *t = tc; *d2 = f2;
    return true;
}

/* does the candidate replace the answer so far? T is the ray's constant limit */
RT_HD bool rt_sweep_replaces(float t, uint32_t prim, uint32_t tri, float T, float bestT, uint32_t bestPrim, uint32_t bestTri) {
    return t < T && rt_hits_before(t, prim, tri, bestT, bestPrim, bestTri);
}

/* ---------------------------------------------------------------- the record */
RT_HD RtSweep rt_sweep_not_found(void) {
    RtSweep r;
    r.t = RT_MISS_DST;
    r.found = 0u; r.isSphere = 0u; r.objectIndex = 0u; r.triIndex = 0u;
    r.uv[0] = 0.f; r.uv[1] = 0.f; r.gap = 0.f;
    r.point[0] = 0.f; r.point[1] = 0.f; r.point[2] = 0.f;
    r.startsInContact = 0u;
    r.normal[0] = 0.f; r.normal[1] = 0.f; r.normal[2] = 0.f;
    r._pad = 0u;
    return r;
}
/* from the contact point p and the centre q at t: gap = rt_sqrt(d2), normal from p towards q, -normalize(d) when they coincide */
RT_HD void rt_sweep_finish(RtSweep* r, rt_vec3 d, float t, rt_vec3 q, rt_vec3 p, float d2) {
    r->t = t; r->found = 1u;
    r->gap = rt_sqrt(d2);
    r->point[0] = p.x; r->point[1] = p.y; r->point[2] = p.z;
    r->startsInContact = t == 0.f ? 1u : 0u;
    rt_vec3 g = rt_sub(q, p);
    rt_vec3 nrm = rt_dot(g, g) > 0.f ? rt_normalize(g) : rt_neg(rt_normalize(d));
    r->normal[0] = nrm.x; r->normal[1] = nrm.y; r->normal[2] = nrm.z;
}
RT_HD RtSweep rt_sweep_sphere_record(rt_vec3 o, rt_vec3 d, float t, rt_vec3 c, float radius, uint32_t index) {
    RtSweep r = rt_sweep_not_found();
    rt_vec3 q = rt_sweep_centre(o, d, t), p;
    float d2 = rt_point_sphere(q, c, radius, &p);
    r.isSphere = 1u; r.objectIndex = index;
    rt_sweep_finish(&r, d, t, q, p, d2);
    return r;
}
/* a, b, c: the WORLD corners */
RT_HD RtSweep rt_sweep_triangle_record(rt_vec3 o, rt_vec3 d, float t, rt_vec3 a, rt_vec3 b, rt_vec3 c, uint32_t object, uint32_t tri) {
    RtSweep r = rt_sweep_not_found();
    rt_vec3 q = rt_sweep_centre(o, d, t);
    float u, v;
    float d2 = rt_point_triangle(q, a, b, c, &u, &v);
    r.objectIndex = object; r.triIndex = tri;
    r.uv[0] = u; r.uv[1] = v;
    rt_sweep_finish(&r, d, t, q, rt_bary_point(a, b, c, u, v), d2);
    return r;
}

/* ---------------------------------------------------------------- pruning (the device descent only; DESIGN.md derives it)
 * The ray against the box [lo, hi] grown by g on every side: *entry and *exit of the slab interval, unclipped. inv is
 * rt_sweep_inv(d): 1 / d per axis held within +-RT_SWEEP_HUGE, so an axis the ray does not move along (or hardly: 1 / d
 * overflows) gives times of the size of HUGE with the signs of the two offsets: the whole line inside the grown slab, none of it
 * outside, and no NaN from 0 x inf. No branch and no flag per axis: the device keeps a ray's inverse in three registers. */
RT_HD rt_vec3 rt_sweep_inv(rt_vec3 d) {
    return rt_v3(rt_min(rt_max(1.f / d.x, -RT_SWEEP_HUGE), RT_SWEEP_HUGE), rt_min(rt_max(1.f / d.y, -RT_SWEEP_HUGE), RT_SWEEP_HUGE),
                 rt_min(rt_max(1.f / d.z, -RT_SWEEP_HUGE), RT_SWEEP_HUGE));
}
RT_HD void rt_sweep_box(rt_vec3 lo, rt_vec3 hi, rt_vec3 o, rt_vec3 inv, float g, float* entry, float* exit) {
    float ax = ((lo.x - o.x) - g) * inv.x, bx = ((hi.x - o.x) + g) * inv.x;
    float ay = ((lo.y - o.y) - g) * inv.y, by = ((hi.y - o.y) + g) * inv.y;
    float az = ((lo.z - o.z) - g) * inv.z, bz = ((hi.z - o.z) + g) * inv.z;
    *entry = rt_max(rt_max(rt_min(ax, bx), rt_min(ay, by)), rt_min(az, bz));
    *exit = rt_min(rt_min(rt_max(ax, bx), rt_max(ay, by)), rt_max(az, bz));
}
/* May the grown box hold an accepted contact below or at the bound? No: it ends before 0, the ray passes it by (by more than the
 * roundings of the two times), or it begins above the bound. A NaN time discards nothing. */
RT_HD bool rt_sweep_box_open(float entry, float exit, float best) {
    if (exit < 0.f) return false;
    if (entry * RT_SWEEP_TDOWN > exit * RT_SWEEP_GROW) return false;   /* (both >= 0 here, or entry < 0 <= exit) */
    if (entry * RT_SWEEP_TDOWN > best) return false;
    return true;
}
/* The pad of one ray and one object, once per object: R + sigma + eta in world units over sMin, and the object-space ray's own
 * rounding. omax = max |o component|, dmax likewise of d; mag, sMin, padQ: the object's pruning record (point_queries.h). A
 * contact's centre lies within R (1 + 2^-10) of the object's world coordinates, so cmax bounds its coordinates, and cmax + omax
 * its step t d. over = sMin for the object's tree, 1 for its world box. */
RT_HD float rt_sweep_pad(float R, float omax, float mag, float sMin, float padQ, float over) {
    float cmax = (mag + R) * 1.0009765625f;
    float sigma = RT_SWEEP_SIGMA * (cmax + omax);
    float eta = rt_nearest_eta(cmax, mag, sMin, padQ);
    float g = ((R + sigma) + eta) / over + padQ * ((rt_max(omax, 1.f) + cmax) + omax);
    return g * RT_SWEEP_GROW;
}

#endif /* RT_SWEEP_H */
