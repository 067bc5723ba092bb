/*
 * rt_tri_overlap.h — the rule of the triangle queries (rt_query_triangles, rt_tris_exhaustive_host): which surfaces a caller's
 * triangle touches, in which order they are reported, and what the device descent may discard. One text for both sides, under
 * rt_det_math.h's discipline (RT_HD, -ffp-contract=off, rt_* math only), the way rt_box_overlap.h is shared: the device kernel
 * (k_tris_overlap) and the exhaustive host loop compile these very functions, so a pair's verdict is the same on both.
 *
 * Declared semantics ("Triangle queries"). The surfaces are rt_query_nearest's: every sphere with rt_sphere_is_surface,
 * as a shell, and every triangle of every object, its world corners rt_xform_point(fwd, v) in fp32 (an identity object's corners
 * as they are). No frontOnly, no materials, no alpha maps. A query triangle is three corners p, q, r; it is valid when its nine
 * numbers are finite (equal corners are valid); any other is not searched and has no member. Triangles are closed: touching counts,
 * every "separated" decision is a strict inequality, an axis that comes out zero separates nothing, and a comparison with a NaN
 * operand is false (rt_min / rt_max are minNum / maxNum: a NaN projection leaves the interval to the other corners, and an
 * interval of NaN alone separates nothing).
 *  - Triangle (rt_tri_triangle): a separating-axis test over 17 axes in a fixed order. (1) The box of p, q, r against the box
 *    of a, b, c, both by rt_min / rt_max, by comparisons alone: rt_box_triangle_stage1 with lo, hi the query's box. Exact.
 *    (2) m = fl(lo 0.5 + hi 0.5) of the query's box; all six corners relative to m: P, Q, R, A, B, C; the edges eQ0 = Q - P,
 *    eQ1 = R - Q, eQ2 = P - R and eT0 = B - A, eT1 = C - B, eT2 = A - C of the relative corners. For each axis all six relative
 *    corners are projected by rt_dot and the pair is out when max of one side < min of the other. The axes: nQ = eQ0 x eQ1;
 *    nT = eT0 x eT1; the nine eQi x eTj, i outer; nQ x eQi; nT x eTj. The last six decide coplanar pairs, where the first
 *    eleven all point along the common normal.
 *    A query with two equal corners has one edge exactly zero and nQ exactly zero: nQ, nQ x eQi and three of the nine separate
 *    nothing, and the eleven left are the complete test of its segment against a triangle unless the segment lies in the
 *    triangle's plane, where the axis it would need (nT x the segment) is not in the list: there the rule is this formula and no
 *    more, and may keep a pair that nT x eTj does not separate. With three equal corners only nT and nT x eTj are left beside
 *    stage 1, which is the complete test of a point against a triangle.
 *  - Sphere (rt_tri_sphere): the surface is the shell. Member iff d2min <= fl(rad rad) <= d2max, d2min = rt_point_triangle's
 *    answer at the centre, d2max the largest of the three corner distances rt_dist2 (summed in x, y, z order): the farthest point
 *    of a triangle from any point is a corner. A triangle wholly inside the ball touches nothing.
 * Key, list entries and records are rt_box_overlap.h's (rt_box_insert, rt_box_record, RT_BOX_WORDS).
 */
#ifndef RT_TRI_OVERLAP_H
#define RT_TRI_OVERLAP_H

#include "rt_box_overlap.h"

/* What stage 2 needs of the query, computed once per query: a function of p, q, r alone */
typedef struct RtTriQuery {
    rt_vec3 lo, hi, m;     /* the query's box and its centre fl(lo 0.5 + hi 0.5) */
    rt_vec3 P, Q, R;       /* the corners relative to m */
    rt_vec3 e0, e1, e2;    /* Q - P, R - Q, P - R */
    rt_vec3 n;             /* e0 x e1 */
    rt_vec3 g0, g1, g2;    /* n x e_i */
    float nLo, nHi;        /* the interval of P, Q, R on n */
    float gLo[3], gHi[3];  /* ... and on g_i */
} RtTriQuery;

RT_HD bool rt_tri_valid(rt_vec3 p, rt_vec3 q, rt_vec3 r) {
    return rt_box_finite(p.x) && rt_box_finite(p.y) && rt_box_finite(p.z) && rt_box_finite(q.x) && rt_box_finite(q.y) &&
           rt_box_finite(q.z) && rt_box_finite(r.x) && rt_box_finite(r.y) && rt_box_finite(r.z);
}

/* the interval of three corners on an axis */
RT_HD void rt_tri_interval(rt_vec3 ax, rt_vec3 a, rt_vec3 b, rt_vec3 c, float* lo, float* hi) {
    float x = rt_dot(ax, a), y = rt_dot(ax, b), z = rt_dot(ax, c);
    *lo = rt_min(rt_min(x, y), z);
    *hi = rt_max(rt_max(x, y), z);
}
/* two intervals strictly apart (NaN: false) */
RT_HD bool rt_tri_apart(float qLo, float qHi, float tLo, float tHi) { return qHi < tLo || qLo > tHi; }
/* one axis with the query's interval known */
RT_HD bool rt_tri_known_out(float qLo, float qHi, rt_vec3 ax, rt_vec3 A, rt_vec3 B, rt_vec3 C) {
    float tLo, tHi;
    rt_tri_interval(ax, A, B, C, &tLo, &tHi);
    return rt_tri_apart(qLo, qHi, tLo, tHi);
}
/* one axis, all six corners projected */
RT_HD bool rt_tri_axis_out(rt_vec3 ax, rt_vec3 P, rt_vec3 Q, rt_vec3 R, rt_vec3 A, rt_vec3 B, rt_vec3 C) {
    float qLo, qHi;
    rt_tri_interval(ax, P, Q, R, &qLo, &qHi);
    return rt_tri_known_out(qLo, qHi, ax, A, B, C);
}

RT_HD RtTriQuery rt_tri_prepare(rt_vec3 p, rt_vec3 q, rt_vec3 r) {
    RtTriQuery t;
    t.lo = rt_v3(rt_min(rt_min(p.x, q.x), r.x), rt_min(rt_min(p.y, q.y), r.y), rt_min(rt_min(p.z, q.z), r.z));
    t.hi = rt_v3(rt_max(rt_max(p.x, q.x), r.x), rt_max(rt_max(p.y, q.y), r.y), rt_max(rt_max(p.z, q.z), r.z));
    t.m = rt_v3(t.lo.x * 0.5f + t.hi.x * 0.5f, t.lo.y * 0.5f + t.hi.y * 0.5f, t.lo.z * 0.5f + t.hi.z * 0.5f);
    t.P = rt_sub(p, t.m); t.Q = rt_sub(q, t.m); t.R = rt_sub(r, t.m);
    t.e0 = rt_sub(t.Q, t.P); t.e1 = rt_sub(t.R, t.Q); t.e2 = rt_sub(t.P, t.R);
    t.n = rt_cross(t.e0, t.e1);
    t.g0 = rt_cross(t.n, t.e0); t.g1 = rt_cross(t.n, t.e1); t.g2 = rt_cross(t.n, t.e2);
    rt_tri_interval(t.n, t.P, t.Q, t.R, &t.nLo, &t.nHi);
    rt_tri_interval(t.g0, t.P, t.Q, t.R, &t.gLo[0], &t.gHi[0]);
    rt_tri_interval(t.g1, t.P, t.Q, t.R, &t.gLo[1], &t.gHi[1]);
    rt_tri_interval(t.g2, t.P, t.Q, t.R, &t.gLo[2], &t.gHi[2]);
    return t;
}

/* the three axes e x eT_j of one query edge e (all three evaluated: the verdict of a pair is the OR over its axes, whatever
 * the order they are looked at in, and straight-line code costs the device less than three more nested branches) */
RT_HD bool rt_tri_edge_out(const RtTriQuery* t, rt_vec3 e, rt_vec3 f0, rt_vec3 f1, rt_vec3 f2, rt_vec3 A, rt_vec3 B, rt_vec3 C) {
    bool o0 = rt_tri_axis_out(rt_cross(e, f0), t->P, t->Q, t->R, A, B, C);
    bool o1 = rt_tri_axis_out(rt_cross(e, f1), t->P, t->Q, t->R, A, B, C);
    bool o2 = rt_tri_axis_out(rt_cross(e, f2), t->P, t->Q, t->R, A, B, C);
    return o0 | o1 | o2;
}

/* a, b, c: the WORLD corners. true: the closed query triangle (valid, prepared) and the closed triangle touch */
RT_HD bool rt_tri_triangle_prepared(const RtTriQuery* t, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    if (!rt_box_triangle_stage1(t->lo, t->hi, a, b, c)) return false;
    rt_vec3 A = rt_sub(a, t->m), B = rt_sub(b, t->m), C = rt_sub(c, t->m);
    rt_vec3 f0 = rt_sub(B, A), f1 = rt_sub(C, B), f2 = rt_sub(A, C);
    rt_vec3 nT = rt_cross(f0, f1);
    bool out = rt_tri_known_out(t->nLo, t->nHi, t->n, A, B, C);                            /* nQ */
    out |= rt_tri_axis_out(nT, t->P, t->Q, t->R, A, B, C);                                 /* nT */
    if (out) return false;
    out = rt_tri_edge_out(t, t->e0, f0, f1, f2, A, B, C);                                  /* eQi x eTj */
    out |= rt_tri_edge_out(t, t->e1, f0, f1, f2, A, B, C);
    out |= rt_tri_edge_out(t, t->e2, f0, f1, f2, A, B, C);
    if (out) return false;
    out = rt_tri_known_out(t->gLo[0], t->gHi[0], t->g0, A, B, C);                          /* nQ x eQi */
    out |= rt_tri_known_out(t->gLo[1], t->gHi[1], t->g1, A, B, C);
    out |= rt_tri_known_out(t->gLo[2], t->gHi[2], t->g2, A, B, C);
    out |= rt_tri_axis_out(rt_cross(nT, f0), t->P, t->Q, t->R, A, B, C);                   /* nT x eTj */
    out |= rt_tri_axis_out(rt_cross(nT, f1), t->P, t->Q, t->R, A, B, C);
    out |= rt_tri_axis_out(rt_cross(nT, f2), t->P, t->Q, t->R, A, B, C);
    return !out;
}
RT_HD bool rt_tri_triangle(rt_vec3 p, rt_vec3 q, rt_vec3 r, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    RtTriQuery t = rt_tri_prepare(p, q, r);
    return rt_tri_triangle_prepared(&t, a, b, c);
}

/* true: the closed triangle touches the shell of the sphere */
RT_HD bool rt_tri_sphere(rt_vec3 p, rt_vec3 q, rt_vec3 r, rt_vec3 centre, float rad) {
    float u, v;
    float r2 = rad * rad;
    float d2min = rt_point_triangle(centre, p, q, r, &u, &v);
    float d2max = rt_max(rt_max(rt_dist2(centre, p), rt_dist2(centre, q)), rt_dist2(centre, r));
    return d2min <= r2 && r2 <= d2max;
}

/* ---------------------------------------------------------------- pruning (the device descent only; DESIGN.md, "Triangle
 * queries", has both derivations).
 * (a) Box against box. A member triangle passed stage 1, which is rt_box_triangle_stage1 on the query's box, so what "Box queries"
 * derives holds word for word with [lo, hi] the query's box: rt_box_apart is exact for an identity object, rt_box_placed_apart
 * and rt_box_object_apart with rt_box_pad(mag) are sound for a placed one.
 * (b) The query's plane against a box. A member passed the nQ axis: not all of its three fp32 projections t(a) =
 * rt_dot(nQ, fl(a - m)) lie above nHi, and not all below nLo. Let [blo, bhi] hold the fp32 world corners of everything below a
 * node: the node's own box for an identity object, and for a placed one the box (a) takes to world space, M centre +- |M| extent
 * grown by rt_box_pad(mag) (rt_tri_world_box; "Box queries" shows that it holds them). Per axis i let d_i be whichever of
 * fl(blo_i - m_i), fl(bhi_i - m_i) makes nQ_i d_i smaller, and L = (nQ_x d_x + nQ_y d_y) + nQ_z d_z in fp32; U likewise with the
 * larger; G = sum of max(|nQ_i fl(blo_i - m_i)|, |nQ_i fl(bhi_i - m_i)|), which is sum |nQ_i| max|x_i - m_i| over the box up to
 * rounding. In exact arithmetic L* <= nQ . (a - m) for every a in the box. t(a) has one rounding in the subtraction, one in the
 * product and two in the sums: |t(a) - nQ . (a - m)| <= 4 u G*. L has the same four: |L - L*| <= 4 u G*. The computed G is at
 * least G* (1 - 4 u), the pad's own product and the final subtraction round once each against at most G* (1 + ..): 4 + 4 + 2 = 10
 * u G* and terms in u^2. The pad is 32 u G and eight times the smallest normal number beside it for products that underflow (six
 * products, gradual or flushed). The subtree goes when L - pad > nHi or U + pad < nLo, strictly. A box with an infinite or NaN
 * bound (an unbounded object: pad +inf) gives an infinite or NaN L, U or pad, the comparisons are false and nothing is discarded;
 * so does a query whose nQ overflowed. nQ exactly zero gives L = U = 0 = nLo = nHi: nothing is discarded. */
#define RT_TRI_PAD 1.9073486328125e-06f /* 32 u = 2^-19, against the 10 u the derivation counts */
RT_HD bool rt_tri_plane_apart(const RtTriQuery* t, rt_vec3 blo, rt_vec3 bhi) {
    float xl = t->n.x * (blo.x - t->m.x), xh = t->n.x * (bhi.x - t->m.x);
    float yl = t->n.y * (blo.y - t->m.y), yh = t->n.y * (bhi.y - t->m.y);
    float zl = t->n.z * (blo.z - t->m.z), zh = t->n.z * (bhi.z - t->m.z);
    float L = (rt_min(xl, xh) + rt_min(yl, yh)) + rt_min(zl, zh);
    float U = (rt_max(xl, xh) + rt_max(yl, yh)) + rt_max(zl, zh);
    float G = (rt_max(rt_abs(xl), rt_abs(xh)) + rt_max(rt_abs(yl), rt_abs(yh))) + rt_max(rt_abs(zl), rt_abs(zh));
    float pad = RT_TRI_PAD * G + 9.4039548e-38f;
    return L - pad > t->nHi || U + pad < t->nLo;
}
/* the world box (a) tests for a node of a placed object, in rt_box_placed_axis_out's very expressions */
RT_HD void rt_tri_world_box(rt_vec3 r0, rt_vec3 r1, rt_vec3 r2, rt_vec3 tr, rt_vec3 blo, rt_vec3 bhi, float pad, rt_vec3* wlo, rt_vec3* whi) {
    rt_vec3 c = rt_v3(blo.x * 0.5f + bhi.x * 0.5f, blo.y * 0.5f + bhi.y * 0.5f, blo.z * 0.5f + bhi.z * 0.5f);
    rt_vec3 e = rt_v3(bhi.x * 0.5f - blo.x * 0.5f, bhi.y * 0.5f - blo.y * 0.5f, bhi.z * 0.5f - blo.z * 0.5f);
    float Cx = ((r0.x * c.x + r0.y * c.y) + r0.z * c.z) + tr.x, Ex = (rt_abs(r0.x) * e.x + rt_abs(r0.y) * e.y) + rt_abs(r0.z) * e.z;
    float Cy = ((r1.x * c.x + r1.y * c.y) + r1.z * c.z) + tr.y, Ey = (rt_abs(r1.x) * e.x + rt_abs(r1.y) * e.y) + rt_abs(r1.z) * e.z;
    float Cz = ((r2.x * c.x + r2.y * c.y) + r2.z * c.z) + tr.z, Ez = (rt_abs(r2.x) * e.x + rt_abs(r2.y) * e.y) + rt_abs(r2.z) * e.z;
    *wlo = rt_v3((Cx - Ex) - pad, (Cy - Ey) - pad, (Cz - Ez) - pad);
    *whi = rt_v3((Cx + Ex) + pad, (Cy + Ey) + pad, (Cz + Ez) + pad);
}

#endif /* RT_TRI_OVERLAP_H */
