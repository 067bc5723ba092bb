/*
 * rt_tri_cut.h — the rule of the cut queries (rt_query_cuts, rt_cuts_exhaustive_host): the segment along which a caller's
 * triangle crosses a triangle of the scene. One text for both sides, under rt_det_math.h's discipline (RT_HD, -ffp-contract=off,
 * rt_* math only), the way rt_tri_overlap.h is shared: the device kernel (k_tris_cut) and the exhaustive host loop compile these
 * very functions, so a pair's cut is the same bits on both.
 *
 * Declared semantics ("Triangle cuts"). The surfaces are the scene's triangles as rt_query_triangles places them;
 * spheres are never members. A query is valid as there. For a valid, prepared query t (rt_tri_prepare) and a scene triangle of
 * world corners a, b, c (rt_tri_cut_prepared):
 *  1. Gate. The pair must pass rt_tri_triangle_prepared(&t, a, b, c). So every cut member is a member of rt_query_triangles
 *     under the same key, and whatever the descent of that query may discard, this one may.
 *  2. Set-up, relative to t.m as stage 2 there: A, B, C = fl(a - m) .., nT = (B - A) x (C - B). The signed heights of the scene
 *     corners over the query's plane, sX = rt_dot(t.n, X) - rt_dot(t.n, t.P), and of the query's corners over the scene
 *     triangle's plane, hX = rt_dot(nT, X) - rt_dot(nT, A). A height is a function of its corner and the other triangle alone:
 *     not of the triangle the corner is looked at in, nor of that triangle's winding.
 *  3. Candidates of a triangle on the other's plane (rt_cut_candidate), at most one per edge index j = 0, 1, 2 (the edge from
 *     corner j to corner j + 1): if the heights of the edge's two ends are strictly of opposite sign, the point
 *     lo + (hi - lo) (s_lo / (s_lo - s_hi)), each component lo + (hi - lo) f in that order of operations, where lo, hi are the
 *     edge's ends ordered by their relative coordinates (x, then y, then z: rt_cut_before), never by winding, and s_lo, s_hi
 *     their heights, computed from lo and hi by the formula of 2; else, if the height of corner j is exactly 0 (either zero),
 *     the corner itself. (An edge whose start lies on the plane cannot cross it strictly,
 *     so the two do not compete for an index.) The point of a scene edge, and a scene corner, are then the same bits in every
 *     triangle that has them. A NaN height makes no candidate. If the three heights of either triangle are all 0 the pair is
 *     coplanar and has no cut; a query with two or three equal corners has nQ = 0, every sX = 0, and never a cut.
 *  4. The common line D = rt_cross(t.n, nT). A triangle's span is the least and the greatest rt_dot(D, candidate) over its
 *     candidates taken in edge order, each with the candidate that gave it: the first candidate gives both, a later one replaces
 *     the lower end only where strictly less and the upper only where strictly greater (the lower edge index wins a tie, and a
 *     NaN projection replaces nothing). No cut if either triangle has no candidate or the spans are strictly apart
 *     (rt_tri_apart: NaN separates nothing). End a is the candidate of the larger of the two lower ends, the scene triangle's
 *     only where strictly larger; end b the candidate of the smaller of the two upper ends, the scene triangle's only where
 *     strictly smaller: on equal projections the query's candidate wins.
 *  5. Output. World coordinates fl(X + t.m) per component. featA / featB: 0..2 the query's edge eQi the point lies on (for a
 *     corner, the edge that starts at it), 3..5 the scene triangle's edge eTj. A cut with a non-finite output number is no
 *     member. A cut of length zero (a == b: the triangles touch in a point) is a member: triangles are closed.
 * Key and list entries are rt_box_overlap.h's (rt_box_insert, RT_BOX_WORDS, rt_box_triangle_word); the record is RtCut.
 */
#ifndef RT_TRI_CUT_H
#define RT_TRI_CUT_H

#include "rt_tri_overlap.h"

/* a cut before it becomes a record: the two ends in world coordinates and the edges they lie on */
typedef struct RtCutSeg {
    rt_vec3 a, b;
    uint32_t featA, featB;
} RtCutSeg;

/* the span of a triangle's candidates on the common line, with the candidates at its two ends */
typedef struct RtCutSpan {
    rt_vec3 lo, hi;
    float dLo, dHi;
    uint32_t fLo, fHi, n;
} RtCutSpan;

/* the canonical order of an edge's ends: by x, then y, then z */
RT_HD bool rt_cut_before(rt_vec3 u, rt_vec3 v) {
    return u.x < v.x || (u.x == v.x && (u.y < v.y || (u.y == v.y && u.z < v.z)));
}

/* c ? a : b, a component at a time (a select of whole structs is a select of addresses, and keeps them in memory) */
RT_HD rt_vec3 rt_cut_pick(bool c, rt_vec3 a, rt_vec3 b) { return rt_v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }

/* the height of the relative corner X over the plane of normal n through the corner whose projection is off */
RT_HD float rt_cut_height(rt_vec3 n, float off, rt_vec3 X) { return rt_dot(n, X) - off; }

/* the candidate of edge index j: the edge from U to V, over the plane (n, off). The heights are taken of the ordered ends
 * themselves (a height is a function of its corner: the same bits whichever way round), so that no predicate of the query's
 * own edges has to outlive the pair. Straight-line code: where the edge does not cross, the quotient is computed and dropped
 * (the device pays less for a select than for a branch) */
RT_HD bool rt_cut_candidate(rt_vec3 n, float off, rt_vec3 U, rt_vec3 V, rt_vec3* x) {
    const bool uFirst = rt_cut_before(U, V);
    const rt_vec3 lo = rt_cut_pick(uFirst, U, V), hi = rt_cut_pick(uFirst, V, U);
    const float sl = rt_cut_height(n, off, lo), sh = rt_cut_height(n, off, hi), su = rt_cut_height(n, off, U);
    const bool crosses = (sl < 0.f && sh > 0.f) || (sl > 0.f && sh < 0.f);
    const float f = sl / (crosses ? sl - sh : 1.f);
    *x = rt_cut_pick(crosses, rt_v3(lo.x + (hi.x - lo.x) * f, lo.y + (hi.y - lo.y) * f, lo.z + (hi.z - lo.z) * f), U);
    return crosses || su == 0.f;
}

/* one more candidate x (is: there is one) into the span */
RT_HD void rt_cut_span_add(RtCutSpan* s, rt_vec3 D, bool is, rt_vec3 x, uint32_t feat) {
    const float d = rt_dot(D, x);
    const bool lower = is && (s->n == 0u || d < s->dLo), upper = is && (s->n == 0u || d > s->dHi);
    s->lo = rt_cut_pick(lower, x, s->lo); s->dLo = lower ? d : s->dLo; s->fLo = lower ? feat : s->fLo;
    s->hi = rt_cut_pick(upper, x, s->hi); s->dHi = upper ? d : s->dHi; s->fHi = upper ? feat : s->fHi;
    s->n += is ? 1u : 0u;
}

/* the span of the triangle U, V, W over the plane (n, off); feat0: the feature code of its edge 0 */
RT_HD RtCutSpan rt_cut_span(rt_vec3 D, rt_vec3 n, float off, rt_vec3 U, rt_vec3 V, rt_vec3 W, uint32_t feat0) {
    RtCutSpan s;
    s.lo = s.hi = rt_v3(0.f, 0.f, 0.f); s.dLo = s.dHi = 0.f; s.fLo = s.fHi = 0u; s.n = 0u;
    rt_vec3 x;
    const bool is0 = rt_cut_candidate(n, off, U, V, &x);
    rt_cut_span_add(&s, D, is0, x, feat0);
    const bool is1 = rt_cut_candidate(n, off, V, W, &x);
    rt_cut_span_add(&s, D, is1, x, feat0 + 1u);
    const bool is2 = rt_cut_candidate(n, off, W, U, &x);
    rt_cut_span_add(&s, D, is2, x, feat0 + 2u);
    return s;
}

/* Steps 2 to 5 for a pair that passed the gate. a, b, c: the WORLD corners. true: the pair has a cut, *seg */
RT_HD bool rt_tri_cut_segment(const RtTriQuery* t, rt_vec3 a, rt_vec3 b, rt_vec3 c, RtCutSeg* seg) {
    const rt_vec3 A = rt_sub(a, t->m), B = rt_sub(b, t->m), C = rt_sub(c, t->m);
    const rt_vec3 nT = rt_cross(rt_sub(B, A), rt_sub(C, B));
    const float nP = rt_dot(t->n, t->P), tA = rt_dot(nT, A);
    const float sA = rt_cut_height(t->n, nP, A), sB = rt_cut_height(t->n, nP, B), sC = rt_cut_height(t->n, nP, C);
    const float hP = rt_cut_height(nT, tA, t->P), hQ = rt_cut_height(nT, tA, t->Q), hR = rt_cut_height(nT, tA, t->R);
    const bool coplanar = (sA == 0.f && sB == 0.f && sC == 0.f) || (hP == 0.f && hQ == 0.f && hR == 0.f);
    const rt_vec3 D = rt_cross(t->n, nT);
    const RtCutSpan q = rt_cut_span(D, nT, tA, t->P, t->Q, t->R, 0u);
    const RtCutSpan s = rt_cut_span(D, t->n, nP, A, B, C, 3u);
    const bool apart = q.n == 0u || s.n == 0u || rt_tri_apart(q.dLo, q.dHi, s.dLo, s.dHi);
    const bool aScene = s.dLo > q.dLo, bScene = s.dHi < q.dHi;
    seg->a = rt_add(rt_cut_pick(aScene, s.lo, q.lo), t->m); seg->featA = aScene ? s.fLo : q.fLo;
    seg->b = rt_add(rt_cut_pick(bScene, s.hi, q.hi), t->m); seg->featB = bScene ? s.fHi : q.fHi;
    return !coplanar && !apart && rt_box_finite(seg->a.x) && rt_box_finite(seg->a.y) && rt_box_finite(seg->a.z) &&
           rt_box_finite(seg->b.x) && rt_box_finite(seg->b.y) && rt_box_finite(seg->b.z);
}
/* a, b, c: the WORLD corners. true: the closed query triangle (valid, prepared) and the closed triangle have a cut, *seg */
RT_HD bool rt_tri_cut_prepared(const RtTriQuery* t, rt_vec3 a, rt_vec3 b, rt_vec3 c, RtCutSeg* seg) {
    if (!rt_tri_triangle_prepared(t, a, b, c)) return false;
    return rt_tri_cut_segment(t, a, b, c, seg);
}
RT_HD bool rt_tri_cut(rt_vec3 p, rt_vec3 q, rt_vec3 r, rt_vec3 a, rt_vec3 b, rt_vec3 c, RtCutSeg* seg) {
    RtTriQuery t = rt_tri_prepare(p, q, r);
    return rt_tri_cut_prepared(&t, a, b, c, seg);
}

/* the record of a slot without a member (all 0), and of a member */
RT_HD RtCut rt_cut_no_member(void) {
    RtCut r;
    r.a[0] = r.a[1] = r.a[2] = 0.f; r.featA = 0u;
    r.b[0] = r.b[1] = r.b[2] = 0.f; r.featB = 0u;
    r.found = 0u; r.objectIndex = 0u; r.triIndex = 0u; r.reserved = 0u;
    return r;
}
RT_HD RtCut rt_cut_record(const RtCutSeg* seg, uint32_t object, uint32_t tri) {
    RtCut r;
    r.a[0] = seg->a.x; r.a[1] = seg->a.y; r.a[2] = seg->a.z; r.featA = seg->featA;
    r.b[0] = seg->b.x; r.b[1] = seg->b.y; r.b[2] = seg->b.z; r.featB = seg->featB;
    r.found = 1u; r.objectIndex = object; r.triIndex = tri; r.reserved = 0u;
    return r;
}

#endif /* RT_TRI_CUT_H */
