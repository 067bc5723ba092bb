/*
 * rt_point_side.h — the rule of the signed point queries (rt_query_nearest_signed, rt_nearest_side_host): on which side of the
 * surface a point lies, given the record rt_query_nearest reported for it. One text for both sides under rt_det_math.h's
 * discipline (RT_HD, -ffp-contract=off, rt_* math only): the device kernel (k_nearest_side) and the host loop compile these very
 * functions, read the topology table and the world corners through an accessor they pass in, and so sum the same terms in the
 * same order and give the same byte.
 *
 * Declared semantics ("Signed point queries"). side is +1 outside, -1 inside, 0 unknown or nothing found.
 *  - A sphere: l = |q - c| as rt_point_sphere computes it; +1 when l > r, -1 when l < r, 0 when l == r.
 *  - A triangle: the sign is relative to the closed component the reported triangle belongs to, by the angle-weighted
 *    pseudo-normal N of the feature the closest point lies on (Baerentzen and Aanaes): the face's normal; the sum of the two unit
 *    face normals at an edge; the sum of corner angle x unit face normal over the fan of triangles around a vertex. All of it from
 *    the WORLD corners rt_xform_point(fwd, v), as the nearest kernel places them. side = sign(dot(q - p, N)) x the object's
 *    orientation, p = rt_bary_point(a, b, c, u, v) of the record's barycentrics.
 *  - 0 when: the triangle's component is not signable; the triangle has no area in world space; the feature is a vertex whose fan
 *    is not one closed cycle of at most RT_SIDE_MAX_FAN triangles; the object's orientation is 0; N is not finite; the dot
 *    product is 0 or NaN.
 *
 * The topology table (one row per triangle, numbered as RtNearest.triIndex numbers them; built by mesh_topology.h):
 *    n[k], k = 0..2   the neighbour across edge k (edge k joins corner k and corner k + 1): neighbourTriangle << 2 | neighbourEdge,
 *                     or RT_TOPO_NONE where the edge is not shared by exactly two non-degenerate triangles
 *    flags            RT_TOPO_FLIP: the stored winding disagrees with the component's outward orientation (the normal is negated);
 *                     RT_TOPO_SIGNABLE: the component is closed, orientable and has a volume;
 *                     RT_TOPO_FAN << k: corner k's fan is one closed cycle of at most RT_SIDE_MAX_FAN triangles
 */
#ifndef RT_POINT_SIDE_H
#define RT_POINT_SIDE_H

#include "rt_point_query.h"

#define RT_SIDE_MAX_FAN 256
#define RT_TOPO_NONE 0xffffffffu
#define RT_TOPO_FLIP 1u
#define RT_TOPO_SIGNABLE 2u
#define RT_TOPO_FAN 4u /* << corner */

/* region codes of rt_point_triangle_feature */
#define RT_FEAT_FACE 0
#define RT_FEAT_A 1
#define RT_FEAT_B 2
#define RT_FEAT_C 3
#define RT_FEAT_AB 4
#define RT_FEAT_AC 5
#define RT_FEAT_BC 6

typedef struct rt_topo_row { uint32_t n[3]; uint32_t flags; } rt_topo_row;

/* the winning edge of rt_point_edges, by its very comparisons */
RT_HD int rt_point_edges_feature(rt_vec3 q, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    float t = rt_point_segment_t(q, a, b);
    int code = RT_FEAT_AB;
    float best = rt_dist2(q, rt_bary_point(a, b, c, t, 0.f));
    t = rt_point_segment_t(q, a, c);
    float d = rt_dist2(q, rt_bary_point(a, b, c, 0.f, t));
    if (d < best) { best = d; code = RT_FEAT_AC; }
    t = rt_point_segment_t(q, b, c);
    d = rt_dist2(q, rt_bary_point(a, b, c, 1.f - t, t));
    if (d < best) { best = d; code = RT_FEAT_BC; }
    return code;
}

/* Which feature of triangle abc the closest point to q lies on: the branch rt_point_triangle takes for the same arguments
 * (rt_point_query.h), statement for statement, and where that falls back to rt_point_edges, the edge that wins there. */
RT_HD int rt_point_triangle_feature(rt_vec3 q, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    rt_vec3 ab = rt_sub(b, a), ac = rt_sub(c, a);
    rt_vec3 n = rt_cross(ab, ac);
    if (!(rt_dot(n, n) > 0.f)) return rt_point_edges_feature(q, a, b, c);
    rt_vec3 ap = rt_sub(q, a);
    float d1 = rt_dot(ab, ap), d2 = rt_dot(ac, ap);
    rt_vec3 bp = rt_sub(q, b);
    float d3 = rt_dot(ab, bp), d4 = rt_dot(ac, bp);
    rt_vec3 cp = rt_sub(q, c);
    float d5 = rt_dot(ab, cp), d6 = rt_dot(ac, cp);
    float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.f && d2 <= 0.f) return RT_FEAT_A;
    if (d3 >= 0.f && d4 <= d3) return RT_FEAT_B;
    if (d6 >= 0.f && d5 <= d6) return RT_FEAT_C;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        float den = d1 - d3;
        if (!(den > 0.f)) return rt_point_edges_feature(q, a, b, c);
        return RT_FEAT_AB;
    }
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        float den = d2 - d6;
        if (!(den > 0.f)) return rt_point_edges_feature(q, a, b, c);
        return RT_FEAT_AC;
    }
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        float den = (d4 - d3) + (d5 - d6);
        if (!(den > 0.f)) return rt_point_edges_feature(q, a, b, c);
        return RT_FEAT_BC;
    }
    float sum = (va + vb) + vc;
    if (!(sum > 0.f) || !(va >= 0.f) || !(vb >= 0.f) || !(vc >= 0.f)) return rt_point_edges_feature(q, a, b, c);
    return RT_FEAT_FACE;
}

/* atan2(y, x) for y >= 0, in [0, pi]: the ratio of the smaller to the larger magnitude, one reduction at tan(pi / 8), an odd
 * polynomial of degree 9 on [-tan(pi / 8), tan(pi / 8)] (the coefficients of Cephes' atanf), and the octant put back. No libm:
 * the host's and the device's differ. y == 0 and x == 0 give 0. */
RT_HD float rt_atan2_pos(float y, float x) {
    float ax = rt_abs(x);
    float hi = rt_max(ax, y), lo = rt_min(ax, y);
    if (!(hi > 0.f)) return 0.f;
    float t = lo / hi; /* [0, 1] */
    float base = 0.f;
    if (t > 0.4142135679721832275390625f) {
        t = (t - 1.f) / (t + 1.f);
        base = 0.785398185253143310546875f;
    }
    float z = t * t;
    float p = 8.05374449538e-2f * z - 1.38776856032e-1f;
    p = p * z + 1.99777106478e-1f;
    p = p * z - 3.33329491539e-1f;
    float r = base + (p * z * t + t);
    if (y > ax) r = 1.57079637050628662109375f - r;
    if (x < 0.f) r = 3.1415927410125732421875f - r;
    return r;
}
/* the angle between e1 and e2: atan2(|e1 x e2|, e1 . e2) */
RT_HD float rt_angle(rt_vec3 e1, rt_vec3 e2) {
    rt_vec3 x = rt_cross(e1, e2);
    return rt_atan2_pos(rt_sqrt(rt_dot(x, x)), rt_dot(e1, e2));
}

RT_HD int rt_point_side_sphere(rt_vec3 q, rt_vec3 centre, float r) {
    rt_vec3 d = rt_sub(q, centre);
    float l = rt_sqrt(rt_dot(d, d));
    return l > r ? 1 : (l < r ? -1 : 0);
}

RT_HD bool rt_v3_finite(rt_vec3 v) {
    return !(rt_isnan(v.x) || rt_isinf(v.x) || rt_isnan(v.y) || rt_isinf(v.y) || rt_isnan(v.z) || rt_isinf(v.z));
}
/* corner k of (a, b, c), k taken mod 3 by the caller: selects, no indexed array */
RT_HD rt_vec3 rt_pick3(rt_vec3 a, rt_vec3 b, rt_vec3 c, uint32_t k) { return k == 0u ? a : (k == 1u ? b : c); }
/* the unit normal of the stored winding, negated where the row says FLIP */
RT_HD rt_vec3 rt_side_unit_normal(rt_vec3 a, rt_vec3 b, rt_vec3 c, uint32_t flags) {
    rt_vec3 n = rt_normalize(rt_cross(rt_sub(b, a), rt_sub(c, a)));
    return (flags & RT_TOPO_FLIP) ? rt_neg(n) : n;
}

#ifdef __cplusplus
/* What both sides pass in:
 *   rt_topo_row row(uint32_t tri) const                                  the table's row of a triangle
 *   void corners(uint32_t tri, rt_vec3* a, rt_vec3* b, rt_vec3* c) const  its world corners under the object of the record
 *
 * The fan of corner k of triangle tri: starting at tri, step across the edge that leaves the corner (edge k); the neighbour's edge
 * number, with the two rows' FLIP bits, tells which of its corners is the shared vertex and which of its edges leaves it; go on
 * until tri comes round again. At most RT_SIDE_MAX_FAN triangles: beyond that, or at a missing neighbour, false (a corrupted table
 * cannot loop for ever). *N: the sum of corner angle x unit normal, in the order walked. *steps: triangles visited. */
template <typename Acc>
RT_HD bool rt_side_fan(const Acc& acc, uint32_t tri, rt_topo_row row, uint32_t k, rt_vec3 a, rt_vec3 b, rt_vec3 c, rt_vec3* N, uint32_t* steps) {
    rt_vec3 sum = rt_v3(0.f, 0.f, 0.f);
    bool leaving = true; /* the edge to cross next starts at the vertex (edge k) or ends at it (edge k - 1) */
    for (uint32_t step = 0; step < (uint32_t)RT_SIDE_MAX_FAN; step++) {
        const rt_vec3 v0 = rt_pick3(a, b, c, k), v1 = rt_pick3(a, b, c, (k + 1u) % 3u), v2 = rt_pick3(a, b, c, (k + 2u) % 3u);
        const float angle = rt_angle(rt_sub(v1, v0), rt_sub(v2, v0));
        sum = rt_add(sum, rt_scale(rt_side_unit_normal(a, b, c, row.flags), angle));
        const uint32_t e = leaving ? k : (k + 2u) % 3u;
        const uint32_t nb = e == 0u ? row.n[0] : (e == 1u ? row.n[1] : row.n[2]);
        if (nb == RT_TOPO_NONE) return false;
        const uint32_t t2 = nb >> 2, e2 = nb & 3u;
        if (t2 == tri) { *N = sum; *steps = step + 1u; return true; }
        const rt_topo_row row2 = acc.row(t2);
        /* consistently wound neighbours run along the shared edge in opposite directions */
        const bool atEnd = leaving != (((row.flags ^ row2.flags) & RT_TOPO_FLIP) != 0u);
        k = atEnd ? (e2 + 1u) % 3u : e2 % 3u;
        leaving = atEnd;
        row = row2;
        acc.corners(t2, &a, &b, &c);
    }
    return false;
}

/* The side of q for a record that reports triangle tri at barycentrics (u, v); orient: the object's orientation (+1, -1, 0).
 * *feature: the region code, or -1 where the rule ended before it; *fan: triangles walked (0 unless a vertex). */
template <typename Acc>
RT_HD int rt_point_side_triangle(const Acc& acc, rt_vec3 q, uint32_t tri, float u, float v, int orient, int* feature, uint32_t* fan) {
    *feature = -1; *fan = 0u;
    if (orient == 0) return 0;
    const rt_topo_row row = acc.row(tri);
    if (!(row.flags & RT_TOPO_SIGNABLE)) return 0;
    rt_vec3 a, b, c;
    acc.corners(tri, &a, &b, &c);
    const rt_vec3 n = rt_cross(rt_sub(b, a), rt_sub(c, a));
    if (!(rt_dot(n, n) > 0.f)) return 0;
    const int feat = rt_point_triangle_feature(q, a, b, c);
    *feature = feat;
    rt_vec3 N;
    if (feat == RT_FEAT_FACE) {
        N = (row.flags & RT_TOPO_FLIP) ? rt_neg(n) : n;
    } else if (feat >= RT_FEAT_AB) {
        const uint32_t nb = feat == RT_FEAT_AB ? row.n[0] : (feat == RT_FEAT_BC ? row.n[1] : row.n[2]);
        if (nb == RT_TOPO_NONE) return 0;
        const rt_topo_row row2 = acc.row(nb >> 2);
        rt_vec3 a2, b2, c2;
        acc.corners(nb >> 2, &a2, &b2, &c2);
        N = rt_add(rt_side_unit_normal(a, b, c, row.flags), rt_side_unit_normal(a2, b2, c2, row2.flags));
    } else {
        const uint32_t k = (uint32_t)(feat - RT_FEAT_A);
        if (!(row.flags & (RT_TOPO_FAN << k))) return 0;
        if (!rt_side_fan(acc, tri, row, k, a, b, c, &N, fan)) return 0;
    }
    if (!rt_v3_finite(N)) return 0;
    const float s = rt_dot(rt_sub(q, rt_bary_point(a, b, c, u, v)), N);
    if (s > 0.f) return orient;
    if (s < 0.f) return -orient;
    return 0;
}
#endif /* __cplusplus */

#endif /* RT_POINT_SIDE_H */
