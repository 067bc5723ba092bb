/*
 * rt_point_query.h — the rule of the point queries (rt_query_nearest, rt_nearest_exhaustive_host): the closest point of a
 * triangle and of a sphere, the running bound, and the pruning test of the device traversal. One text for both sides, under
 * rt_det_math.h's discipline (RT_HD, -ffp-contract=off, rt_* math only), the way rt_ao_rays.h is shared: the device kernel
 * (k_nearest_points) and the exhaustive host loop compile these very functions, so a primitive's squared distance has the same 32
 * bits on both.
 *
 * Declared semantics of a query ("Point queries").
 *  - Scene surfaces: the surface of every sphere with radius > 0 (the sphere table's unused slots are zeroed: centre 0, radius 0;
 *    they are no surface), and every triangle of every object, placed by the object's FORWARD matrix: a triangle's world corners
 *    are rt_xform_point(fwd, v), computed in fp32 from the object's matrix and the object-space corner; an object whose matrix is
 *    exactly the identity (RT_OBJ_FWD_IDENTITY) uses the corner itself (bit-identical: products with 1 and 0 and sums with 0).
 *  - The distance is Euclidean in world space, whatever the object's scale or shear. frontOnly, materials and alpha maps play no
 *    part: this is geometry, not visibility.
 *  - Point i with limit T (maxDist[i]; no limit when the array is NULL) keeps a running bound best2, started at fl(T * T), or +inf
 *    without a limit. A primitive replaces the current answer when its squared distance is STRICTLY less than best2. found = 1 when
 *    one did, and dst = rt_sqrt(best2). A limit that is NaN or <= 0 gives the not-found record without a search.
 *  - dst does not depend on the visiting order: it is the minimum of one function (the fp32 squared distance below) over one set,
 *    provided pruning never discards a subtree that holds the minimiser (rt_nearest_threshold).
 *  - Which primitive is reported does depend on the order where two are equally near (a closest point on a shared edge or vertex
 *    is the common case): the reported primitive is A minimiser in fp32, not a particular one.
 */
#ifndef RT_POINT_QUERY_H
#define RT_POINT_QUERY_H

#include "rt_det_math.h"

/* p = w a + u b + v c, w = (1 - u) - v: a corner comes back exactly at (0,0), (1,0), (0,1) */
RT_HD rt_vec3 rt_bary_point(rt_vec3 a, rt_vec3 b, rt_vec3 c, float u, float v) {
    float w = (1.f - u) - v;
    return rt_add(rt_add(rt_scale(a, w), rt_scale(b, u)), rt_scale(c, v));
}

RT_HD float rt_dist2(rt_vec3 q, rt_vec3 p) {
    rt_vec3 d = rt_sub(q, p);
    return rt_dot(d, d);
}

/* parameter of the point of segment a + t (b - a), t in [0, 1], closest to q; a == b gives 0 */
RT_HD float rt_point_segment_t(rt_vec3 q, rt_vec3 a, rt_vec3 b) {
    rt_vec3 ab = rt_sub(b, a);
    float den = rt_dot(ab, ab);
    if (!(den > 0.f)) return 0.f;
    return rt_clamp01(rt_dot(rt_sub(q, a), ab) / den);
}

/* The nearest of the three edges (ab, ac, bc in this order, strictly nearer replaces): what a triangle of zero area is. A
 * triangle that is one point gives that point. */
RT_HD float rt_point_edges(rt_vec3 q, rt_vec3 a, rt_vec3 b, rt_vec3 c, float* u, float* v) {
    float t = rt_point_segment_t(q, a, b);
    float bu = t, bv = 0.f;
    float best = rt_dist2(q, rt_bary_point(a, b, c, bu, bv));
    t = rt_point_segment_t(q, a, c);
    float d = rt_dist2(q, rt_bary_point(a, b, c, 0.f, t));
    if (d < best) { best = d; bu = 0.f; bv = t; }
    t = rt_point_segment_t(q, b, c);
    d = rt_dist2(q, rt_bary_point(a, b, c, 1.f - t, t));
    if (d < best) { best = d; bu = 1.f - t; bv = t; }
    *u = bu; *v = bv;
    return best;
}

/* Squared distance from q to triangle abc and the barycentrics of the closest point p = w a + u b + v c (u towards corner 1, v
 * towards corner 2). Region classification of Ericson, Real-Time Collision Detection, 5.1.5: the three vertex regions, the three
 * edge regions, the face. Every division is by a quantity that is positive in the region where it is used (an edge's squared
 * length, twice the squared area); where rounding or a zero area makes it not so, the answer is the nearest of the three edges
 * (rt_point_edges), never NaN for finite inputs. The returned value is |q - p|^2 of the p it returns (rt_bary_point of the
 * returned u, v), not a separately derived expression. */
RT_HD float rt_point_triangle(rt_vec3 q, rt_vec3 a, rt_vec3 b, rt_vec3 c, float* u, float* v) {
    rt_vec3 ab = rt_sub(b, a), ac = rt_sub(c, a);
    rt_vec3 n = rt_cross(ab, ac);
    if (!(rt_dot(n, n) > 0.f)) return rt_point_edges(q, a, b, c, u, v);
    float bu, bv;
    rt_vec3 ap = rt_sub(q, a);
    float d1 = rt_dot(ab, ap), d2 = rt_dot(ac, ap);
    rt_vec3 bp = rt_sub(q, b);
    float d3 = rt_dot(ab, bp), d4 = rt_dot(ac, bp);
    rt_vec3 cp = rt_sub(q, c);
    float d5 = rt_dot(ab, cp), d6 = rt_dot(ac, cp);
    float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.f && d2 <= 0.f) { bu = 0.f; bv = 0.f; }                       /* vertex a */
    else if (d3 >= 0.f && d4 <= d3) { bu = 1.f; bv = 0.f; }                   /* vertex b */
    else if (d6 >= 0.f && d5 <= d6) { bu = 0.f; bv = 1.f; }                   /* vertex c */
    else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                           /* edge ab */
        float den = d1 - d3;
        if (!(den > 0.f)) return rt_point_edges(q, a, b, c, u, v);
        bu = d1 / den; bv = 0.f;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {                         /* edge ac */
        float den = d2 - d6;
        if (!(den > 0.f)) return rt_point_edges(q, a, b, c, u, v);
        bu = 0.f; bv = d2 / den;
    } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {           /* edge bc */
        float den = (d4 - d3) + (d5 - d6);
        if (!(den > 0.f)) return rt_point_edges(q, a, b, c, u, v);
        bv = (d4 - d3) / den; bu = 1.f - bv;
    } else {                                                                  /* face */
        float sum = (va + vb) + vc;
        if (!(sum > 0.f) || !(va >= 0.f) || !(vb >= 0.f) || !(vc >= 0.f)) return rt_point_edges(q, a, b, c, u, v);
        bu = vb / sum; bv = vc / sum;
    }
    *u = bu; *v = bv;
    return rt_dist2(q, rt_bary_point(a, b, c, bu, bv));
}

/* (|q - c| - r)^2 and p = c + r (q - c) / |q - c|; q == c exactly: p = c + (r, 0, 0) */
RT_HD float rt_point_sphere(rt_vec3 q, rt_vec3 centre, float r, rt_vec3* p) {
    rt_vec3 d = rt_sub(q, centre);
    float l = rt_sqrt(rt_dot(d, d));
    float e = l - r;
    if (l > 0.f) *p = rt_add(centre, rt_scale(d, r / l));
    else *p = rt_v3(centre.x + r, centre.y, centre.z);
    return e * e;
}
/* a sphere that is a surface: the zeroed slots of the sphere table are not */
RT_HD bool rt_sphere_is_surface(float r) { return r > 0.f; }

/* the bound a search starts with; *search = false: the not-found record without a search (a limit that is NaN or <= 0) */
RT_HD float rt_nearest_start(bool hasLimit, float T, bool* search) {
    *search = true;
    if (!hasLimit) return rt_u2f(0x7f800000u);
    if (!(T > 0.f)) { *search = false; return 0.f; }
    return T * T;
}

/* ---------------------------------------------------------------- pruning (the device traversal only)
 * Squared distance from q to the box [lo, hi]: per axis max(lo - q, 0, q - hi). One subtraction of two floats has a relative
 * error of u = 2^-24 only, so the box side carries no absolute pad; the three squares and two sums add 2.5 u more. */
RT_HD float rt_point_box2(rt_vec3 q, rt_vec3 lo, rt_vec3 hi) {
    float dx = rt_max(rt_max(lo.x - q.x, 0.f), q.x - hi.x);
    float dy = rt_max(rt_max(lo.y - q.y, 0.f), q.y - hi.y);
    float dz = rt_max(rt_max(lo.z - q.z, 0.f), q.z - hi.z);
    return (dx * dx + dy * dy) + dz * dz;
}

/* eta for one point and one object ("Point queries", has the derivation): what the fp32 distance of any of the
 * object's triangles can fall below the distance the boxes speak of. qmax = max |q component|; mag bounds |M| |[v; 1]| over the
 * object's corners and the object's world box; sMin and padQ: the object's pruning record (point_queries.h). */
#define RT_NEAR_ETA 3.814697265625e-06f      /* 64 u = 2^-18, against the 28 u the derivation counts */
#define RT_NEAR_SLACK 1.000003814697265625f   /* 1 + 2^-18: the roundings of the threshold itself and of rt_point_box2 (< 16 u) */
RT_HD float rt_nearest_eta(float qmax, float mag, float sMin, float padQ) {
    return RT_NEAR_ETA * (qmax + mag) + (sMin * padQ) * rt_max(qmax, 1.f);
}
/* A subtree whose box, in the space where world distance >= sMin x box distance, has squared distance d2box from the point is
 * discarded only when sMin sqrt(d2box) > sqrt(best2) + eta. In squared form, recomputed only when best2 changes: discard when
 * d2box > rt_nearest_threshold(...). sMin == 0 (a singular matrix) and eta == +inf (an unbounded object) give +inf or NaN:
 * the comparison is false and nothing is discarded. */
RT_HD float rt_nearest_threshold(float best2, float eta, float sMin) {
    float t = (rt_sqrt(best2) + eta) / sMin;
    return (t * t) * RT_NEAR_SLACK;
}

#endif /* RT_POINT_QUERY_H */
