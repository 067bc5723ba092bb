/*
 * rt_obb_overlap.h — the rule of the oriented box queries (rt_query_oriented_boxes, rt_obbs_exhaustive_host): which surfaces a
 * box placed by a frame touches. One text for both sides, under rt_det_math.h's discipline (RT_HD, -ffp-contract=off, rt_* math
 * only): the device kernel (k_obbs_overlap) and the exhaustive host loop compile these very functions. The box machinery is
 * rt_box_overlap.h's, included and called, not copied: rt_box_triangle, rt_box_sphere, the key, rt_box_insert, the record.
 *
 * Declared semantics ("Oriented box queries"). Box i is the set { p : lo <= F p <= hi }, closed; F is the world-to-box
 * frame, sixteen floats in RenderObject.transformMatrix's layout (column-major), of which twelve are read (m[3], m[7], m[11] and
 * m[15] never are), and F p is rt_xform_point(F, p) in fp32: rt_obb_point below is that expression over the frame held as rows,
 * bit for bit (tests/obb_queries_check.cpp compares them). F need not be orthonormal or invertible: a singular frame is not
 * refused, the rule applies as written. A box is valid when the twelve frame numbers that are read are finite and
 * rt_box_valid(lo, hi) holds; any other box is not searched and has no member.
 *  - Surfaces are rt_query_nearest's. A triangle's world corners are rt_xform_point(fwd, v) in fp32 (an identity object's corners
 *    as they are). A linear map takes triangles to triangles, so a triangle is a member when rt_box_triangle(lo, hi, F a, F b, F c)
 *    keeps it (rt_obb_triangle).
 *  - A sphere is a member when rt_box_sphere(lo, hi, F centre, fl(r s)) keeps it (rt_obb_sphere), s = rt_sqrt((m[0] m[0] + m[1]
 *    m[1]) + m[2] m[2]) the length of the frame's first column. This is the geometry of the shell exactly when the linear part of
 *    F is a rotation or reflection times a uniform scale (the image of the sphere is then the sphere of radius r s about F centre).
 *    For any other frame the image is an ellipsoid and this is the formula above and no more.
 *  - With an identity frame the frame step is exact (products with 1 and 0, sums with 0; s = 1), so on scenes with finite corners
 *    the answer is rt_query_boxes' in every byte.
 * Order, records, k and counts are rt_query_boxes': rt_box_insert, rt_box_record.
 */
#ifndef RT_OBB_OVERLAP_H
#define RT_OBB_OVERLAP_H

#include "rt_box_overlap.h"

#define RT_OBB_FRAME_FLOATS 16u /* floats of one frame in a batch */

/* the frame as the three rows of its 3 x 4 part: row d = (m[d], m[4 + d], m[8 + d]) and t = (m[12], m[13], m[14]) */
typedef struct RtObbFrame { rt_vec3 r0, r1, r2, t; } RtObbFrame;

RT_HD RtObbFrame rt_obb_frame(const float* m) {
    RtObbFrame f;
    f.r0 = rt_v3(m[0], m[4], m[8]); f.r1 = rt_v3(m[1], m[5], m[9]); f.r2 = rt_v3(m[2], m[6], m[10]);
    f.t = rt_v3(m[12], m[13], m[14]);
    return f;
}
RT_HD RtObbFrame rt_obb_identity(void) {
    RtObbFrame f;
    f.r0 = rt_v3(1.f, 0.f, 0.f); f.r1 = rt_v3(0.f, 1.f, 0.f); f.r2 = rt_v3(0.f, 0.f, 1.f); f.t = rt_v3(0.f, 0.f, 0.f);
    return f;
}
RT_HD bool rt_obb_finite3(rt_vec3 v) { return rt_box_finite(v.x) && rt_box_finite(v.y) && rt_box_finite(v.z); }
/* the twelve numbers that are read are finite, and the local box is a valid box */
RT_HD bool rt_obb_valid(RtObbFrame f, rt_vec3 lo, rt_vec3 hi) {
    return rt_obb_finite3(f.r0) && rt_obb_finite3(f.r1) && rt_obb_finite3(f.r2) && rt_obb_finite3(f.t) && rt_box_valid(lo, hi);
}

/* F p: rt_xform_point's sums over the rows */
RT_HD rt_vec3 rt_obb_point(RtObbFrame f, rt_vec3 p) {
    return rt_v3(((f.r0.x * p.x + f.r0.y * p.y) + f.r0.z * p.z) + f.t.x,
                 ((f.r1.x * p.x + f.r1.y * p.y) + f.r1.z * p.z) + f.t.y,
                 ((f.r2.x * p.x + f.r2.y * p.y) + f.r2.z * p.z) + f.t.z);
}
/* the length of the frame's first column */
RT_HD float rt_obb_scale(RtObbFrame f) { return rt_sqrt((f.r0.x * f.r0.x + f.r1.x * f.r1.x) + f.r2.x * f.r2.x); }

/* a, b, c: the WORLD corners */
RT_HD bool rt_obb_triangle(RtObbFrame f, rt_vec3 lo, rt_vec3 hi, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    return rt_box_triangle(lo, hi, rt_obb_point(f, a), rt_obb_point(f, b), rt_obb_point(f, c));
}
/* scale: rt_obb_scale(f), taken once per box */
RT_HD bool rt_obb_sphere(RtObbFrame f, float scale, rt_vec3 lo, rt_vec3 hi, rt_vec3 centre, float r) {
    return rt_box_sphere(lo, hi, rt_obb_point(f, centre), r * scale);
}

/* ---------------------------------------------------------------- pruning (the device descent only; DESIGN.md, "Oriented box
 * queries", has the count). A member triangle passed stage 1 of rt_box_triangle on its fp32 frame corners z = fl(F w), w its fp32
 * world corner. A subtree is discarded only when a box known to hold every such z lies strictly apart from [lo, hi]: the test is
 * rt_box_placed_apart (rt_box_overlap.h) with the rows of a map G in place of an object's matrix, G c +- |G| e over the node's
 * box, padded by rt_obb_pad(mag).
 *  - Identity object: w is the node box's own number, G = F. z lies within 4 u mag of F w, the projection costs 7 u mag more:
 *    11 u mag, mag >= |F| |[w; 1]| over the object's root box (rt_obb_mag).
 *  - Placed object: G = fl(F M), g = fl(F t + s), composed once per lane and object (rt_obb_compose). With b >= |F| (|M| |[v; 1]|)
 *    + |s|: the two roundings in a row move z by at most 8 u b from G v + g, the composition by 4 u b, the projection by 7 u b:
 *    19 u b. rt_obb_mag_placed bounds b from layout_nearest's scale of the object, which bounds every component of |M| |[v; 1]|.
 * RT_OBB_PAD is 64 u for both, a constant of its own: RT_BOX_PAD's 32 u would leave the placed count 13 u for its second-order
 * terms and the rounding of the magnitude itself; 64 u leaves 45 u. A larger pad costs time, never correctness. A magnitude of +inf
 * gives a pad of +inf, one of NaN (0 x inf) a pad of NaN: every comparison with either is false, and nothing is discarded. */
#define RT_OBB_PAD 3.814697265625e-06f /* 64 u = 2^-18 */
RT_HD float rt_obb_pad(float mag) { return RT_OBB_PAD * mag + 1.17549435e-38f; }

RT_HD float rt_obb_mag_row(rt_vec3 row, float t, rt_vec3 a) { return ((rt_abs(row.x) * a.x + rt_abs(row.y) * a.y) + rt_abs(row.z) * a.z) + rt_abs(t); }
/* |F| |[w; 1]| over the box [blo, bhi], the largest component */
RT_HD float rt_obb_mag(RtObbFrame f, rt_vec3 blo, rt_vec3 bhi) {
    rt_vec3 a = rt_v3(rt_max(rt_abs(blo.x), rt_abs(bhi.x)), rt_max(rt_abs(blo.y), rt_abs(bhi.y)), rt_max(rt_abs(blo.z), rt_abs(bhi.z)));
    return rt_max(rt_max(rt_obb_mag_row(f.r0, f.t.x, a), rt_obb_mag_row(f.r1, f.t.y, a)), rt_obb_mag_row(f.r2, f.t.z, a));
}
/* |F| (objMag, objMag, objMag) + |s|: objMag bounds every component of |M| |[v; 1]| over the object */
RT_HD float rt_obb_mag_placed(RtObbFrame f, float objMag) { return rt_obb_mag(f, rt_v3(objMag, objMag, objMag), rt_v3(objMag, objMag, objMag)); }

/* G = F M, g = F t + s in fp32, M given as its rows m0, m1, m2 and translation mt */
RT_HD rt_vec3 rt_obb_compose_row(rt_vec3 fr, rt_vec3 m0, rt_vec3 m1, rt_vec3 m2) {
    return rt_v3((fr.x * m0.x + fr.y * m1.x) + fr.z * m2.x, (fr.x * m0.y + fr.y * m1.y) + fr.z * m2.y, (fr.x * m0.z + fr.y * m1.z) + fr.z * m2.z);
}
RT_HD RtObbFrame rt_obb_compose(RtObbFrame f, rt_vec3 m0, rt_vec3 m1, rt_vec3 m2, rt_vec3 mt) {
    RtObbFrame g;
    g.r0 = rt_obb_compose_row(f.r0, m0, m1, m2); g.r1 = rt_obb_compose_row(f.r1, m0, m1, m2); g.r2 = rt_obb_compose_row(f.r2, m0, m1, m2);
    g.t = rt_obb_point(f, mt);
    return g;
}
/* the box [blo, bhi] taken through g lies strictly apart from [lo, hi] on one of the box's axes */
RT_HD bool rt_obb_apart(rt_vec3 lo, rt_vec3 hi, RtObbFrame g, rt_vec3 blo, rt_vec3 bhi, float pad) {
    return rt_box_placed_apart(lo, hi, g.r0, g.r1, g.r2, g.t, blo, bhi, pad);
}

#endif /* RT_OBB_OVERLAP_H */
