/*
 * rt_box_overlap.h — the rule of the box queries (rt_query_boxes, rt_boxes_exhaustive_host): which surfaces an axis-aligned box
 * touches, in which order they are reported, and the record of one. One text for both sides, under rt_det_math.h's discipline
 * (RT_HD, -ffp-contract=off, rt_* math only), the way rt_point_within.h is shared: the device kernel (k_boxes_overlap) and the
 * exhaustive host loop compile these very functions, so a pair's verdict is the same on both.
 *
 * Declared semantics ("Box queries"). The surfaces are rt_query_nearest's: every sphere with rt_sphere_is_surface, and
 * every triangle of every object, its world corners rt_xform_point(fwd, v) in fp32 (an identity object's corners as they are).
 * No frontOnly, no materials, no alpha maps. A box is valid when its six numbers are finite and lo <= hi on every axis (flat and
 * point boxes are); any other box is not searched and has no member. Boxes are closed: touching counts, every "separated"
 * decision is a strict inequality, and an axis that comes out zero separates nothing. A comparison with a NaN operand is false,
 * so NaN separates nothing on a triangle's axes (a triangle with a NaN corner is a member unless an axis of finite numbers
 * separates it), and a sphere whose distances or radius are NaN is no member (both of its comparisons must hold).
 *  - Triangle (rt_box_triangle): the 13-axis separating-axis test in a fixed order. (1) The three box axes by comparisons alone:
 *    out when max(a_i, b_i, c_i) < lo_i or min(a_i, b_i, c_i) > hi_i. Exact. (2) centre = fl(lo 0.5 + hi 0.5), half =
 *    fl(hi 0.5 - lo 0.5) (no overflow for finite input), the corners relative to the centre, the plane axis e0 x e1: out when
 *    |n . v0| > half . |n|. (3) The nine axes e_j x unit_i, each the two-term projection of two corners against half . |axis|.
 *    A triangle with two equal corners has one edge exactly zero and an exactly zero normal: those axes separate nothing and the
 *    six left are the complete test of its segment; with three equal corners stage 1 alone decides for its point.
 *  - Sphere (rt_box_sphere): the surface is the shell. Member iff d2min <= fl(r r) <= d2max, d2min = rt_point_box2(centre, lo,
 *    hi), d2max the squared distance to the farthest corner summed per axis in x, y, z order. A box wholly inside the ball does
 *    not touch its surface.
 * The member set is a function of the box and the scene alone. Its order is rt_ray_hits.h's key (rt_hits_before) with a constant
 * first word: spheres before triangles, the lower sphere or object index, the lower triangle index. A list entry is two words
 * {primitive word, triangle}: the primitive word of a triangle is its object index, that of a sphere rt_hits_sphere_word(index,
 * false). rt_box_insert is rt_hits_insert's insertion over entries without the distance word.
 */
#ifndef RT_BOX_OVERLAP_H
#define RT_BOX_OVERLAP_H

#include "rt_amd.h"
#include "rt_point_query.h"
#include "rt_ray_hits.h"

#define RT_BOX_WORDS 2u /* words of a list entry */

RT_HD bool rt_box_finite(float x) { return (rt_f2u(x) & 0x7fffffffu) < 0x7f800000u; }
/* six finite numbers, lo <= hi on every axis */
RT_HD bool rt_box_valid(rt_vec3 lo, rt_vec3 hi) {
    return rt_box_finite(lo.x) && rt_box_finite(lo.y) && rt_box_finite(lo.z) && rt_box_finite(hi.x) && rt_box_finite(hi.y) &&
           rt_box_finite(hi.z) && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
}

/* the interval [min(p, q), max(p, q)] lies strictly outside [-r, r] (NaN: false) */
RT_HD bool rt_box_axis_out(float p, float q, float r) { return rt_min(p, q) > r || rt_max(p, q) < -r; }

/* the three axes e x unit_i of one edge e; v and w: a corner of the edge and the corner opposite it, relative to the centre */
RT_HD bool rt_box_edge_out(rt_vec3 e, rt_vec3 v, rt_vec3 w, rt_vec3 h) {
    float ax = rt_abs(e.x), ay = rt_abs(e.y), az = rt_abs(e.z);
    if (rt_box_axis_out(e.z * v.y - e.y * v.z, e.z * w.y - e.y * w.z, h.y * az + h.z * ay)) return true;   /* e x unit_x */
    if (rt_box_axis_out(e.x * v.z - e.z * v.x, e.x * w.z - e.z * w.x, h.x * az + h.z * ax)) return true;   /* e x unit_y */
    return rt_box_axis_out(e.y * v.x - e.x * v.y, e.y * w.x - e.x * w.y, h.x * ay + h.y * ax);             /* e x unit_z */
}

/* stage 1 alone: the box of the corners against the box, by comparisons (exact; what the pruning is derived from) */
RT_HD bool rt_box_triangle_stage1(rt_vec3 lo, rt_vec3 hi, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    if (rt_max(rt_max(a.x, b.x), c.x) < lo.x || rt_min(rt_min(a.x, b.x), c.x) > hi.x) return false;
    if (rt_max(rt_max(a.y, b.y), c.y) < lo.y || rt_min(rt_min(a.y, b.y), c.y) > hi.y) return false;
    if (rt_max(rt_max(a.z, b.z), c.z) < lo.z || rt_min(rt_min(a.z, b.z), c.z) > hi.z) return false;
    return true;
}

/* a, b, c: the WORLD corners. true: the closed box [lo, hi] (valid) and the closed triangle touch */
RT_HD bool rt_box_triangle(rt_vec3 lo, rt_vec3 hi, rt_vec3 a, rt_vec3 b, rt_vec3 c) {
    if (!rt_box_triangle_stage1(lo, hi, a, b, c)) return false;
    rt_vec3 m = rt_v3(lo.x * 0.5f + hi.x * 0.5f, lo.y * 0.5f + hi.y * 0.5f, lo.z * 0.5f + hi.z * 0.5f);
    rt_vec3 h = rt_v3(hi.x * 0.5f - lo.x * 0.5f, hi.y * 0.5f - lo.y * 0.5f, hi.z * 0.5f - lo.z * 0.5f);
    rt_vec3 v0 = rt_sub(a, m), v1 = rt_sub(b, m), v2 = rt_sub(c, m);
    rt_vec3 e0 = rt_sub(v1, v0), e1 = rt_sub(v2, v1), e2 = rt_sub(v0, v2);
    rt_vec3 n = rt_cross(e0, e1);
    float d = rt_dot(n, v0);
    float r = (h.x * rt_abs(n.x) + h.y * rt_abs(n.y)) + h.z * rt_abs(n.z);
    if (rt_box_axis_out(d, d, r)) return false;
    if (rt_box_edge_out(e0, v0, v2, h)) return false;
    if (rt_box_edge_out(e1, v1, v0, h)) return false;
    if (rt_box_edge_out(e2, v2, v1, h)) return false;
    return true;
}

/* the squared distance from p to the farthest corner of [lo, hi] */
RT_HD float rt_box_far2(rt_vec3 p, rt_vec3 lo, rt_vec3 hi) {
    float fx = rt_max(p.x - lo.x, hi.x - p.x);
    float fy = rt_max(p.y - lo.y, hi.y - p.y);
    float fz = rt_max(p.z - lo.z, hi.z - p.z);
    return (fx * fx + fy * fy) + fz * fz;
}
/* true: the closed box touches the shell of the sphere */
RT_HD bool rt_box_sphere(rt_vec3 lo, rt_vec3 hi, rt_vec3 centre, float r) {
    float r2 = r * r;
    return rt_point_box2(centre, lo, hi) <= r2 && r2 <= rt_box_far2(centre, lo, hi);
}

RT_HD uint32_t rt_box_sphere_word(uint32_t index) { return rt_hits_sphere_word(index, false); }
RT_HD uint32_t rt_box_triangle_word(uint32_t object) { return object; }

/* One member into a list sorted by the key that keeps the first k: rt_hits_insert over entries {primitive word, triangle}, the
 * distance word being the same for all (rt_hits_before decides with 0 on both sides). Entry e's word w lies at
 * list[(e * RT_BOX_WORDS + w) * stride]. */
RT_HD uint32_t rt_box_insert(uint32_t* list, uint32_t stride, uint32_t k, uint32_t have, uint32_t prim, uint32_t tri) {
    if (k == 0u) return 0u;
    uint32_t pos = have;
    if (have == k) {
        const uint32_t* last = list + (size_t)(k - 1u) * RT_BOX_WORDS * stride;
        if (!rt_hits_before(0.f, prim, tri, 0.f, last[0], last[stride])) return have;
        pos = k - 1u;
    } else {
        have++;
    }
    while (pos > 0u) {
        uint32_t* prev = list + (size_t)(pos - 1u) * RT_BOX_WORDS * stride;
        if (!rt_hits_before(0.f, prim, tri, 0.f, prev[0], prev[stride])) break;
        uint32_t* here = prev + (size_t)RT_BOX_WORDS * stride;
        here[0] = prev[0]; here[stride] = prev[stride];
        pos--;
    }
    uint32_t* at = list + (size_t)pos * RT_BOX_WORDS * stride;
    at[0] = prim; at[stride] = tri;
    return have;
}

/* the record of a slot without a member (all 0), and of a member, from its list entry */
RT_HD RtOverlap rt_box_no_member(void) {
    RtOverlap r;
    r.found = 0u; r.isSphere = 0u; r.objectIndex = 0u; r.triIndex = 0u;
    return r;
}
RT_HD RtOverlap rt_box_record(uint32_t prim, uint32_t tri) {
    RtOverlap r;
    r.found = 1u;
    r.isSphere = rt_hits_is_sphere(prim) ? 1u : 0u;
    r.objectIndex = rt_hits_is_sphere(prim) ? rt_hits_sphere_index(prim) : prim;
    r.triIndex = rt_hits_is_sphere(prim) ? 0u : tri;
    return r;
}

/* ---------------------------------------------------------------- pruning (the device descent only; DESIGN.md, "Box queries",
 * has the derivation). A member triangle passed stage 1, so the box of its fp32 world corners meets the query box under exact
 * comparisons. rt_box_apart is that comparison between two boxes: for an identity object the node boxes hold the very corners,
 * so it discards only non-members, with no pad. */
RT_HD bool rt_box_apart(rt_vec3 lo, rt_vec3 hi, rt_vec3 blo, rt_vec3 bhi) {
    return bhi.x < lo.x || blo.x > hi.x || bhi.y < lo.y || blo.y > hi.y || bhi.z < lo.z || blo.z > hi.z;
}
/* For a placed object: the fp32 world corners of everything below a node lie within 4 u mag of the exact image of the node's
 * box, which fits in M centre +- |M| extent; computing that in fp32 costs 7 u mag more (the count is in DESIGN.md). The pad is
 * 32 u mag and the smallest normal number beside it for the underflow of a product. mag: layout_nearest's scale (+inf: the pad is
 * +inf and nothing is discarded). */
#define RT_BOX_PAD 1.9073486328125e-06f /* 32 u = 2^-19 */
RT_HD float rt_box_pad(float mag) { return RT_BOX_PAD * mag + 1.17549435e-38f; }
/* one axis: row (x, y, z) and translation t of the forward matrix; c, e: centre and half-extent of the node's box */
RT_HD bool rt_box_placed_axis_out(float lo, float hi, rt_vec3 row, float t, rt_vec3 c, rt_vec3 e, float pad) {
    float C = ((row.x * c.x + row.y * c.y) + row.z * c.z) + t;
    float E = (rt_abs(row.x) * e.x + rt_abs(row.y) * e.y) + rt_abs(row.z) * e.z;
    return (C + E) + pad < lo || (C - E) - pad > hi;
}
RT_HD bool rt_box_placed_apart(rt_vec3 lo, rt_vec3 hi, rt_vec3 r0, rt_vec3 r1, rt_vec3 r2, rt_vec3 t, rt_vec3 blo, rt_vec3 bhi, float pad) {
    rt_vec3 c = rt_v3(blo.x * 0.5f + bhi.x * 0.5f, blo.y * 0.5f + bhi.y * 0.5f, blo.z * 0.5f + bhi.z * 0.5f);
    rt_vec3 e = rt_v3(bhi.x * 0.5f - blo.x * 0.5f, bhi.y * 0.5f - blo.y * 0.5f, bhi.z * 0.5f - blo.z * 0.5f);
    return rt_box_placed_axis_out(lo.x, hi.x, r0, t.x, c, e, pad) || rt_box_placed_axis_out(lo.y, hi.y, r1, t.y, c, e, pad) ||
           rt_box_placed_axis_out(lo.z, hi.z, r2, t.z, c, e, pad);
}
/* the object's world box (layout_nearest's), padded the same way for a placed object */
RT_HD bool rt_box_object_apart(rt_vec3 lo, rt_vec3 hi, rt_vec3 olo, rt_vec3 ohi, float pad) {
    return ohi.x + pad < lo.x || olo.x - pad > hi.x || ohi.y + pad < lo.y || olo.y - pad > hi.y || ohi.z + pad < lo.z || olo.z - pad > hi.z;
}

#endif /* RT_BOX_OVERLAP_H */
