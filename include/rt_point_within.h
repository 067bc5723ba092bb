/*
 * rt_point_within.h — the rule of the radius point queries (rt_query_within, rt_within_exhaustive_host): which surfaces lie
 * within a point's reach, in which order they are reported, and the record of one. One text for both sides, under
 * rt_det_math.h's discipline (RT_HD, -ffp-contract=off, rt_* math only), the way rt_point_query.h and rt_ray_hits.h are shared:
 * the device kernels (k_points_within, k_points_within_resolve) and the exhaustive host loop compile these very functions, so a
 * member's squared distance and its record have the same bits on both.
 *
 * Declared semantics ("Radius point queries"). Point i has the reach R (maxDist[i]; none when the array is NULL) and
 * the bound R2 = rt_nearest_start(...): fl(R * R), +inf without a reach; a reach that is NaN or <= 0 means no search. Its member
 * set C: every sphere that is a surface (rt_sphere_is_surface) whose rt_point_sphere squared distance is STRICTLY < R2, and every
 * triangle of every object whose rt_point_triangle squared distance is < R2, the world corners placed as rt_query_nearest
 * places them. R2 never shrinks, so C is a function of the point and the scene alone: not of the visiting order, the BVH, the
 * stack or any knob. The key that orders C is rt_ray_hits.h's (rt_hits_before) on {d2, primitive word, triangle}: the squared
 * distance as an fp32 compare; spheres before triangles; the lower sphere or object index; the lower triangle index. The
 * primitive word of a triangle is its object index, that of a sphere rt_hits_sphere_word(index, false). The key is total, so
 * the reported primitives are particular ones, unlike rt_query_nearest's.
 */
#ifndef RT_POINT_WITHIN_H
#define RT_POINT_WITHIN_H

#include "rt_amd.h"
#include "rt_point_query.h"
#include "rt_ray_hits.h"

/* membership: strictly below the constant bound (a NaN distance is no member) */
RT_HD bool rt_within_member(float d2, float R2) { return d2 < R2; }

/* the primitive word of a list entry */
RT_HD uint32_t rt_within_sphere_word(uint32_t index) { return rt_hits_sphere_word(index, false); }
RT_HD uint32_t rt_within_triangle_word(uint32_t object) { return object; }

/* the record of a slot without a member: rt_query_nearest's not-found record. (Every field by name, the struct has no hole: a
 * memset here, in a second kernel of the device module, reorders instructions of k_ray_hits_resolve: tools/disasm_compare.py.) */
RT_HD RtNearest rt_within_not_found(void) {
    RtNearest r;
    r.dst = RT_MISS_DST;
    r.found = 0u; r.isSphere = 0u; r.objectIndex = 0u; r.triIndex = 0u;
    r.uv[0] = 0.f; r.uv[1] = 0.f;
    r.point[0] = 0.f; r.point[1] = 0.f; r.point[2] = 0.f;
    r._pad[0] = 0u; r._pad[1] = 0u;
    return r;
}

/* The record of a member, from the point and the primitive: what rt_query_nearest builds when it reports that primitive. d2 is
 * the squared distance the search listed (the value rt_point_sphere / rt_point_triangle return for these very arguments). */
RT_HD RtNearest rt_within_sphere_record(rt_vec3 q, rt_vec3 centre, float radius, uint32_t index, float d2) {
    RtNearest r = rt_within_not_found();
    rt_vec3 p;
    (void)rt_point_sphere(q, centre, radius, &p);
    r.dst = rt_sqrt(d2);
    r.found = 1u; r.isSphere = 1u; r.objectIndex = index;
    r.point[0] = p.x; r.point[1] = p.y; r.point[2] = p.z;
    return r;
}
/* a, b, c: the WORLD corners (rt_xform_point(fwd, v) in fp32; an identity object's corners as they are) */
RT_HD RtNearest rt_within_triangle_record(rt_vec3 q, rt_vec3 a, rt_vec3 b, rt_vec3 c, uint32_t object, uint32_t tri, float d2) {
    RtNearest r = rt_within_not_found();
    float u, v;
    (void)rt_point_triangle(q, a, b, c, &u, &v);
    const rt_vec3 p = rt_bary_point(a, b, c, u, v);
    r.dst = rt_sqrt(d2);
    r.found = 1u; r.objectIndex = object; r.triIndex = tri;
    r.uv[0] = u; r.uv[1] = v;
    r.point[0] = p.x; r.point[1] = p.y; r.point[2] = p.z;
    return r;
}

#endif /* RT_POINT_WITHIN_H */
