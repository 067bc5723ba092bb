/*
 * rt_ray_hits.h — the rule of the all-hit ray queries (rt_query_hits, rt_hits_walk_host): which primitives a ray crosses below
 * its limit, and in which order they are reported. One text for both sides, under rt_det_math.h's discipline (RT_HD,
 * -ffp-contract=off, rt_* math only), the way rt_point_query.h is shared: the device kernel (k_ray_hits) and the host walk
 * compile these very functions, so a candidate's distance has the same 32 bits on both.
 *
 * Declared semantics ("All-hit ray queries"). Ray i with the limit T (tmax[i]; RT_MISS_DST when tmax is NULL) has
 * the candidate set C: what calculateIntersections (raytrace.comp:276-353) accepts when its bound is the constant T and never
 * shrinks.
 *  - A sphere gives up to two candidates, from sphereIntersection's arithmetic: the entry root (b - sqrtd) / a, a front face, and
 *    the exit root (b + sqrtd) / a, a back face; each counts when it is >= 0 and < T. From inside only the exit exists.
 *  - Objects in index order, the ray taken to object space by inverse(transformMatrix); the object's root is entered untested, a
 *    child box is entered when its slab distance is < T, a triangle is a candidate when the triangle test says didHit, dst < T
 *    and its alpha texel does not cut it out.
 * T is constant, so C does not depend on the order anything is visited in. The key that orders C, compared lexicographically:
 * dst (fp32 compare); spheres before triangles; the lower sphere or object index; the lower triangle index; a sphere's entry
 * before its exit. A list entry is three words {dst, primitive word, triangle}: the primitive word is the object index of a
 * triangle, or RT_HITS_SPHERE | index << 1 | exit for a sphere root.
 */
#ifndef RT_RAY_HITS_H
#define RT_RAY_HITS_H

#include "rt_det_math.h"

#define RT_HITS_SPHERE 0x80000000u
#define RT_HITS_EMPTY 0xffffffffu /* the primitive word of a slot without a candidate */
#define RT_HITS_WORDS 3u          /* words of a list entry */

RT_HD uint32_t rt_hits_sphere_word(uint32_t index, bool exit) { return RT_HITS_SPHERE | (index << 1) | (exit ? 1u : 0u); }
RT_HD bool rt_hits_is_sphere(uint32_t prim) { return (prim & RT_HITS_SPHERE) != 0u; }
RT_HD uint32_t rt_hits_sphere_index(uint32_t prim) { return (prim & ~RT_HITS_SPHERE) >> 1; }
RT_HD bool rt_hits_sphere_exit(uint32_t prim) { return (prim & 1u) != 0u; }

/* the limit of a ray; *search = false: count 0 and miss records without a search (a limit that is NaN or <= 0) */
RT_HD float rt_hits_start(bool hasLimit, float tmax, bool* search) {
    float T = hasLimit ? tmax : RT_MISS_DST;
    *search = T > 0.f;
    return T;
}

/* raytrace.comp:195-224, the distance part, both roots. false: the ray's line misses the sphere (or a NaN discriminant). The
 * roots are not yet held against 0 or T (rt_hits_accepts). */
RT_HD bool rt_hits_sphere_roots(rt_vec3 centre, float radius, rt_vec3 ro, rt_vec3 rd, float* tEntry, float* tExit) {
    rt_vec3 oc = rt_sub(centre, ro);
    float a = rt_dot(rd, rd);
    float b = rt_dot(oc, rd);
    float c = rt_dot(oc, oc) - radius * radius;
    float disc = b * b - a * c;
    if (!(disc >= 0.f)) return false;
    float sq = rt_sqrt(disc);
    *tEntry = (b - sq) / a;
    *tExit = (b + sq) / a;
    return true;
}
/* a root or a triangle distance that counts: >= 0 (NaN does not) and below the limit */
RT_HD bool rt_hits_accepts(float dst, float T) { return dst >= 0.f && dst < T; }

/* raytrace.comp:227-247, tri_intersect's operations in its order */
typedef struct RtHitsTri { bool didHit, frontFace; float dst, u, v, w; } RtHitsTri;
RT_HD RtHitsTri rt_hits_triangle(rt_vec3 ro, rt_vec3 rd, rt_vec3 v0, rt_vec3 v1, rt_vec3 v2, bool frontOnly) {
    rt_vec3 v1v0 = rt_sub(v1, v0);
    rt_vec3 v2v0 = rt_sub(v2, v0);
    rt_vec3 rov0 = rt_sub(ro, v0);
    rt_vec3 n = rt_cross(v1v0, v2v0);
    rt_vec3 q = rt_cross(rov0, rd);
    float d0 = -rt_dot(rd, n);
    float d = 1.f / d0;
    RtHitsTri h;
    h.dst = rt_dot(rov0, n) * d;
    h.u = rt_dot(v2v0, q) * d;
    h.v = -rt_dot(v1v0, q) * d;
    h.w = 1.f - h.u - h.v;
    h.frontFace = d0 >= 0.00000001f;
    h.didHit = h.dst >= 0.f && h.u >= 0.f && h.v >= 0.f && h.w >= 0.f && !(!h.frontFace && frontOnly);
    return h;
}

/* raytrace.comp:263-274, box_intersect's operations in its order: the distance the ray enters the box at, or RT_MISS_DST */
RT_HD float rt_hits_box(rt_vec3 lo, rt_vec3 hi, rt_vec3 ro, rt_vec3 inv) {
    float ax = (lo.x - ro.x) * inv.x, ay = (lo.y - ro.y) * inv.y, az = (lo.z - ro.z) * inv.z;
    float bx = (hi.x - ro.x) * inv.x, by = (hi.y - ro.y) * inv.y, bz = (hi.z - ro.z) * inv.z;
    float tNear = rt_max(rt_max(rt_min(ax, bx), rt_min(ay, by)), rt_min(az, bz));
    float tFar = rt_min(rt_min(rt_max(ax, bx), rt_max(ay, by)), rt_max(az, bz));
    bool hit = tFar >= tNear && tFar > 0.f;
    return hit ? (tNear > 0.f ? tNear : 0.f) : RT_MISS_DST;
}

/* the key: is candidate a reported before candidate b? Spheres sort below objects with the top bit turned round; a sphere's word
 * already orders index, then entry before exit, and its triangle word is 0. */
RT_HD bool rt_hits_before(float aDst, uint32_t aPrim, uint32_t aTri, float bDst, uint32_t bPrim, uint32_t bTri) {
    if (aDst < bDst) return true;
    if (bDst < aDst) return false;
    uint32_t ap = aPrim ^ RT_HITS_SPHERE, bp = bPrim ^ RT_HITS_SPHERE;
    if (ap != bp) return ap < bp;
    return aTri < bTri;
}

/* One candidate into a list sorted by the key that keeps the first k: entry e's word w lies at list[(e * RT_HITS_WORDS + w) *
 * stride] (stride 1 on the host, the wave's 64 lanes on the device). `have` entries are valid (min(candidates so far, k));
 * returns the new `have`. With k entries held, a candidate that does not come before the last one is dropped, else the last one is. */
RT_HD uint32_t rt_hits_insert(uint32_t* list, uint32_t stride, uint32_t k, uint32_t have, float dst, uint32_t prim, uint32_t tri) {
    if (k == 0u) return 0u;
    uint32_t pos = have;
    if (have == k) {
        const uint32_t* last = list + (size_t)(k - 1u) * RT_HITS_WORDS * stride;
        if (!rt_hits_before(dst, prim, tri, rt_u2f(last[0]), last[stride], last[2u * stride])) return have;
        pos = k - 1u;
    } else {
        have++;
    }
    while (pos > 0u) {
        uint32_t* prev = list + (size_t)(pos - 1u) * RT_HITS_WORDS * stride;
        if (!rt_hits_before(dst, prim, tri, rt_u2f(prev[0]), prev[stride], prev[2u * stride])) break;
        uint32_t* here = prev + (size_t)RT_HITS_WORDS * stride;
        here[0] = prev[0]; here[stride] = prev[stride]; here[2u * stride] = prev[2u * stride];
        pos--;
    }
    uint32_t* at = list + (size_t)pos * RT_HITS_WORDS * stride;
    at[0] = rt_f2u(dst); at[stride] = prim; at[2u * stride] = tri;
    return have;
}

#endif /* RT_RAY_HITS_H */
