/*
 * rt_ao_rays.h — the one rule that makes the rays of the ambient-occlusion pass (rt_render_ao, rt_ao_rays_host), compiled by the
 * host and by the device from this text. rt_det_math.h's discipline holds: rt_* primitives only, no contraction
 * (-ffp-contract=off), a fixed evaluation order, so both sides get the same 32 bits.
 */
#ifndef RT_AO_RAYS_H
#define RT_AO_RAYS_H

#include "rt_det_math.h"

/* The rt_random state of record i's sample `sample` under `seed`: two steps of rt_random's own generator (an odd multiplier and an
 * odd increment: a bijection of the 32-bit words), the sample and the seed mixed in between. For a fixed (sample, seed) different
 * records get different states, and for a fixed record different samples do. */
RT_HD uint32_t rt_ao_state(uint32_t i, uint32_t sample, uint32_t seed) {
    uint32_t h = i * 747796405u + 2891336453u;
    h ^= sample;
    h = h * 747796405u + 2891336453u;
    h ^= seed * 2654435769u;
    return h;
}

/* cosineHemisphereDir (raytrace.comp:405-424) about `n`, with the arithmetic of shade_path's diffuse branch */
RT_HD rt_vec3 rt_cosine_hemisphere_dir(rt_vec3 n, uint32_t* state) {
    float r1 = rt_random(state);
    float r2 = rt_random(state);
    float phi = (2.f * RT_PI) * r1;
    float sqrtR2 = rt_sqrt(r2);
    float sn, cs;
    rt_sincos(phi, &sn, &cs);
    float x = cs * sqrtR2, y = sn * sqrtR2, z = rt_sqrt(1.f - r2);
    rt_vec3 axis = rt_abs(rt_dot(n, rt_v3(1.f, 0.f, 0.f))) < 1.f ? rt_v3(1.f, 0.f, 0.f) : rt_v3(0.f, 0.f, 1.f);
    rt_vec3 tt = rt_normalize(rt_cross(n, axis));
    rt_vec3 bb = rt_cross(n, tt);
    return rt_add(rt_add(rt_scale(tt, x), rt_scale(bb, y)), rt_scale(n, z));
}

/* The ray of record i (position.xyz, normalDepth.xyz and ids.w of the first-hit planes). false: the record has no hit and shoots
 * nothing. The origin is the next-ray origin of shading: hitPoint + (normal * 1) * 0.00001. */
RT_HD bool rt_ao_ray(rt_vec3 position, rt_vec3 normal, uint32_t idsW, uint32_t i, uint32_t sample, uint32_t seed, rt_vec3* origin,
                     rt_vec3* dir) {
    if (!(idsW & 1u)) return false;
    uint32_t state = rt_ao_state(i, sample, seed);
    *origin = rt_add(position, rt_scale(rt_scale(normal, 1.f), 0.00001f));
    *dir = rt_cosine_hemisphere_dir(normal, &state);
    return true;
}

#endif /* RT_AO_RAYS_H */
