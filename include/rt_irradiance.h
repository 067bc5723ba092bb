/*
 * rt_irradiance.h — the one rule of the baked-light queries (rt_query_irradiance, rt_query_sh_probes and their host forms
 * rt_irradiance_rays_host / rt_irradiance_gather_host), compiled by the host and by the device from this text: which rays a
 * point shoots, how their radiance is weighed, and in which order it is summed. rt_det_math.h's discipline holds: rt_*
 * primitives only, no contraction (-ffp-contract=off), a fixed evaluation order, so both sides get the same 32 bits.
 * ("Irradiance and SH probes")
 */
#ifndef RT_IRRADIANCE_H
#define RT_IRRADIANCE_H

#include "rt_ao_rays.h"

#define RT_IRR_LANES 64u            /* partial sums per point: sample s goes to partial s mod 64 */
#define RT_IRR_MAX_SAMPLES (1u << 24) /* samples < 2^24: (float)s is exact */
#define RT_SH9 9                    /* the real spherical harmonics of bands 0..2 */

/* the bits of a word in reverse order, by swaps of halves */
RT_HD uint32_t rt_bitreverse32(uint32_t v) {
    v = (v >> 16) | (v << 16);
    v = ((v & 0xff00ff00u) >> 8) | ((v & 0x00ff00ffu) << 8);
    v = ((v & 0xf0f0f0f0u) >> 4) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v & 0xccccccccu) >> 2) | ((v & 0x33333333u) << 2);
    v = ((v & 0xaaaaaaaau) >> 1) | ((v & 0x55555555u) << 1);
    return v;
}

/* The RNG id of sample s of point pid: the id rt_query_radiance seeds that ray with (32 bits, wrapping) */
RT_HD uint32_t rt_irr_ray_id(uint32_t pid, uint32_t s, uint32_t samples) { return pid * samples + s; }

/* The point's shift of the Hammersley set: two draws of the state rt_ao_state(pid, 0, seed) */
RT_HD void rt_irr_shift(uint32_t pid, uint32_t seed, float* u1, float* u2) {
    uint32_t st = rt_ao_state(pid, 0u, seed);
    *u1 = rt_random(&st);
    *u2 = rt_random(&st);
}

/* Sample s of `samples`: r1 = (s + u1) / S, the stratum of s jittered by the point's shift (in [0, 1]; 1 only where s + u1 rounds
 * up to S), and r2 = the radical inverse of s (24 bits) rotated by u2 (in [0, 1)) */
RT_HD void rt_irr_draws(uint32_t s, uint32_t samples, float u1, float u2, float* r1, float* r2) {
    *r1 = ((float)s + u1) / (float)samples;
    float v = (float)(rt_bitreverse32(s) >> 8) * 5.9604644775390625e-8f; /* 2^-24: exact */
    float r = v + u2;
    if (r >= 1.f) r = r - 1.f;
    *r2 = r;
}

/* cosineHemisphereDir's arithmetic about n, as rt_cosine_hemisphere_dir evaluates it, with the draws given: `radial` is the draw
 * under the square roots, `azimuth` the one that makes phi */
RT_HD rt_vec3 rt_irr_cosine_dir(rt_vec3 n, float radial, float azimuth) {
    float phi = (2.f * RT_PI) * azimuth;
    float sqrtR = rt_sqrt(radial);
    float sn, cs;
    rt_sincos(phi, &sn, &cs);
    float x = cs * sqrtR, y = sn * sqrtR, z = rt_sqrt(1.f - radial);
    rt_vec3 axis = rt_abs(rt_dot(n, rt_v3(1.f, 0.f, 0.f))) < 1.f ? rt_v3(1.f, 0.f, 0.f) : rt_v3(0.f, 0.f, 1.f);
    rt_vec3 tt = rt_normalize(rt_cross(n, axis));
    rt_vec3 bb = rt_cross(n, tt);
    return rt_add(rt_add(rt_scale(tt, x), rt_scale(bb, y)), rt_scale(n, z));
}

/* uniform on the sphere, in world axes: z = 1 - 2 r1, the circle of that height at angle 2 pi r2 */
RT_HD rt_vec3 rt_irr_sphere_dir(float r1, float r2) {
    float z = 1.f - 2.f * r1;
    float rho = rt_sqrt(rt_max(0.f, 1.f - z * z));
    float phi = (2.f * RT_PI) * r2;
    float sn, cs;
    rt_sincos(phi, &sn, &cs);
    return rt_v3(rho * cs, rho * sn, z);
}

/* The direction of sample s of a point with the shift (u1, u2): about n (cosine form), or on the sphere (n is not read) */
RT_HD rt_vec3 rt_irr_dir(int sphere, rt_vec3 n, uint32_t s, uint32_t samples, float u1, float u2) {
    float r1, r2;
    rt_irr_draws(s, samples, u1, u2, &r1, &r2);
    return sphere ? rt_irr_sphere_dir(r1, r2) : rt_irr_cosine_dir(n, r1, r2);
}

/* The origin: the next-ray origin of shading for the cosine form (p + (n * 1) * bias), p itself for a probe */
RT_HD rt_vec3 rt_irr_origin(int sphere, rt_vec3 p, rt_vec3 n, float bias) {
    return sphere ? p : rt_add(p, rt_scale(rt_scale(n, 1.f), bias));
}

/* The nine real spherical harmonics of bands 0..2 at the unit vector d, in the order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 */
RT_HD void rt_sh9(rt_vec3 d, float* y) {
    y[0] = 0.282095f;
    y[1] = 0.488603f * d.y;
    y[2] = 0.488603f * d.z;
    y[3] = 0.488603f * d.x;
    y[4] = 1.092548f * (d.x * d.y);
    y[5] = 1.092548f * (d.y * d.z);
    y[6] = 0.315392f * (3.f * (d.z * d.z) - 1.f);
    y[7] = 1.092548f * (d.x * d.z);
    y[8] = 0.546274f * (d.x * d.x - d.y * d.y);
}

/* What a finished sum becomes: E = pi * sum / S, c_j = 4 pi * sum / S */
RT_HD float rt_irr_scale(int sphere, float sum, uint32_t samples) {
    return ((sphere ? 4.f * RT_PI : RT_PI) * sum) / (float)samples;
}

/* rt_render's progressive blend (raytrace.comp:577-578) of one channel with what the output holds */
RT_HD float rt_irr_blend(float oldv, float v, uint32_t frameCount) {
    float weight = 1.f / ((float)frameCount + 1.f);
    return oldv * (1.f - weight) + v * weight;
}

/* The last step of the sum on the host: 64 partials to one by halves, partial[l] += partial[l + 32], then 16, ..., 1. (The
 * device does the same additions across the lanes of a wave.) */
RT_HD float rt_irr_fold(float* partial) {
    for (uint32_t half = RT_IRR_LANES / 2u; half >= 1u; half >>= 1)
        for (uint32_t l = 0; l < half; l++) partial[l] = partial[l] + partial[l + half];
    return partial[0];
}

#endif /* RT_IRRADIANCE_H */
