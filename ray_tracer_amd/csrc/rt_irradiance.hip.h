// rt_irradiance.hip.h — the two kernels of the baked-light queries (rt_query_irradiance, rt_query_sh_probes; DESIGN.md,
// "Irradiance and SH probes") around the radiance pipeline: k_irradiance_rays makes a chunk's rays by the rule of
// include/rt_irradiance.h into the ctx scratch, radiance_device() traces them as one piece, k_irradiance_gather sums each point's
// records in the rule's order. SPHERE: the probe form (directions on the sphere, nine SH coefficients per channel).
#pragma once

#include "rt_irradiance.h"

#define RT_IRR_BLOCK 256   // four waves: four points per work-group of k_irradiance_gather

struct IrradianceArgs {
    const float* points;      // the batch: packed, 3 floats per point
    const float* normals;     // likewise (not read by the probe form)
    const uint32_t* ids;      // per point of the batch, or NULL: the point's index
    uint32_t first, count;    // the chunk: points [first, first + count) of the batch, its rays [0, count x samples) of the scratch
    uint32_t samples, seed;   // seed: frameCount
    float bias;
    float* origins;           // the scratch: RtRayBatch's packed layout, the ray ids, the radiance records
    float* dirs;
    uint32_t* rayIds;
    const float4* radiance;
    float* out;               // the batch's result: 4 (irradiance) or 27 (probes) floats per point
    uint32_t progressive, frameCount;
};

// One lane per ray of the chunk: ray r is sample r % samples of point first + r / samples
template <bool SPHERE>
__global__ __launch_bounds__(RT_IRR_BLOCK) void k_irradiance_rays(IrradianceArgs a) {
    const uint32_t r = blockIdx.x * RT_IRR_BLOCK + threadIdx.x;
    if (r >= a.count * a.samples) return;
    const uint32_t k = r / a.samples, s = r - k * a.samples;
    const size_t i = (size_t)a.first + k;
    const uint32_t pid = a.ids ? a.ids[i] : (uint32_t)i;
    const float* const pp = a.points + 3 * i;
    const rt_vec3 p = rt_v3(pp[0], pp[1], pp[2]);
    rt_vec3 n = rt_v3(0.f, 0.f, 0.f);
    if (!SPHERE) {
        const float* const np = a.normals + 3 * i;
        n = rt_v3(np[0], np[1], np[2]);
    }
    float u1, u2;
    rt_irr_shift(pid, a.seed, &u1, &u2);
    const rt_vec3 o = rt_irr_origin(SPHERE ? 1 : 0, p, n, a.bias);
    const rt_vec3 d = rt_irr_dir(SPHERE ? 1 : 0, n, s, a.samples, u1, u2);
    float* const po = a.origins + 3 * (size_t)r;
    float* const pd = a.dirs + 3 * (size_t)r;
    po[0] = o.x; po[1] = o.y; po[2] = o.z;
    pd[0] = d.x; pd[1] = d.y; pd[2] = d.z;
    a.rayIds[r] = rt_irr_ray_id(pid, s, a.samples);
}

// partial[l] += partial[l ^ half] on every lane; lane l < half holds partial[l] + partial[l + half], the rule's fold
__device__ __forceinline__ float irr_fold_wave(float v) {
#pragma unroll
    for (int half = 32; half >= 1; half >>= 1) v = v + __shfl_xor(v, half, 64);
    return v;
}

// One wave per point. Lane l walks the samples l, l + 64, ...: one 16-byte record each, a wave's loads contiguous; the probe form
// makes the sample's direction again from the rule for the SH weights. The 64 partial sums fold across the lanes and lane 0 scales,
// blends and stores.
template <bool SPHERE>
__global__ __launch_bounds__(RT_IRR_BLOCK) void k_irradiance_gather(IrradianceArgs a) {
    const uint32_t k = blockIdx.x * (RT_IRR_BLOCK / 64) + threadIdx.x / 64;   // wave-uniform
    if (k >= a.count) return;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = (size_t)a.first + k;
    const float4* const rec = a.radiance + (size_t)k * a.samples;
    constexpr int NSUMS = SPHERE ? 3 * RT_SH9 : 3;
    float sum[NSUMS];
#pragma unroll
    for (int j = 0; j < NSUMS; j++) sum[j] = 0.f;
    float u1 = 0.f, u2 = 0.f;
    if (SPHERE) rt_irr_shift(a.ids ? a.ids[i] : (uint32_t)i, a.seed, &u1, &u2);
    for (uint32_t s = lane; s < a.samples; s += 64u) {
        const float4 L = rec[s];
        if (SPHERE) {
            float y[RT_SH9];
            rt_sh9(rt_irr_dir(1, rt_v3(0.f, 0.f, 0.f), s, a.samples, u1, u2), y);
#pragma unroll
            for (int j = 0; j < RT_SH9; j++) {
                sum[3 * j] = sum[3 * j] + L.x * y[j];
                sum[3 * j + 1] = sum[3 * j + 1] + L.y * y[j];
                sum[3 * j + 2] = sum[3 * j + 2] + L.z * y[j];
            }
        } else {
            sum[0] = sum[0] + L.x;
            sum[1] = sum[1] + L.y;
            sum[2] = sum[2] + L.z;
        }
    }
#pragma unroll
    for (int j = 0; j < NSUMS; j++) sum[j] = irr_fold_wave(sum[j]);
    if (lane != 0u) return;
    float* const o = a.out + i * (SPHERE ? 3 * RT_SH9 : 4);
#pragma unroll
    for (int j = 0; j < NSUMS; j++) {
        const float v = rt_irr_scale(SPHERE ? 1 : 0, sum[j], a.samples);
        sum[j] = a.progressive ? rt_irr_blend(o[j], v, a.frameCount) : v;
    }
    if (SPHERE) {
#pragma unroll
        for (int j = 0; j < NSUMS; j++) o[j] = sum[j];
    } else {
        *(float4*)o = make_float4(sum[0], sum[1], sum[2], 1.f);   // (16-byte aligned, as rt_query_radiance's output)
    }
}
