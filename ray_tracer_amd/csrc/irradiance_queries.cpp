// irradiance_queries.cpp — see irradiance_queries.h. Host only: compiled into the library by hipcc and into
// tests/irradiance_check.cpp by g++ (with radiance_queries.cpp, whose piece cap the chunks are cut to).
#include "irradiance_queries.h"

#include <algorithm>

#include "radiance_queries.h"
#include "rt_irradiance.h"

namespace {
bool finite_f(float x) { return !rt_isnan(x) && !rt_isinf(x); }
bool samples_ok(uint32_t s) { return s >= 1u && s < (uint32_t)RT_IRR_MAX_SAMPLES; }
bool bias_ok(float b) { return finite_f(b) && b >= 0.f; }
rt_vec3 v3_at(const float* a, size_t i) { return rt_v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]); }
}  // namespace

std::string check_irradiance_query(const char* fn, bool sphere, bool sceneUploaded, const RtPointNormalBatch* batch,
                                   const RtIrradianceParams* params, const void* out, uint64_t maxSlots) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!batch || !params) return f + ": the batch and the params are required";
    if (batch->n == 0) return "";
    if (!batch->points || (!sphere && !batch->normals) || !out)
        return f + (sphere ? ": points and the output are required" : ": points, normals and the output are required");
    if (!samples_ok(params->samples)) return f + ": samples must be in 1 .. 2^24 - 1";
    if (params->bounceLimit >= (uint32_t)RT_RADIANCE_BOUNCE_LIMIT) return f + ": bounceLimit needs more than 28 bits";
    if (!bias_ok(params->bias)) return f + ": bias must be finite and >= 0";
    const uint32_t cap = radiance_piece_cap(maxSlots);
    if (params->samples > cap)
        return f + ": the " + std::to_string(params->samples) + " rays of a point do not fit a piece of " + std::to_string(cap) + " rays (radiance_max_kslots)";
    if (batch->n >= (uint32_t)RT_IRRADIANCE_MAX_POINTS) return f + ": a batch of " + std::to_string(batch->n) + " points does not fit the 30 bits of a slot id";
    return "";
}

uint32_t irradiance_chunk_points(uint32_t samples, uint64_t maxSlots) {
    return samples ? radiance_piece_cap(maxSlots) / samples : 0u;
}

uint32_t irradiance_chunk_count(uint32_t n, uint32_t samples, uint64_t maxSlots) {
    const uint64_t per = irradiance_chunk_points(samples, maxSlots);
    return per ? (uint32_t)(((uint64_t)n + per - 1) / per) : 0u;
}

IrradianceChunk irradiance_chunk(uint32_t n, uint32_t samples, uint64_t maxSlots, uint32_t k) {
    const uint64_t per = irradiance_chunk_points(samples, maxSlots);
    const uint64_t first = std::min<uint64_t>((uint64_t)k * per, n);
    return IrradianceChunk{(uint32_t)first, (uint32_t)std::min<uint64_t>(per, (uint64_t)n - first)};
}

IrradianceShape irradiance_shape(uint32_t n, bool hasIds, bool sphere) {
    return IrradianceShape{(size_t)n * 3 * sizeof(float), hasIds ? (size_t)n * sizeof(uint32_t) : 0,
                           (size_t)n * (sphere ? 3 * RT_SH9 : 4) * sizeof(float)};
}

IrradianceScratch irradiance_scratch(uint32_t rays) {
    const size_t r = rays;
    return IrradianceScratch{0, 16 * r, 28 * r, 40 * r, 44 * r};
}

extern "C" {

void rt_irradiance_params_default(RtIrradianceParams* p) {
    if (p) *p = RtIrradianceParams{64u, 8u, 0u, 0u, 0.00001f};
}

int rt_irradiance_rays_host(const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params, int sphere, uint32_t first,
                            uint32_t count, float* origins, float* dirs, uint32_t* rayIds) {
    if (!batch || !params || !origins || !dirs || !rayIds) return -1;
    if (!samples_ok(params->samples) || !bias_ok(params->bias)) return -1;
    if ((uint64_t)first + count > batch->n) return -1;
    if (count && (!batch->points || (!sphere && !batch->normals))) return -1;
    const uint32_t S = params->samples;
    for (uint32_t k = 0; k < count; k++) {
        const size_t i = (size_t)first + k;
        const uint32_t pid = ids ? ids[i] : (uint32_t)i;
        const rt_vec3 p = v3_at(batch->points, i), n = sphere ? rt_v3(0.f, 0.f, 0.f) : v3_at(batch->normals, i);
        float u1, u2;
        rt_irr_shift(pid, params->frameCount, &u1, &u2);
        const rt_vec3 o = rt_irr_origin(sphere, p, n, params->bias);
        for (uint32_t s = 0; s < S; s++) {
            const size_t r = (size_t)k * S + s;
            const rt_vec3 d = rt_irr_dir(sphere, n, s, S, u1, u2);
            origins[3 * r] = o.x; origins[3 * r + 1] = o.y; origins[3 * r + 2] = o.z;
            dirs[3 * r] = d.x; dirs[3 * r + 1] = d.y; dirs[3 * r + 2] = d.z;
            rayIds[r] = rt_irr_ray_id(pid, s, S);
        }
    }
    return 0;
}

int rt_irradiance_gather_host(const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params, int sphere,
                              const float* radiance, float* out) {
    if (!batch || !params) return -1;
    if (!samples_ok(params->samples)) return -1;
    if (batch->n && (!radiance || !out)) return -1;
    const uint32_t S = params->samples;
    const int nSums = sphere ? 3 * RT_SH9 : 3;
    for (size_t i = 0; i < batch->n; i++) {
        const uint32_t pid = ids ? ids[i] : (uint32_t)i;
        float u1, u2;
        rt_irr_shift(pid, params->frameCount, &u1, &u2);
        float partial[3 * RT_SH9][RT_IRR_LANES];
        for (int j = 0; j < nSums; j++)
            for (uint32_t l = 0; l < RT_IRR_LANES; l++) partial[j][l] = 0.f;
        for (uint32_t s = 0; s < S; s++) {
            const float* const L = radiance + 4 * (i * S + s);
            const uint32_t l = s % RT_IRR_LANES;
            if (sphere) {
                float y[RT_SH9];
                rt_sh9(rt_irr_dir(1, rt_v3(0.f, 0.f, 0.f), s, S, u1, u2), y);
                for (int j = 0; j < RT_SH9; j++)
                    for (int ch = 0; ch < 3; ch++) partial[3 * j + ch][l] = partial[3 * j + ch][l] + L[ch] * y[j];
            } else {
                for (int ch = 0; ch < 3; ch++) partial[ch][l] = partial[ch][l] + L[ch];
            }
        }
        float* const o = out + i * (sphere ? 3 * RT_SH9 : 4);
        for (int j = 0; j < nSums; j++) {
            const float v = rt_irr_scale(sphere, rt_irr_fold(partial[j]), S);
            o[j] = params->progressive ? rt_irr_blend(o[j], v, params->frameCount) : v;
        }
        if (!sphere) o[3] = 1.f;
    }
    return 0;
}

}  // extern "C"
