// ray_queries.cpp — see ray_queries.h. Host only: compiled into the library by hipcc and into tests/ray_queries_check.cpp by g++.
#include "ray_queries.h"

#include "rt_ao_rays.h"

std::string check_ray_query(const char* fn, bool sceneUploaded, const RtRayBatch* rays, const void* out) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!rays) return f + ": the batch is NULL";
    if (rays->n == 0) return "";
    if (!rays->origins || !rays->dirs || !out) return f + ": origins, dirs and the output are required";
    if (rays->n >= (uint32_t)RT_QUERY_MAX_SLOTS) return f + ": a batch of " + std::to_string(rays->n) + " rays does not fit the 30 bits of a slot id";
    return "";
}

QueryShape query_shape(uint32_t n, uint32_t threads) {
    QueryShape s;
    s.slots = n;
    s.blocks = (uint32_t)(((uint64_t)n + threads - 1) / threads);
    s.vecBytes = (size_t)n * 3 * sizeof(float);
    s.tmaxBytes = (size_t)n * sizeof(float);
    s.hitBytes = (size_t)n * sizeof(RtHit);
    s.occludedBytes = (size_t)n;
    s.queueBytes = (size_t)n * sizeof(uint32_t);
    return s;
}

std::string check_ao(const char* fn, bool sceneUploaded, uint32_t nPixels, const RtAoParams& p, const RtAovBuffers* aovs, bool ownedValid,
                     size_t ownedPixels) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (p.samples < 1u || p.samples > (uint32_t)RT_AO_MAX_SAMPLES) return f + ": samples must be 1.." + std::to_string((int)RT_AO_MAX_SAMPLES);
    if (!(p.radius > 0.f) || rt_isinf(p.radius)) return f + ": radius must be finite and > 0";
    if (nPixels == 0) return f + ": no pixels";
    if (nPixels >= (uint32_t)RT_QUERY_MAX_SLOTS) return f + ": " + std::to_string(nPixels) + " pixels do not fit the 30 bits of a slot id";
    if (aovs) {
        if (!aovs->position || !aovs->normalDepth || !aovs->ids) return f + ": the planes need position, normalDepth and ids";
    } else {
        if (!ownedValid) return f + ": no ctx-owned AOV planes: rt_render_aovs was never called with d_out = NULL";
        if (ownedPixels != nPixels) return f + ": the ctx-owned AOV planes hold " + std::to_string(ownedPixels) + " pixels, not " + std::to_string(nPixels);
    }
    return "";
}

extern "C" {

void rt_ao_params_default(RtAoParams* p) {
    if (p) *p = RtAoParams{4u, 0.5f, 0u};
}

int rt_ao_rays_host(uint32_t nPixels, const RtAovBuffers* aovs, const RtAoParams* params, uint32_t sample, float* origins, float* dirs,
                    uint8_t* valid) {
    if (!aovs || !params || !origins || !dirs || !valid) return -1;
    if (!check_ao("rt_ao_rays_host", true, nPixels, *params, aovs, false, 0).empty() || sample >= params->samples) return -1;
    const float* pos = aovs->position;
    const float* nd = aovs->normalDepth;
    const uint32_t* ids = aovs->ids;
    for (uint32_t i = 0; i < nPixels; i++) {
        rt_vec3 o = rt_v3(0.f, 0.f, 0.f), d = rt_v3(0.f, 0.f, 0.f);
        const size_t r = (size_t)i * 4;
        valid[i] = rt_ao_ray(rt_v3(pos[r], pos[r + 1], pos[r + 2]), rt_v3(nd[r], nd[r + 1], nd[r + 2]), ids[r + 3], i, sample, params->seed, &o, &d) ? 1 : 0;
        origins[(size_t)i * 3] = o.x; origins[(size_t)i * 3 + 1] = o.y; origins[(size_t)i * 3 + 2] = o.z;
        dirs[(size_t)i * 3] = d.x; dirs[(size_t)i * 3 + 1] = d.y; dirs[(size_t)i * 3 + 2] = d.z;
    }
    return 0;
}

}  // extern "C"
