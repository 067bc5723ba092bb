// radiance_queries.cpp — see radiance_queries.h. Host only: compiled into the library by hipcc and into
// tests/radiance_queries_check.cpp by g++.
#include "radiance_queries.h"

#include <algorithm>

#include "rt_det_math.h"

std::string check_radiance_query(const char* fn, bool sceneUploaded, const RtRayBatch* rays, const RtRadianceParams* params, const void* out) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!rays || !params) return f + ": the batch and the params are required";
    if (rays->n == 0) return "";
    if (!rays->origins || !rays->dirs || !out) return f + ": origins, dirs and the output are required";
    if (rays->tmax) return f + ": tmax must be NULL (a path has no reach limit)";
    if (params->samples == 0) return f + ": samples must be >= 1";
    if (params->bounceLimit >= (uint32_t)RT_RADIANCE_BOUNCE_LIMIT) return f + ": bounceLimit needs more than 28 bits";
    if (rays->n >= (uint32_t)RT_RADIANCE_MAX_SLOTS) return f + ": a batch of " + std::to_string(rays->n) + " rays does not fit the 30 bits of a slot id";
    return "";
}

uint32_t radiance_piece_cap(uint64_t maxSlots) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(maxSlots, 1), (uint64_t)RT_RADIANCE_MAX_SLOTS - 1);
}

uint32_t radiance_piece_count(uint32_t n, uint64_t maxSlots) {
    const uint64_t cap = radiance_piece_cap(maxSlots);
    return (uint32_t)(((uint64_t)n + cap - 1) / cap);
}

RadiancePiece radiance_piece(uint32_t n, uint64_t maxSlots, uint32_t k) {
    const uint64_t cap = radiance_piece_cap(maxSlots);
    const uint64_t first = std::min<uint64_t>((uint64_t)k * cap, n);
    return RadiancePiece{(uint32_t)first, (uint32_t)std::min<uint64_t>(cap, (uint64_t)n - first)};
}

RadianceShape radiance_shape(uint32_t n, bool hasIds) {
    return RadianceShape{(size_t)n * 3 * sizeof(float), hasIds ? (size_t)n * sizeof(uint32_t) : 0, (size_t)n * 4 * sizeof(float)};
}

uint32_t radiance_starting_seed(uint32_t frameCount) {
    uint32_t lol = frameCount;
    return (uint32_t)(rt_random(&lol) * 23892183.f);
}

extern "C" {

void rt_radiance_params_default(RtRadianceParams* p) {
    if (p) *p = RtRadianceParams{1u, 8u, 0u, 0u};
}

}  // extern "C"
