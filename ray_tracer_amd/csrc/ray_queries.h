// ray_queries.h — the host logic of the ray queries (rt_query_closest, rt_query_occluded and their _host forms) and of the
// ambient-occlusion pass (rt_render_ao, rt_ao_rays_host): what they refuse, in which order and with which words, and the slot and
// byte arithmetic of a batch. Nothing in this pair of files needs a device: it does pointer arithmetic only and never dereferences
// an array of a batch or a plane. rt_device.hip gathers the facts, asks here, and allocates, copies and launches;
// tests/ray_queries_check.cpp pins every message and figure on the CPU, with made-up addresses.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_QUERY_MAX_SLOTS = 1 << 30 };   // a batch's rays live in path-state slots [0, n): slot ids have 30 bits (a queue entry is slot * 4 + kind)
enum { RT_AO_MAX_SAMPLES = 64 };

// What a query entry point (fn) refuses before anything is allocated or written: no uploaded scene; a NULL batch; origins, dirs
// or the output NULL with n > 0; n >= 2^30. Empty: accepted (n == 0 is, whatever the pointers: the call does nothing).
std::string check_ray_query(const char* fn, bool sceneUploaded, const RtRayBatch* rays, const void* out);

// A batch of n rays on the device: one lane per ray in work-groups of `threads`, and the bytes of its arrays (size_t: 2^30 - 1
// records of sizeof(RtHit) bytes are past 32 bits)
struct QueryShape {
    uint32_t slots;          // path-state slots the pass uses: [0, slots)
    uint32_t blocks;         // work-groups of the per-ray kernels
    size_t vecBytes;         // origins, dirs: 12 n
    size_t tmaxBytes;        // 4 n
    size_t hitBytes;         // sizeof(RtHit) n
    size_t occludedBytes;    // n
    size_t queueBytes;       // the pass's queue: 4 n
};
QueryShape query_shape(uint32_t n, uint32_t threads);

// What rt_render_ao and rt_ao_rays_host (fn) refuse, in this order: no uploaded scene (rt_render_ao only: sceneUploaded is true for
// the host function); samples outside 1..RT_AO_MAX_SAMPLES or a radius that is not finite and > 0; nPixels 0 or >= 2^30; planes
// given without position, normalDepth or ids; none given and no ctx-owned planes of nPixels records (ownedValid, ownedPixels).
std::string check_ao(const char* fn, bool sceneUploaded, uint32_t nPixels, const RtAoParams& p, const RtAovBuffers* aovs, bool ownedValid,
                     size_t ownedPixels);
