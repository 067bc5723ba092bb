// sweep_queries.h — the host logic of the sphere sweeps (rt_query_sweep, rt_query_sweep_host) and the exhaustive host form
// (rt_sweep_exhaustive_host): what they refuse, in which order and with which words, the block and byte arithmetic of a batch
// and the choice of the kernel's stack. Nothing in this pair of files needs a device: the checks do pointer arithmetic only and
// never dereference an array of a batch. rt_device.hip gathers the facts, asks here, and allocates, copies and launches;
// tests/sweep_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule itself (a primitive's contact
// time, the acceptance, the key, the record, the pruning test) is include/rt_sweep.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_SWEEP_MAX_RAYS = 1 << 30 };   // as a ray batch's: one lane per ray, indices and block counts stay in 32 bits
enum { RT_SWEEP_STACK = 24, RT_SWEEP_STACK_DEEP = 64 };   // entries of the two instantiations of k_sweep_spheres (point_queries.h: nearest_stack's pair)

// What a sweep entry point (fn) refuses before anything is allocated or written, in check_ray_query's order and words: no
// uploaded scene; a NULL batch; origins, dirs, radius or the output NULL with n > 0; n >= 2^30. Empty: accepted (n == 0 is,
// whatever the pointers).
std::string check_sweep_query(const char* fn, bool sceneUploaded, const RtSweepBatch* batch, const void* out);

// A batch of n rays on the device: one lane per ray in work-groups of `threads`, and the bytes of its arrays (size_t throughout:
// 2^30 - 1 records of 64 bytes are past 32 bits)
struct SweepShape {
    uint32_t blocks;       // ceil(n / threads)
    size_t vecBytes;       // 12 n: origins, dirs
    size_t scalarBytes;    // 4 n: radius, tmax
    size_t outBytes;       // sizeof(RtSweep) n
};
SweepShape sweep_shape(uint32_t n, uint32_t threads);

// The stack k_sweep_spheres needs for a scene whose deepest leaf is at maxLeafDepth: far siblings only, one per level, so
// nearest_stack's rule (point_queries.h) decides: RT_SWEEP_STACK, RT_SWEEP_STACK_DEEP, or 0 with the refusal in *error
uint32_t sweep_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
