// ray_hits.h — the host logic of the all-hit ray queries (rt_query_hits, rt_query_hits_host) and the host walk
// (rt_hits_walk_host): what they refuse, in which order and with which words, the block and byte arithmetic of a batch and the
// choice of the search kernel's stack. Nothing in this pair of files needs a device: the checks do pointer arithmetic only and
// never dereference an array of a batch. rt_device.hip gathers the facts, asks here, and allocates, copies and launches;
// tests/ray_hits_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule itself (the roots, the
// triangle and slab tests, the limit, the key, the list) is include/rt_ray_hits.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_HITS_STACK = 24, RT_HITS_STACK_DEEP = 64 };   // entries of the two instantiations of k_ray_hits (point_queries.h: nearest_stack's pair)

// What an all-hit entry point (fn) refuses before anything is allocated or written, in check_ray_query's order and words with two
// more tests after its NULL tests: no uploaded scene; a NULL batch; origins or dirs NULL with n > 0; k > RT_HITS_MAX_K; counts
// NULL, or hits NULL with k > 0; n >= 2^30. Empty: accepted (n == 0 is, whatever the pointers and k).
std::string check_hits_query(const char* fn, bool sceneUploaded, const RtRayBatch* rays, uint32_t k, const void* hits, const void* counts);

// A batch of n rays with k slots each on the device (size_t throughout: 2^30 - 1 rays of 8 records are past 32 bits): the search
// runs one lane per ray, the resolve one lane per slot, in work-groups of `threads`
struct HitsShape {
    uint32_t searchBlocks;   // ceil(n / threads)
    uint32_t resolveBlocks;  // ceil(n k / threads); 0 with k == 0: no resolve
    size_t vecBytes;         // origins, dirs: 12 n
    size_t tmaxBytes;        // 4 n
    size_t hitBytes;         // sizeof(RtHit) n k
    size_t countBytes;       // 4 n
    size_t listBytes;        // the deep search's lists: RT_HITS_MAX_K entries of 3 words for every lane of every work-group
};
HitsShape hits_shape(uint32_t n, uint32_t k, uint32_t threads);

// The stack k_ray_hits needs for a scene whose deepest leaf is at maxLeafDepth: far siblings only, one per level, so
// nearest_stack's rule (point_queries.h) decides: RT_HITS_STACK, RT_HITS_STACK_DEEP, or 0 with the refusal in *error
uint32_t hits_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
