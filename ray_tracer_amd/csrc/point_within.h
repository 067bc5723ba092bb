// point_within.h — the host logic of the radius point queries (rt_query_within, rt_query_within_host) and the exhaustive host
// form (rt_within_exhaustive_host): what they refuse, in which order and with which words, the block and byte arithmetic of a
// batch and the choice of the search kernel's stack. Nothing in this pair of files needs a device: the checks do pointer
// arithmetic only and never dereference an array of a batch. rt_device.hip gathers the facts, asks here, and allocates, copies
// and launches; tests/point_within_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule itself
// (membership, the key, the record of a member) is include/rt_point_within.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_WITHIN_STACK = 24, RT_WITHIN_STACK_DEEP = 64 };   // entries of the two instantiations of k_points_within (point_queries.h: nearest_stack's pair)

// What a radius entry point (fn) refuses before anything is allocated or written: check_point_query itself, with two more tests
// between its pointer test and its size test: no uploaded scene; a NULL batch; points NULL with n > 0; k > RT_WITHIN_MAX_K; counts
// NULL, or out NULL with k > 0; n >= 2^30. Empty: accepted (n == 0 is, whatever the pointers and k).
std::string check_within_query(const char* fn, bool sceneUploaded, const RtPointBatch* points, uint32_t k, const void* out, const void* counts);

// A batch of n points with k slots each on the device (size_t throughout: 2^30 - 1 points of 8 records are past 32 bits): the
// search runs one lane per point, the resolve one lane per slot, in work-groups of `threads`
struct WithinShape {
    uint32_t searchBlocks;   // ceil(n / threads)
    uint32_t resolveBlocks;  // ceil(n k / threads); 0 with k == 0: no resolve
    size_t pointBytes;       // 12 n
    size_t limitBytes;       // 4 n
    size_t outBytes;         // sizeof(RtNearest) n k
    size_t countBytes;       // 4 n
    size_t listBytes;        // the deep search's lists: RT_WITHIN_MAX_K entries of 3 words for every lane of every work-group
};
WithinShape within_shape(uint32_t n, uint32_t k, uint32_t threads);

// The stack k_points_within needs for a scene whose deepest leaf is at maxLeafDepth: far siblings only, one per level, so
// nearest_stack's rule (point_queries.h) decides: RT_WITHIN_STACK, RT_WITHIN_STACK_DEEP, or 0 with the refusal in *error
uint32_t within_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
