// tri_queries.h — the host logic of the triangle queries (rt_query_triangles, rt_query_triangles_host) and the exhaustive host
// form (rt_tris_exhaustive_host): what they refuse, in which order and with which words, the block and byte arithmetic of a batch
// and the choice of the search kernel's stack. Nothing in this pair of files needs a device: the checks do pointer arithmetic
// only and never dereference an array of a batch. rt_device.hip gathers the facts, asks here, and allocates, copies and
// launches; tests/tri_queries_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule itself (the
// triangle and sphere tests, the pruning comparisons) is include/rt_tri_overlap.h; key and records are include/rt_box_overlap.h's.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_TRIS_MAX_TRIS = 1 << 30 };   // as a box batch's: one lane per triangle, indices and block counts stay in 32 bits

// What a triangle entry point (fn) refuses before anything is allocated or written, in check_boxes_query's order: no uploaded
// scene; a NULL batch; corners NULL with n > 0; k > RT_BOXES_MAX_K; counts NULL, or out NULL with k > 0; n >= 2^30. Empty:
// accepted (n == 0 is, whatever the pointers and k).
std::string check_tris_query(const char* fn, bool sceneUploaded, const RtTriangleBatch* tris, uint32_t k, const void* out, const void* counts);

// A batch of n triangles with k slots each on the device (size_t throughout): the search runs one lane per triangle in
// work-groups of `threads` and writes the records itself
struct TrisShape {
    uint32_t blocks;      // ceil(n / threads)
    size_t cornerBytes;   // 36 n
    size_t outBytes;      // sizeof(RtOverlap) n k
    size_t countBytes;    // 4 n
    size_t listBytes;     // the deep search's lists: RT_BOXES_MAX_K entries of 2 words for every lane of every work-group
};
TrisShape tris_shape(uint32_t n, uint32_t k, uint32_t threads);

// The stack k_tris_overlap needs for a scene whose deepest leaf is at maxLeafDepth: siblings only, one per level, so boxes_stack's
// rule (box_queries.h) decides: RT_BOXES_STACK, RT_BOXES_STACK_DEEP, or 0 with the refusal in *error
uint32_t tris_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
