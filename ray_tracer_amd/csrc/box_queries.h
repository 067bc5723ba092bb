// box_queries.h — the host logic of the box queries (rt_query_boxes, rt_query_boxes_host) and the exhaustive host form
// (rt_boxes_exhaustive_host): what they refuse, in which order and with which words, the block and byte arithmetic of a batch
// and the choice of the search kernel's stack. Nothing in this pair of files needs a device: the checks do pointer arithmetic
// only and never dereference an array of a batch. rt_device.hip gathers the facts, asks here, and allocates, copies and
// launches; tests/box_queries_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule itself (the
// triangle and sphere tests, the key, the record of a member, the pruning comparisons) is include/rt_box_overlap.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_BOXES_MAX_BOXES = 1 << 30 };   // as a point batch's: one lane per box, indices and block counts stay in 32 bits
enum { RT_BOXES_STACK = 24, RT_BOXES_STACK_DEEP = 64 };   // entries of the two instantiations of k_boxes_overlap (point_queries.h: nearest_stack's pair)

// What a box entry point (fn) refuses before anything is allocated or written, in check_within_query's order: no uploaded scene; a
// NULL batch; lo or hi NULL with n > 0; k > RT_BOXES_MAX_K; counts NULL, or out NULL with k > 0; n >= 2^30. Empty: accepted
// (n == 0 is, whatever the pointers and k).
std::string check_boxes_query(const char* fn, bool sceneUploaded, const RtBoxBatch* boxes, uint32_t k, const void* out, const void* counts);

// A batch of n boxes with k slots each on the device (size_t throughout: 2^30 - 1 boxes of 8 records are past 32 bits): the search
// runs one lane per box in work-groups of `threads` and writes the records itself
struct BoxesShape {
    uint32_t blocks;      // ceil(n / threads)
    size_t cornerBytes;   // 12 n, lo and hi each
    size_t outBytes;      // sizeof(RtOverlap) n k
    size_t countBytes;    // 4 n
    size_t listBytes;     // the deep search's lists: RT_BOXES_MAX_K entries of 2 words for every lane of every work-group
};
BoxesShape boxes_shape(uint32_t n, uint32_t k, uint32_t threads);

// The stack k_boxes_overlap needs for a scene whose deepest leaf is at maxLeafDepth: siblings only, one per level, so
// nearest_stack's rule (point_queries.h) decides: RT_BOXES_STACK, RT_BOXES_STACK_DEEP, or 0 with the refusal in *error
uint32_t boxes_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
