// obb_queries.h — the host logic of the oriented box queries (rt_query_oriented_boxes, rt_query_oriented_boxes_host) and the
// exhaustive host form (rt_obbs_exhaustive_host): what they refuse, in which order and with which words, the block and byte
// arithmetic of a batch and the choice of the search kernel's stack. Nothing in this pair of files needs a device: the checks do
// pointer arithmetic only and never dereference an array of a batch. rt_device.hip gathers the facts, asks here, and allocates,
// copies and launches; tests/obb_queries_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule
// itself (the frame and its arithmetic, the triangle and sphere tests through the frame, the pruning's pad) is
// include/rt_obb_overlap.h, over include/rt_box_overlap.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"
#include "box_queries.h"

// What an oriented box entry point (fn) refuses before anything is allocated or written, in check_boxes_query's order: no uploaded
// scene; a NULL batch; frames, lo or hi NULL with n > 0 ("frames, lo and hi are required"); k > RT_BOXES_MAX_K; sharedFrame > 1;
// counts NULL, or out NULL with k > 0; n >= 2^30. Empty: accepted (n == 0 is, whatever the pointers, k and sharedFrame).
std::string check_obbs_query(const char* fn, bool sceneUploaded, const RtObbBatch* batch, uint32_t k, const void* out, const void* counts);

// A batch of n boxes with k slots each on the device (size_t throughout): BoxesShape's figures and the frames
struct ObbShape {
    uint32_t blocks;      // ceil(n / threads)
    size_t frameBytes;    // 64 n, or 64 for a shared frame (0 for an empty batch)
    size_t cornerBytes;   // 12 n, lo and hi each
    size_t outBytes;      // sizeof(RtOverlap) n k
    size_t countBytes;    // 4 n
    size_t listBytes;     // the deep search's lists: RT_BOXES_MAX_K entries of 2 words for every lane of every work-group
};
ObbShape obbs_shape(uint32_t n, uint32_t k, bool sharedFrame, uint32_t threads);

// The stack k_obbs_overlap needs for a scene whose deepest leaf is at maxLeafDepth: boxes_stack's rule (siblings only, one per
// level): RT_BOXES_STACK, RT_BOXES_STACK_DEEP, or 0 with the refusal in *error
uint32_t obbs_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
