// cut_queries.h — the host logic of the cut queries (rt_query_cuts, rt_query_cuts_host) and the exhaustive host form
// (rt_cuts_exhaustive_host): the block and byte arithmetic of a batch and the choice of the search kernel's stack. What the
// entry points refuse is check_tris_query's (tri_queries.h), asked under their own names: the batch is the triangle queries'.
// Nothing in this pair of files needs a device. rt_device.hip gathers the facts, asks here, and allocates, copies and launches;
// tests/cut_queries_check.cpp pins every message and figure on the CPU, with made-up addresses. The rule itself is
// include/rt_tri_cut.h; key and list entries are include/rt_box_overlap.h's.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"
#include "tri_queries.h"

// A batch of n triangles with k slots each on the device (size_t throughout): the search runs one lane per triangle in
// work-groups of `threads` and writes the records itself
struct CutsShape {
    uint32_t blocks;      // ceil(n / threads)
    size_t cornerBytes;   // 36 n
    size_t outBytes;      // sizeof(RtCut) n k
    size_t countBytes;    // 4 n
    size_t listBytes;     // the deep search's key lists: the triangle queries'
};
CutsShape cuts_shape(uint32_t n, uint32_t k, uint32_t threads);

// The stack k_tris_cut needs for a scene whose deepest leaf is at maxLeafDepth: it is k_tris_overlap's descent, so tris_stack's
// answer, with the refusal naming this kernel
uint32_t cuts_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);
