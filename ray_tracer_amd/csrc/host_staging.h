// host_staging.h — how the parts of a _host call (its input arrays, its outputs) lie in the ctx staging buffer. The one rule:
//   the parts lie one behind the other in the order given;
//   each part starts at a multiple of 256 bytes;
//   a part of 0 bytes is absent: it takes no room, and its offset is the next part's (the total, behind the last one);
//   the total is a multiple of 256; all arithmetic is in size_t (2^30 - 1 records of 60 bytes are past 32 bits).
// Nothing in this pair of files needs a device. rt_device.hip's `staged` asks here and allocates, copies and launches;
// tests/host_staging_check.cpp pins the rule on the CPU with the part lists of every _host entry point. ("Staging")
#pragma once

#include <stddef.h>

enum { RT_STAGE_MAX_PARTS = 8 };   // the temporal form has 7

struct StageLayout {
    bool ok;                               // false: nParts outside 0 .. RT_STAGE_MAX_PARTS (nothing else is set)
    size_t offset[RT_STAGE_MAX_PARTS];     // of part k, k < nParts
    size_t bytes;                          // the buffer the parts need
};
StageLayout stage_layout(const size_t* partBytes, int nParts);
