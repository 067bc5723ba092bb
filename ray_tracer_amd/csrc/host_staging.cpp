// host_staging.cpp — see host_staging.h. Host only: compiled into the library by hipcc and into tests/host_staging_check.cpp by g++.
#include "host_staging.h"

StageLayout stage_layout(const size_t* partBytes, int nParts) {
    StageLayout g{};
    if (nParts < 0 || nParts > (int)RT_STAGE_MAX_PARTS) return g;
    g.ok = true;
    for (int k = 0; k < nParts; k++) {
        g.offset[k] = g.bytes;
        g.bytes += (partBytes[k] + 255) & ~(size_t)255;
    }
    return g;
}
