// texel_queries.h — the host logic of the lightmap texel passes (rt_bake_texels, rt_texels_compact, rt_texels_scatter,
// rt_dilate_texels, rt_bake_lightmap): what they refuse, in which order and with which words, the launch shapes and the byte
// counts of their ctx scratch, the levels of the exclusive scan, and the host forms of the rule (rt_texels_exhaustive_host,
// rt_dilate_texels_host; include/rt_texels.h). Nothing in this pair of files needs a device, and the checks and the arithmetic
// never dereference an array. rt_device.hip gathers the facts, asks here, and allocates and launches; tests/texels_check.cpp pins
// every message and figure on the CPU, with made-up addresses. ("Lightmap texels")
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"

enum { RT_TEXEL_THREADS = 256, RT_TEXEL_SCAN_BLOCK = 256, RT_TEXEL_MAX_LEVELS = 6 };

// What a bake (fn) refuses before anything is allocated or written, in this order: no uploaded scene; a NULL output; object >=
// the object count; width or height 0 or > 8192; a mesh whose triangles are not one contiguous range (triTotal == ~0u; the caller
// passes the object's RootInfo.triTotal, anything when the object is out of range). Empty: accepted.
std::string check_texel_bake(const char* fn, bool sceneUploaded, const void* out, uint32_t object, uint32_t objectCount, uint32_t width,
                             uint32_t height, uint32_t triTotal);
// rt_bake_lightmap after those: NULL params; progressive; dilatePasses > 254; a NULL fill plane. (rt_query_irradiance's own come next.)
std::string check_lightmap(const char* fn, const RtIrradianceParams* params, uint32_t dilatePasses, const void* fill);
// rt_texels_compact, rt_texels_scatter, rt_dilate_texels: a NULL array (allRequired: none of the call's arrays is NULL); nTexels
// 0 or > 8192 x 8192 (a width or height 0 or > 8192); nCovered > nTexels; passes > 254
std::string check_texel_pass(const char* fn, bool allRequired, uint64_t nTexels, uint32_t nCovered, uint32_t passes);
std::string check_texel_size(const char* fn, uint32_t width, uint32_t height);

// groups of `threads` lanes that give every one of n items a lane
uint32_t texel_groups(uint64_t n, uint32_t threads);

// The exclusive scan of n values runs level by level: level 0 scans blocks of 256 values and leaves one sum per block, level 1 scans
// those sums, and so on until a level has a single value (at least two levels, so that the sums of level 0 are always scanned:
// the compaction reads them). count[l]: the values of level l (count[0] = n), offset[l]: where level l's sums (the values of
// level l + 1) start in the scratch, in elements; elems: the scratch's size. 2^28 + 1 values take five levels.
struct ScanLevels { int levels; uint64_t count[RT_TEXEL_MAX_LEVELS], offset[RT_TEXEL_MAX_LEVELS]; uint64_t elems; };
ScanLevels scan_levels(uint64_t n);

// The ctx scratch of a bake over nTris triangles and a width x height map, each part 256-byte aligned: the statistics (4 words),
// the owner plane (4 bytes per texel), the overlapped plane (1 byte per texel), the block counts (4 bytes per triangle and one
// more), their exclusive scan (8 bytes per triangle and one more: the last entry is the total), the scan's sums (8 bytes each)
struct TexelScratch { size_t stats, owner, overlapped, counts, offsets, sums, bytes; };
TexelScratch texel_scratch(uint32_t nTris, uint32_t width, uint32_t height);

// The ctx scratch of rt_bake_lightmap over n = width x height texels: the records (48 n), the compacted points and normals (12 n
// each) and index (4 n), the count (one word), the irradiance values (16 n)
struct LightmapScratch { size_t texels, points, normals, index, count, values, bytes; };
LightmapScratch lightmap_scratch(uint32_t width, uint32_t height);
