// rt_texels.hip.h — the kernels of the lightmap texel passes (rt_bake_texels, rt_texels_compact, rt_texels_scatter,
// rt_dilate_texels; DESIGN.md, "Lightmap texels"). The rule is include/rt_texels.h, the very functions the exhaustive host loop
// compiles. uv triangles differ in area by six orders of magnitude, so no kernel loops over a triangle's covered area: the work is
// cut into (triangle, 8 x 8-texel block) items, one wave each.
//   k_texel_bins     one lane per triangle of the object: the blocks its clipped bounding box touches (0 when it is skipped)
//   k_scan_local, k_scan_add   the exclusive scan of those counts (64-bit totals), level by level (texel_queries.h: scan_levels)
//   k_texel_cover    one wave per item, found by binary search in the scan; one lane per texel; atomicMin on the owner plane
//   k_texel_resolve  one lane per texel: the 48-byte record from the owner, three 16-byte stores; one wave per group, 16 runs of 64
//                    consecutive texels each, so the statistics are one atomic per group and counter without any LDS (with one
//                    run per group the 262 144 atomics on one address were 2.6 of the 3.0 ms of a 4096 x 4096 map)
//   k_texel_compact  one lane per texel: the covered ones to the front, in texel order, by the same scan
//   k_texel_scatter  one lane per covered texel: its value back into the map
//   k_texel_dilate   one lane per texel: one pass of rt_dilate_texel
// The only LDS is the scan's (one word pair per wave of a group).
#pragma once

#include "rt_kernels.hip.h"
#include "rt_texels.h"

#define RT_TEXEL_GROUP 256    // the groups of every kernel here but k_texel_resolve
#define RT_TEXEL_RESOLVE 64   // k_texel_resolve: one wave per group
#define RT_TEXEL_RESOLVE_RUNS 16u   // ... which takes 16 runs of 64 consecutive texels: a sixteenth of the atomics on the counters

struct TexelArgs {
    uint32_t object, triFirst, triCount;   // the object's triangles: [triFirst, triFirst + triCount)
    uint32_t width, height;
    uint32_t* owner;                       // width x height words: the lowest covering triangle, or RT_TEXEL_EMPTY
    uint8_t* overlapped;                   // width x height bytes: 1 where a second triangle covered the centre
    uint32_t* counts;                      // triCount + 1: the items of each triangle, and 0
    unsigned long long* offsets;           // triCount + 1: their exclusive scan; the last entry is the total
    uint32_t* stats;                       // RtTexelStats
    float4* out;                           // the records, 3 x float4 per texel
};

// ---------------------------------------------------------------- the exclusive scan
// within a wave by __shfl_up, across the waves of a group through LDS; the group's total goes to every lane
template <typename T>
__device__ __forceinline__ T scan_group_exclusive(T v, T* total) {
    __shared__ T s_wave[RT_TEXEL_GROUP / RT_WAVE];
    const uint32_t lane = threadIdx.x & (RT_WAVE - 1), wave = threadIdx.x / RT_WAVE;
    T incl = v;
#pragma unroll
    for (int o = 1; o < RT_WAVE; o <<= 1) {
        const T below = __shfl_up(incl, o, RT_WAVE);
        if (lane >= (uint32_t)o) incl += below;
    }
    if (lane == RT_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < RT_TEXEL_GROUP / RT_WAVE; w++) {
        const T s = s_wave[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();   // (the array is free for the next call)
    *total = all;
    return before + (incl - v);
}

struct ScanLoadU32 {
    const uint32_t* p;
    __device__ __forceinline__ unsigned long long operator()(size_t i) const { return p[i]; }
};
template <typename T>
struct ScanLoadSame {
    const T* p;
    __device__ __forceinline__ T operator()(size_t i) const { return p[i]; }
};
// 1 for a covered record (state is the fourth word of its first 16 bytes)
struct ScanLoadCovered {
    const float4* texels;
    __device__ __forceinline__ uint32_t operator()(size_t i) const { return __float_as_uint(texels[3 * i].w) != 0u ? 1u : 0u; }
};

// One level: excl[i] (when given; may be the array the loader reads) = the exclusive scan of value i within its block of 256, and
// sums[block] = the block's total
template <typename T, typename LOAD>
__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_scan_local(LOAD load, unsigned long long n, T* excl, T* sums) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RT_TEXEL_GROUP + threadIdx.x;
    const T v = i < n ? (T)load((size_t)i) : (T)0;
    T total;
    const T e = scan_group_exclusive<T>(v, &total);
    if (excl && i < n) excl[i] = e;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// ... and the scanned sums added back
template <typename T>
__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_scan_add(T* excl, unsigned long long n, const T* sums) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RT_TEXEL_GROUP + threadIdx.x;
    if (i < n) excl[i] += sums[blockIdx.x];
}

// ---------------------------------------------------------------- the bake
__device__ __forceinline__ void texel_uv(const DevScene& sc, uint32_t tri, float* uv) {
    const float4 a = sc.triUV[2 * (size_t)tri], b = sc.triUV[2 * (size_t)tri + 1];   // {u0 v0 u1 v1} {u2 v2}
    uv[0] = a.x; uv[1] = a.y; uv[2] = a.z; uv[3] = a.w; uv[4] = b.x; uv[5] = b.y;
}

__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_texel_bins(DevScene sc, TexelArgs a) {
    const uint32_t i = blockIdx.x * RT_TEXEL_GROUP + threadIdx.x;
    bool skipped = false;
    if (i <= a.triCount) {
        uint32_t blocks = 0;
        if (i < a.triCount) {
            float uv[6];
            texel_uv(sc, a.triFirst + i, uv);
            blocks = rt_texel_tri_blocks(uv, a.width, a.height, &skipped);
        }
        a.counts[i] = blocks;
    }
    const unsigned long long m = __ballot(skipped);
    if (m && lane_id() == 0) atomicAdd(&a.stats[2], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_texel_cover(DevScene sc, TexelArgs a) {
    const unsigned long long total = a.offsets[a.triCount];
    const unsigned long long nWaves = (unsigned long long)gridDim.x * (RT_TEXEL_GROUP / RT_WAVE);
    const uint32_t lane = threadIdx.x & (RT_WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / RT_WAVE);
    for (unsigned long long item = (unsigned long long)blockIdx.x * (RT_TEXEL_GROUP / RT_WAVE) + wave; item < total; item += nWaves) {
        // the last triangle whose offset is <= item (triangles without items share their successor's offset)
        uint32_t lo = 0, hi = a.triCount;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (a.offsets[mid] <= item) lo = mid;
            else hi = mid;
        }
        const uint32_t tri = a.triFirst + lo;
        const uint32_t k = (uint32_t)(item - a.offsets[lo]);
        float uv[6];
        texel_uv(sc, tri, uv);
        rt_texel_tri t;
        rt_texel_box box;
        if (!rt_texel_setup(uv, a.width, a.height, &t) || !rt_texel_bounds(&t, a.width, a.height, &box)) continue;   // (never: it has items)
        uint32_t bx, by;
        rt_texel_box_block(&box, k, &bx, &by);
        if (rt_texel_block_outside(&t, bx, by)) continue;
        const uint32_t x = bx + (lane & 7u), y = by + (lane >> 3);
        const bool inMap = x < a.width && y < a.height;
        const bool covered = inMap && rt_texel_covers(&t, x, y, nullptr, nullptr);
        if (!__ballot(covered)) continue;
        if (covered) {
            const size_t i = (size_t)y * a.width + x;
            if (atomicMin(&a.owner[i], tri) != RT_TEXEL_EMPTY) a.overlapped[i] = 1;
        }
    }
}

__global__ __launch_bounds__(RT_TEXEL_RESOLVE) void k_texel_resolve(DevScene sc, TexelArgs a) {
    const unsigned long long n = (unsigned long long)a.width * a.height;
    const float4 f0 = sc.objFwd[3 * (size_t)a.object], f1 = sc.objFwd[3 * (size_t)a.object + 1], f2 = sc.objFwd[3 * (size_t)a.object + 2];
    rt_rows fwd;
    fwd.r[0][0] = f0.x; fwd.r[0][1] = f0.y; fwd.r[0][2] = f0.z; fwd.r[0][3] = f0.w;
    fwd.r[1][0] = f1.x; fwd.r[1][1] = f1.y; fwd.r[1][2] = f1.z; fwd.r[1][3] = f1.w;
    fwd.r[2][0] = f2.x; fwd.r[2][1] = f2.y; fwd.r[2][2] = f2.z; fwd.r[2][3] = f2.w;
    const bool identity = (sc.objMeta[a.object].w & RT_OBJ_FWD_IDENTITY) != 0u;
    uint32_t nCovered = 0, nOverlapped = 0, nDegenerate = 0;   // of the wave's texels so far (the same on every lane)
    for (uint32_t k = 0; k < RT_TEXEL_RESOLVE_RUNS; k++) {
        const unsigned long long i = ((unsigned long long)blockIdx.x * RT_TEXEL_RESOLVE_RUNS + k) * RT_TEXEL_RESOLVE + threadIdx.x;
        bool isCovered = false, isOverlapped = false, isDegenerate = false;
        if (i < n) {
            float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
            const uint32_t tri = a.owner[i];
            if (tri != RT_TEXEL_EMPTY) {
                const uint32_t x = (uint32_t)(i % a.width), y = (uint32_t)(i / a.width);
                float uv[6];
                texel_uv(sc, tri, uv);
                rt_texel_tri t;
                int64_t e1 = 0, e2 = 0;
                (void)rt_texel_setup(uv, a.width, a.height, &t);
                (void)rt_texel_covers(&t, x, y, &e1, &e2);
                const float4* tp = sc.triPos + 3 * (size_t)tri;
                const float4* tn = sc.triNrm + 3 * (size_t)tri;
                rt_texel_record r;
                if (rt_texel_make_record(e1, e2, t.area, f4xyz(tp[0]), f4xyz(tp[1]), f4xyz(tp[2]), f4xyz(tn[0]), f4xyz(tn[1]), f4xyz(tn[2]), &fwd, identity, &r)) {
                    isCovered = true;
                    isOverlapped = a.overlapped[i] != 0;
                    r0 = mk4u(r.point, isOverlapped ? 3u : 1u);
                    r1 = mk4u(r.normal, tri);
                    r2 = make_float4(r.u, r.v, 0.f, 0.f);
                } else {
                    isDegenerate = true;
                }
            }
            float4* const o = a.out + 3 * (size_t)i;
            o[0] = r0; o[1] = r1; o[2] = r2;
        }
        nCovered += (uint32_t)__popcll(__ballot(isCovered));
        nOverlapped += (uint32_t)__popcll(__ballot(isOverlapped));
        nDegenerate += (uint32_t)__popcll(__ballot(isDegenerate));
    }
    // the group is one wave: one atomic per group and counter
    if (threadIdx.x == 0) {
        if (nCovered) atomicAdd(&a.stats[0], nCovered);
        if (nOverlapped) atomicAdd(&a.stats[1], nOverlapped);
        if (nDegenerate) atomicAdd(&a.stats[3], nDegenerate);
    }
}

// ---------------------------------------------------------------- compaction, scatter, dilation
struct TexelCompactArgs {
    uint32_t nTexels;
    const float4* texels;
    const uint32_t* sums;   // the scanned block sums of the covered flags: how many covered texels precede block g
    float* points;
    float* normals;
    uint32_t* index;
    uint32_t* countOut;
};
__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_texel_compact(TexelCompactArgs a) {
    const uint32_t i = blockIdx.x * RT_TEXEL_GROUP + threadIdx.x;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (i < a.nTexels) { r0 = a.texels[3 * (size_t)i]; r1 = a.texels[3 * (size_t)i + 1]; }
    const uint32_t flag = __float_as_uint(r0.w) != 0u ? 1u : 0u;
    uint32_t total;
    const uint32_t j = a.sums[blockIdx.x] + scan_group_exclusive<uint32_t>(flag, &total);
    if (flag) {
        float* const p = a.points + 3 * (size_t)j;
        float* const q = a.normals + 3 * (size_t)j;
        p[0] = r0.x; p[1] = r0.y; p[2] = r0.z;
        q[0] = r1.x; q[1] = r1.y; q[2] = r1.z;
        a.index[j] = i;
    }
    if (i == a.nTexels - 1u) a.countOut[0] = j + flag;
}

__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_texel_scatter(uint32_t nCovered, const uint32_t* index, const float4* values, float4* rgba, uint8_t* fill, uint32_t nTexels) {
    const uint32_t j = blockIdx.x * RT_TEXEL_GROUP + threadIdx.x;
    if (j >= nCovered) return;
    const uint32_t i = index[j];
    if (i >= nTexels) return;   // (an index array that is not a compaction's: nothing is written outside the map)
    rgba[i] = values[j];
    fill[i] = 1;
}

__global__ __launch_bounds__(RT_TEXEL_GROUP) void k_texel_dilate(uint32_t width, uint32_t height, uint32_t pass, const float* rgba, const uint8_t* fill, float4* rgbaOut, uint8_t* fillOut) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RT_TEXEL_GROUP + threadIdx.x;
    if (i >= (unsigned long long)width * height) return;
    float o[4];
    uint8_t f;
    rt_dilate_texel(width, height, (uint32_t)(i % width), (uint32_t)(i / width), pass, rgba, fill, o, &f);
    rgbaOut[i] = make_float4(o[0], o[1], o[2], o[3]);
    fillOut[i] = f;
}
