// rt_refit.hip.h — the kernels of rt_update_points (mesh_refit.h states the rule and the plan they run; DESIGN.md, "Deforming
// meshes"). They rewrite the tables of one mesh in place: triPos / triNrm / triUV from the points, the boxes of `nodes` bottom-up,
// the interleaved pairs of `nodesPk`. Plain C++ on wave64; every launch is ordered by the stream, no kernel waits for another block.
#pragma once

#include "rt_kernels.hip.h"
#include "mesh_refit.h"

// `p < lo ? p : lo` and `hi < p ? p : hi`: the builder's comparisons. Of two equal values (zeros of either sign) the first stays.
__device__ __forceinline__ float refit_lo(float lo, float p) { return p < lo ? p : lo; }
__device__ __forceinline__ float refit_hi(float hi, float p) { return hi < p ? p : hi; }

struct RefitBox { float lo[3], hi[3]; };
__device__ __forceinline__ RefitBox refit_empty() { return RefitBox{{RT_REFIT_LO, RT_REFIT_LO, RT_REFIT_LO}, {RT_REFIT_HI, RT_REFIT_HI, RT_REFIT_HI}}; }
__device__ __forceinline__ void refit_grow(RefitBox& b, const float4 p) {
    b.lo[0] = refit_lo(b.lo[0], p.x); b.lo[1] = refit_lo(b.lo[1], p.y); b.lo[2] = refit_lo(b.lo[2], p.z);
    b.hi[0] = refit_hi(b.hi[0], p.x); b.hi[1] = refit_hi(b.hi[1], p.y); b.hi[2] = refit_hi(b.hi[2], p.z);
}
// a node's box with its two .w words kept
__device__ __forceinline__ void refit_store(float4* nodes, uint32_t node, const RefitBox& b) {
    float4* n = nodes + 2 * (size_t)node;
    n[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], n[0].w);
    n[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], n[1].w);
}

// Gather: one thread per triangle of the mesh, [triFirst, triFirst + triCount). triIdx: {v0, v1, v2, frontOnly} per triangle;
// points: 2 x float4 per TrianglePoint {position.xyz, u} {normal.xyz, v}. Writes what layout_meshes writes for the triangle.
__global__ void k_refit_gather(const uint4* __restrict__ triIdx, const float4* __restrict__ points, uint32_t triFirst, uint32_t triCount,
                               float4* __restrict__ triPos, float4* __restrict__ triNrm, float4* __restrict__ triUV) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= triCount) return;
    const size_t t = (size_t)triFirst + k;
    const uint4 tr = triIdx[t];
    const float4 p0 = points[2 * (size_t)tr.x], n0 = points[2 * (size_t)tr.x + 1];
    const float4 p1 = points[2 * (size_t)tr.y], n1 = points[2 * (size_t)tr.y + 1];
    const float4 p2 = points[2 * (size_t)tr.z], n2 = points[2 * (size_t)tr.z + 1];
    triPos[3 * t] = make_float4(p0.x, p0.y, p0.z, __uint_as_float(tr.w ? 1u : 0u));
    triPos[3 * t + 1] = make_float4(p1.x, p1.y, p1.z, 0.f);
    triPos[3 * t + 2] = make_float4(p2.x, p2.y, p2.z, 0.f);
    triNrm[3 * t] = make_float4(n0.x, n0.y, n0.z, 0.f);
    triNrm[3 * t + 1] = make_float4(n1.x, n1.y, n1.z, 0.f);
    triNrm[3 * t + 2] = make_float4(n2.x, n2.y, n2.z, 0.f);
    triUV[2 * t] = make_float4(p0.w, n0.w, p1.w, n1.w);
    triUV[2 * t + 1] = make_float4(p2.w, n2.w, 0.f, 0.f);
}

// Leaves whose W0 holds {count <= 7, first triangle}: one thread per leaf, the triangles in order
__global__ void k_refit_leaves_inline(const uint32_t* __restrict__ leaves, uint32_t n, const float4* __restrict__ triPos, float4* nodes) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t node = leaves[k];
    const uint32_t ref = __float_as_uint(nodes[2 * (size_t)node].w);
    const uint32_t cnt = (ref >> RT_LEAF_CNT_SHIFT) & 7u;
    const size_t first = ref & RT_LEAF_IDX_MASK;
    RefitBox b = refit_empty();
    for (uint32_t c = 0; c < 3 * cnt; c++) refit_grow(b, triPos[3 * first + c]);
    refit_store(nodes, node, b);
}

// The other leaves (first triangle in leafFirst, count in nodes[2 i + 1].w; they can hold hundreds of triangles): one wave per
// leaf. Lane l folds the l-th of 64 consecutive runs of the leaf's corners in order; the runs are then folded in lane order (at
// every step the lower lane holds the earlier run and keeps its value against an equal one), which gives what the serial loop
// over all corners gives, the sign of a zero included.
__global__ void __launch_bounds__(256) k_refit_leaves_big(const uint32_t* __restrict__ leaves, uint32_t n, const uint32_t* __restrict__ leafFirst,
                                                          const float4* __restrict__ triPos, float4* nodes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // (uniform over the wave)
    if (k >= n) return;
    const uint32_t node = leaves[k];
    const uint32_t corners = 3u * __float_as_uint(nodes[2 * (size_t)node + 1].w);
    const size_t first = 3 * (size_t)leafFirst[node];
    const uint32_t per = (corners + 63u) >> 6;
    const uint32_t begin = min(lane * per, corners), end = min(begin + per, corners);
    RefitBox b = refit_empty();
    for (uint32_t c = begin; c < end; c++) refit_grow(b, triPos[first + c]);
    for (int off = 1; off < 64; off <<= 1)
        for (int a = 0; a < 3; a++) {
            const float lo = __shfl_down(b.lo[a], off, 64), hi = __shfl_down(b.hi[a], off, 64);
            if (lane + off < 64u) { b.lo[a] = refit_lo(b.lo[a], lo); b.hi[a] = refit_hi(b.hi[a], hi); }
        }
    if (lane == 0) refit_store(nodes, node, b);
}

// an interior node from its child pair (64 bytes at nodes[2 * W0]): the left child's box grown by the right child's
__device__ __forceinline__ void refit_interior(float4* nodes, uint32_t node) {
    const uint32_t child = __float_as_uint(nodes[2 * (size_t)node].w);
    const float4* c = nodes + 2 * (size_t)child;
    const float4 llo = c[0], lhi = c[1], rlo = c[2], rhi = c[3];
    RefitBox b{{llo.x, llo.y, llo.z}, {lhi.x, lhi.y, lhi.z}};
    b.lo[0] = refit_lo(b.lo[0], rlo.x); b.lo[1] = refit_lo(b.lo[1], rlo.y); b.lo[2] = refit_lo(b.lo[2], rlo.z);
    b.hi[0] = refit_hi(b.hi[0], rhi.x); b.hi[1] = refit_hi(b.hi[1], rhi.y); b.hi[2] = refit_hi(b.hi[2], rhi.z);
    refit_store(nodes, node, b);
}

// One level of interior nodes: one thread per node. The levels below it were written by earlier launches on the stream.
__global__ void k_refit_level(const uint32_t* __restrict__ interior, uint32_t n, float4* nodes) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    refit_interior(nodes, interior[k]);
}

// The narrow levels towards the root in one block: levelOff[0 .. nLevels] are the levels' starts in `interior` (deepest of them
// first) and the end. A barrier between levels: every thread of the block has stored its nodes before any reads them as children.
__global__ void __launch_bounds__(256) k_refit_top(const uint32_t* __restrict__ interior, const uint32_t* __restrict__ levelOff, uint32_t nLevels, float4* nodes) {
    for (uint32_t l = 0; l < nLevels; l++) {
        const uint32_t begin = levelOff[l], end = levelOff[l + 1];
        for (uint32_t k = begin + threadIdx.x; k < end; k += blockDim.x) refit_interior(nodes, interior[k]);
        __threadfence_block();
        __syncthreads();
    }
}

// Pack: nodesPk of every child pair of the mesh and of the pair the root sits in, from `nodes`, as layout_meshes interleaves them.
// Thread k < nInterior takes the child pair of interior[k]; thread nInterior takes the pair of the root (a root on an odd slot
// shares it with its predecessor).
__global__ void k_refit_pack(const uint32_t* __restrict__ interior, uint32_t nInterior, uint32_t root, uint32_t nodeCount, const float4* __restrict__ nodes,
                             float4* __restrict__ nodesPk) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nInterior) return;
    const size_t p = k < nInterior ? __float_as_uint(nodes[2 * (size_t)interior[k]].w) : (root & ~1u);
    if (p + 1 >= nodeCount) return;
    const float4 lo1 = nodes[2 * p], hi1 = nodes[2 * p + 1], lo2 = nodes[2 * p + 2], hi2 = nodes[2 * p + 3];
    nodesPk[2 * p] = make_float4(lo1.x, lo1.y, hi1.x, hi1.y);
    nodesPk[2 * p + 1] = make_float4(lo2.x, lo2.y, hi2.x, hi2.y);
    nodesPk[2 * p + 2] = make_float4(lo1.z, hi1.z, lo2.z, hi2.z);
    nodesPk[2 * p + 3] = make_float4(lo1.w, lo2.w, 0.f, 0.f);
}
