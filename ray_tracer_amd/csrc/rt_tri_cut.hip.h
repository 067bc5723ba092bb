// rt_tri_cut.hip.h — k_tris_cut, the kernel of the cut queries (rt_query_cuts; DESIGN.md, "Triangle cuts").
//
// k_tris_overlap's shape and its very descent (rt_tri_overlap.hip.h: tris_objects, tris_descend, tris_node_in, the lane's
// prepared query, the sibling-only stack lane-interleaved in LDS behind the `sp < STACK` guard, the key lists of RT_BOX_WORDS
// words in LDS beside the 24-entry stack or, GLIST, in the ctx buffer of the box queries): one lane per query triangle, wave64,
// 256-thread groups. Only what a leaf does differs (CutExists): a triangle is a member when the pair has a cut
// (include/rt_tri_cut.h, the very functions the exhaustive host loop compiles). A cut member passed rt_tri_triangle_prepared, the gate of the rule, so what
// the descent may discard for the triangle query, (a) by the query's box and (b) by its plane, it may discard here, and the
// nodes and triangles it looks at are that query's, one for one.
// The lists hold keys only: a cut is a function of the pair, so after the search the lane computes the at most k kept cuts again
// from the kept keys and writes each 48-byte record with three 16-byte stores. No end point is carried through the descent.
#pragma once

#include "rt_tri_overlap.hip.h"
#include "rt_tri_cut.h"

struct CutsArgs {
    const float* corners;     // n x 9, packed: p, q, r
    uint32_t n, k, plane;     // plane: pruning (b) on
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    uint4* out;               // n x k RtCut records of three uint4 (NULL with k == 0)
    uint32_t* counts;         // n
    uint32_t* lists;          // GLIST: RT_BOXES_MAX_K x RT_BOX_WORDS x 64 words per wave of the grid
    DevCounters* counters;
};

// The world corners of triangle j
__device__ __forceinline__ void cut_corners(const DevScene& sc, uint32_t j, bool placed, float4 f0, float4 f1, float4 f2, rt_vec3& a, rt_vec3& b, rt_vec3& c) {
    a = f4xyz(sc.triPos[3 * (size_t)j]); b = f4xyz(sc.triPos[3 * (size_t)j + 1]); c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
    if (placed) { a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c); }
}

// What a leaf does here, in two passes over at most 32 triangles at a time: the gate (rt_tri_triangle_prepared) over all of them
// into a bit mask, then steps 2 to 5 of the rule (rt_tri_cut_segment) over the set bits. One pass would be the same answer, but
// the gate leaves through nine nested branches and everything behind it would sit inside them, each holding a saved exec mask:
// the scalar file overflows (tests/test_cuts_budget.py). A loop of its own starts from none.
struct CutExists {
    static __device__ __forceinline__ void leaf(const DevScene& sc, TriLane& tl, uint32_t obj, uint32_t first, uint32_t count, bool placed, float4 f0, float4 f1, float4 f2) {
        for (uint32_t base = first; base < first + count; base += 32u) {
            const uint32_t some = min(32u, first + count - base);
            uint32_t passed = 0u;
            for (uint32_t i = 0; i < some; i++) {
                rt_vec3 a, b, c;
                cut_corners(sc, base + i, placed, f0, f1, f2, a, b, c);
                passed |= rt_tri_triangle_prepared(&tl.t, a, b, c) ? 1u << i : 0u;
            }
            while (passed) {
                const uint32_t j = base + (uint32_t)__builtin_ctz(passed);
                passed &= passed - 1u;
                rt_vec3 a, b, c;
                RtCutSeg seg;
                cut_corners(sc, j, placed, f0, f1, f2, a, b, c);
                if (!rt_tri_cut_segment(&tl.t, a, b, c, &seg)) continue;
                tl.count++;
                tl.have = rt_box_insert(tl.list, RT_WAVE, tl.k, tl.have, rt_box_triangle_word(obj), j);
            }
        }
    }
};

template <int STACK, bool GLIST>
__global__ __launch_bounds__(RT_BLOCK) void k_tris_cut(DevScene sc, CutsArgs ca) {
    constexpr uint32_t LIST = RT_BOXES_MAX_K * RT_BOX_WORDS * RT_WAVE;   // words of a wave's lists
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * RT_WAVE];
    __shared__ uint32_t s_list[GLIST ? 1 : (RT_BLOCK / RT_WAVE) * LIST];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x / RT_WAVE, lane = threadIdx.x & (RT_WAVE - 1);
    const bool mine = gid < ca.n;
    TriLane tl;
    tl.stack = s_stack + wave * STACK * RT_WAVE + lane;
    tl.list = GLIST ? ca.lists + ((size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * LIST + lane : s_list + wave * LIST + lane;
    tl.k = ca.k; tl.have = 0; tl.count = 0; tl.nBox = 0; tl.nTri = 0; tl.plane = ca.plane != 0u;
    // (a lane past the batch takes a NaN corner: not valid, not searched)
    const float nan = __uint_as_float(0x7fc00000u);
    rt_vec3 p = rt_v3(nan, nan, nan), q = p, r = p;
    if (mine) {
        const float* const pc = ca.corners + (size_t)gid * 9;
        p = rt_v3(pc[0], pc[1], pc[2]); q = rt_v3(pc[3], pc[4], pc[5]); r = rt_v3(pc[6], pc[7], pc[8]);
    }
    const bool searched = rt_tri_valid(p, q, r);
    if (searched) {
        tl.t = rt_tri_prepare(p, q, r);
        tris_objects<STACK, CutExists>(sc, tl, ca.objNear);
    }
    if (mine) {
        ca.counts[gid] = tl.count;
        // the kept keys' cuts, computed again (have <= k, and 0 for a lane that did not search)
        for (uint32_t e = 0; e < tl.k; e++) {
            const uint32_t* const le = tl.list + (size_t)e * RT_BOX_WORDS * RT_WAVE;
            // (no record struct here: its arrays would live in scratch)
            RtCutSeg seg;
            bool cut = false;
            uint32_t obj = 0u, j = 0u;
            if (e < tl.have) {
                obj = le[0]; j = le[RT_WAVE];
                rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)j]), b = f4xyz(sc.triPos[3 * (size_t)j + 1]), c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
                if ((sc.objMeta[obj].w & RT_OBJ_FWD_IDENTITY) == 0u) {
                    const float4* const fwd = rt_global(sc.objFwd) + 3 * (size_t)obj;
                    const float4 f0 = fwd[0], f1 = fwd[1], f2 = fwd[2];
                    a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c);
                }
                cut = rt_tri_cut_segment(&tl.t, a, b, c, &seg);   // (a kept key passed the gate)
            }
            // rt_cut_record's words, or rt_cut_no_member's
            uint4* const at = ca.out + ((size_t)gid * tl.k + e) * 3;
            at[0] = cut ? make_uint4(__float_as_uint(seg.a.x), __float_as_uint(seg.a.y), __float_as_uint(seg.a.z), seg.featA) : make_uint4(0u, 0u, 0u, 0u);
            at[1] = cut ? make_uint4(__float_as_uint(seg.b.x), __float_as_uint(seg.b.y), __float_as_uint(seg.b.z), seg.featB) : make_uint4(0u, 0u, 0u, 0u);
            at[2] = cut ? make_uint4(1u, obj, j, 0u) : make_uint4(0u, 0u, 0u, 0u);
        }
    }

    // one atomic per wave and counter
    const unsigned long long wb = wave_sum_u64(tl.nBox), wt = wave_sum_u64(tl.nTri);
    const uint32_t ws = wave_sum_u32(searched ? 1u : 0u), wf = wave_sum_u32(tl.count ? 1u : 0u);
    if (lane_id() == 0 && ws) {
        atomicAdd(&ca.counters->boxTests, wb);
        atomicAdd(&ca.counters->triTests, wt);
        atomicAdd(&ca.counters->raysTraced, (unsigned long long)ws);
        atomicAdd(&ca.counters->raysHit, (unsigned long long)wf);
    }
}
