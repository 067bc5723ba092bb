// rt_tri_overlap.hip.h — k_tris_overlap, the kernel of the triangle queries (rt_query_triangles; DESIGN.md, "Triangle queries").
//
// k_boxes_overlap's shape (rt_box_overlap.hip.h): one lane per query triangle, wave64, 256-thread groups, no path state, the
// batch read from the caller's packed array of nine floats a triangle; a sibling-only stack lane-interleaved in LDS (entry e of
// lane l at word e * 64 + l: conflict-free); the list of 8 entries of 2 words lane-interleaved the same way, in LDS beside a
// 24-entry stack (24 KB + 16 KB: three groups a CU) and, GLIST, in a ctx buffer per wave where the 64-entry stack takes the whole
// 64 KB; the records written by the search itself, one 16-byte store each; one atomic per wave and counter. The rule is
// include/rt_tri_overlap.h, the very functions the exhaustive host loop compiles, so a pair's verdict is the same on both sides,
// and membership does not depend on the order of the visits.
// The lane prepares its query once (rt_tri_prepare: the box, its centre, the relative corners, the edges, nQ, nQ x eQi and the
// query's intervals on those four axes: 56 numbers in vector registers) and carries it through the whole search.
// The descent discards a subtree (a) when its box lies apart from the query's box, k_boxes_overlap's very test with the query's
// box for the box, and (b), `plane`, when its box lies strictly on one side of the query's plane by more than the counted pad
// (rt_tri_plane_apart): for an identity object the node's own numbers, for a placed one the padded world box that (a) tests.
// A node counts once in boxTests, whether (a) alone or (a) and (b) looked at it, so the figure compares with k_boxes_overlap's
// over the queries' own boxes: the same descent, which can only have discarded more. (b) runs only on what (a) kept.
#pragma once

#include "rt_kernels.hip.h"
#include "rt_tri_overlap.h"

struct TrisArgs {
    const float* corners;     // n x 9, packed: p, q, r
    uint32_t n, k, plane;     // plane: pruning (b) on
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    uint4* out;               // n x k RtOverlap records (NULL with k == 0)
    uint32_t* counts;         // n
    uint32_t* lists;          // GLIST: RT_BOXES_MAX_K x RT_BOX_WORDS x 64 words per wave of the grid
    DevCounters* counters;
};

// What a lane carries through a search: the prepared query, its list and its tallies
struct TriLane {
    RtTriQuery t;
    uint32_t* stack;   // entry e at stack[e * RT_WAVE]
    uint32_t* list;    // entry e's word w at list[(e * RT_BOX_WORDS + w) * RT_WAVE]
    uint32_t k, have, count, nBox, nTri;
    bool plane;
};

// One node box of the descent: kept unless (a) or (b) discards it. Counts the node.
__device__ __forceinline__ bool tris_node_in(TriLane& tl, bool placed, float4 f0, float4 f1, float4 f2, float pad, rt_vec3 blo, rt_vec3 bhi) {
    tl.nBox++;
    if (placed) {
        const rt_vec3 ft = rt_v3(f0.w, f1.w, f2.w);
        if (rt_box_placed_apart(tl.t.lo, tl.t.hi, f4xyz(f0), f4xyz(f1), f4xyz(f2), ft, blo, bhi, pad)) return false;
        if (!tl.plane) return true;
        rt_tri_world_box(f4xyz(f0), f4xyz(f1), f4xyz(f2), ft, blo, bhi, pad, &blo, &bhi);
    } else {
        if (rt_box_apart(tl.t.lo, tl.t.hi, blo, bhi)) return false;
        if (!tl.plane) return true;
    }
    return !rt_tri_plane_apart(&tl.t, blo, bhi);
}

// The descent of one object's tree. placed: the object has a forward matrix (rows f0..f2) and the pad of its scale; else the
// node boxes and the corners are used as they are. Pair: what a leaf does with its triangles (TriTouch here; rt_tri_cut.hip.h's
// CutExists runs the same descent: a cut member passed rt_tri_triangle_prepared).
struct TriTouch {
    // the triangles [first, first + count) of a leaf of object obj against the lane's query
    static __device__ __forceinline__ void leaf(const DevScene& sc, TriLane& tl, uint32_t obj, uint32_t first, uint32_t count, bool placed, float4 f0, float4 f1, float4 f2) {
        for (uint32_t j = first; j < first + count; j++) {
            rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)j]), b = f4xyz(sc.triPos[3 * (size_t)j + 1]), c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
            if (placed) { a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c); }
            if (!rt_tri_triangle_prepared(&tl.t, a, b, c)) continue;
            tl.count++;
            tl.have = rt_box_insert(tl.list, RT_WAVE, tl.k, tl.have, rt_box_triangle_word(obj), j);
        }
    }
};
template <int STACK, typename Pair = TriTouch>
__device__ __forceinline__ void tris_descend(const DevScene& sc, TriLane& tl, uint32_t obj, uint32_t root, uint32_t rootCnt, bool placed, float4 f0, float4 f1, float4 f2, float pad) {
    uint32_t* const stack = tl.stack;
    uint32_t sp = 0, curIdx = root, curCnt = rootCnt;
    if (curCnt) leaf_from_ref(sc, root, curIdx, curCnt);
    bool have_node = true;
    for (;;) {
        if (!have_node) {
            if (sp == 0) break;
            const uint32_t ref = stack[(--sp) * RT_WAVE];
            if (ref & RT_LEAF_BIT) leaf_from_ref(sc, ref, curIdx, curCnt);
            else { curIdx = ref; curCnt = 0; }
            have_node = true;
        }
        if (curCnt != 0) {
            tl.nTri += curCnt;
            Pair::leaf(sc, tl, obj, curIdx, curCnt, placed, f0, f1, f2);
            have_node = false;
        } else {
            const float4* pr = sc.nodes + 2 * (size_t)curIdx;
            const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
            const bool in1 = tris_node_in(tl, placed, f0, f1, f2, pad, f4xyz(lo1), f4xyz(hi1));
            const bool in2 = tris_node_in(tl, placed, f0, f1, f2, pad, f4xyz(lo2), f4xyz(hi2));
            // (sp < STACK always: one sibling per level, and tris_stack chose STACK >= the deepest leaf's depth; the test keeps
            // a table that broke that promise from writing outside the stack)
            if (in1 && in2 && sp < (uint32_t)STACK) { stack[sp * RT_WAVE] = __float_as_uint(lo2.w); sp++; }
            if (in1 || in2) {
                const uint32_t w = __float_as_uint(in1 ? lo1.w : lo2.w), cnt = __float_as_uint(in1 ? hi1.w : hi2.w);
                curIdx = w; curCnt = cnt;
                if (cnt) leaf_from_ref(sc, w, curIdx, curCnt);
            } else have_node = false;
        }
    }
}

// Every object of the scene for a prepared query: its box by (a) and (b), then its tree
template <int STACK, typename Pair>
__device__ __forceinline__ void tris_objects(const DevScene& sc, TriLane& tl, const float4* objNear) {
    for (uint32_t obj = 0; obj < sc.objectCount; obj++) {
        // The object's record and, below, its rows through a per-lane index, as k_boxes_overlap reads the rows: every lane
        // reads the same numbers (threadIdx.y is 0 in this one-dimensional launch), but as vector loads into vector
        // registers; as scalars they live through the whole descent and the scalar file overflows
        // (tests/test_triangles_budget.py)
        const float4* const near = rt_global(objNear) + 3 * (size_t)(obj + threadIdx.y);
        const float4 n0 = near[0], n1 = near[1];
        const uint4 meta = sc.objMeta[obj];
        tl.nBox++;
        const bool placed = (meta.w & RT_OBJ_FWD_IDENTITY) == 0u;
        const float pad = rt_box_pad(near[2].x);
        if (placed ? rt_box_object_apart(tl.t.lo, tl.t.hi, f4xyz(n0), f4xyz(n1), pad) : rt_box_apart(tl.t.lo, tl.t.hi, f4xyz(n0), f4xyz(n1))) continue;
        if (tl.plane) {
            // the object's world box, grown by the pad rt_box_object_apart grows a placed one by
            const float g = placed ? pad : 0.f;
            if (rt_tri_plane_apart(&tl.t, rt_v3(n0.x - g, n0.y - g, n0.z - g), rt_v3(n1.x + g, n1.y + g, n1.z + g))) continue;
        }
        const float4* const fwd = rt_global(sc.objFwd) + 3 * (size_t)(obj + threadIdx.y);
        float4 f0 = make_float4(1.f, 0.f, 0.f, 0.f), f1 = make_float4(0.f, 1.f, 0.f, 0.f), f2 = make_float4(0.f, 0.f, 1.f, 0.f);
        if (placed) { f0 = fwd[0]; f1 = fwd[1]; f2 = fwd[2]; }
        tris_descend<STACK, Pair>(sc, tl, obj, meta.x, meta.y, placed, f0, f1, f2, pad);
    }
}

template <int STACK, bool GLIST>
__global__ __launch_bounds__(RT_BLOCK) void k_tris_overlap(DevScene sc, TrisArgs ta) {
    constexpr uint32_t LIST = RT_BOXES_MAX_K * RT_BOX_WORDS * RT_WAVE;   // words of a wave's lists
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * RT_WAVE];
    __shared__ uint32_t s_list[GLIST ? 1 : (RT_BLOCK / RT_WAVE) * LIST];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x / RT_WAVE, lane = threadIdx.x & (RT_WAVE - 1);
    const bool mine = gid < ta.n;
    TriLane tl;
    tl.stack = s_stack + wave * STACK * RT_WAVE + lane;
    tl.list = GLIST ? ta.lists + ((size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * LIST + lane : s_list + wave * LIST + lane;
    tl.k = ta.k; tl.have = 0; tl.count = 0; tl.nBox = 0; tl.nTri = 0; tl.plane = ta.plane != 0u;
    // (a lane past the batch takes a NaN corner: not valid, not searched)
    const float nan = __uint_as_float(0x7fc00000u);
    rt_vec3 p = rt_v3(nan, nan, nan), q = p, r = p;
    if (mine) {
        const float* const pc = ta.corners + (size_t)gid * 9;
        p = rt_v3(pc[0], pc[1], pc[2]); q = rt_v3(pc[3], pc[4], pc[5]); r = rt_v3(pc[6], pc[7], pc[8]);
    }
    const bool searched = rt_tri_valid(p, q, r);
    if (searched) {
        for (uint32_t i = 0; i < sc.sphereCount; i++) {
            const float4 s = sc.spheres[i];
            if (!rt_sphere_is_surface(s.w)) continue;
            if (!rt_tri_sphere(p, q, r, f4xyz(s), s.w)) continue;
            tl.count++;
            tl.have = rt_box_insert(tl.list, RT_WAVE, tl.k, tl.have, rt_box_sphere_word(i), 0u);
        }
        tl.t = rt_tri_prepare(p, q, r);
        tris_objects<STACK, TriTouch>(sc, tl, ta.objNear);
    }
    if (mine) {
        ta.counts[gid] = tl.count;
        for (uint32_t e = 0; e < tl.k; e++) {
            const uint32_t* const le = tl.list + (size_t)e * RT_BOX_WORDS * RT_WAVE;
            RtOverlap rec = rt_box_no_member();
            if (e < tl.have) rec = rt_box_record(le[0], le[RT_WAVE]);
            ta.out[(size_t)gid * tl.k + e] = make_uint4(rec.found, rec.isSphere, rec.objectIndex, rec.triIndex);
        }
    }

    // one atomic per wave and counter
    const unsigned long long wb = wave_sum_u64(tl.nBox), wt = wave_sum_u64(tl.nTri);
    const uint32_t ws = wave_sum_u32(searched ? 1u : 0u), wf = wave_sum_u32(tl.count ? 1u : 0u);
    if (lane_id() == 0 && ws) {
        atomicAdd(&ta.counters->boxTests, wb);
        atomicAdd(&ta.counters->triTests, wt);
        atomicAdd(&ta.counters->raysTraced, (unsigned long long)ws);
        atomicAdd(&ta.counters->raysHit, (unsigned long long)wf);
    }
}
