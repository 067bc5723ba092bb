// rt_box_overlap.hip.h — k_boxes_overlap, the kernel of the box queries (rt_query_boxes; DESIGN.md, "Box queries").
//
// One lane per box, wave64, 256-thread groups, no path state, boxes read from the caller's packed arrays: the shape of
// k_points_within. The rule is include/rt_box_overlap.h, the very functions the exhaustive host loop compiles, so a pair's verdict
// is the same on both sides; and membership does not depend on the order of the visits: whatever the descent discards holds no
// member (a member triangle passed the rule's first stage, so the box of its world corners meets the query box under exact
// comparisons; DESIGN.md has the derivation), and what is left is the set the host loop finds. Per valid box: the sphere loop;
// then the objects in index order, each skipped when its world box (layout_nearest's) lies apart from the query box, else
// entered: the object's tree is descended from the 64-byte child pairs with an explicit stack of siblings, a child entered unless
// its box lies apart: rt_box_apart on the node's own numbers for an identity object, and for a placed one rt_box_placed_apart,
// the node's box taken to world space as M centre +- |M| extent and padded by rt_box_pad(mag). The query box never moves, so a
// popped entry needs no second test and the stack holds references only. At a leaf the corners go forward to world space, and
// every triangle rt_box_triangle keeps bumps the lane's count and goes through rt_box_insert into the lane's sorted list of at
// most k entries.
// The stack is lane-interleaved in LDS as trace_wave's (entry e of lane l at word e * 64 + l: conflict-free) and holds siblings
// only, one per level at most, so STACK >= the deepest leaf's depth is enough (box_queries.h: boxes_stack). The list, 8 entries of
// 2 words, is lane-interleaved the same way: in LDS beside a 24-entry stack (24 KB + 16 KB), and, GLIST, in a ctx buffer per wave
// where the 64-entry stack takes the whole 64 KB: what k_points_within does. k == 0 keeps no list.
// The search writes the records itself, one 16-byte store each: a record is its list entry re-spelt (rt_box_record: no geometry,
// no arithmetic), so a resolve pass would only read two words and write four.
#pragma once

#include "rt_kernels.hip.h"
#include "rt_box_overlap.h"

struct BoxesArgs {
    const float* lo;          // n x 3, packed
    const float* hi;          // n x 3, packed
    uint32_t n, k;
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    uint4* out;               // n x k RtOverlap records (NULL with k == 0)
    uint32_t* counts;         // n
    uint32_t* lists;          // GLIST: RT_BOXES_MAX_K x RT_BOX_WORDS x 64 words per wave of the grid
    DevCounters* counters;
};

// What a lane carries through a search: the box, its list and its tallies
struct BoxLane {
    rt_vec3 lo, hi;
    uint32_t* stack;   // entry e at stack[e * RT_WAVE]
    uint32_t* list;    // entry e's word w at list[(e * RT_BOX_WORDS + w) * RT_WAVE]
    uint32_t k, have, count, nBox, nTri;
};

// The descent of one object's tree. placed: the object has a forward matrix (rows f0..f2) and the pad of its scale; else the
// node boxes and the corners are used as they are.
template <int STACK>
__device__ __forceinline__ void boxes_descend(const DevScene& sc, BoxLane& bl, uint32_t obj, uint32_t root, uint32_t rootCnt, bool placed, float4 f0, float4 f1, float4 f2, float pad) {
    const rt_vec3 lo = bl.lo, hi = bl.hi;
    uint32_t* const stack = bl.stack;
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
            bl.nTri += curCnt;
            for (uint32_t j = curIdx; j < curIdx + curCnt; j++) {
                rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)j]), b = f4xyz(sc.triPos[3 * (size_t)j + 1]), c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
                if (placed) { a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c); }
                if (!rt_box_triangle(lo, hi, a, b, c)) continue;
                bl.count++;
                bl.have = rt_box_insert(bl.list, RT_WAVE, bl.k, bl.have, rt_box_triangle_word(obj), j);
            }
            have_node = false;
        } else {
            const float4* pr = sc.nodes + 2 * (size_t)curIdx;
            const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
            bool in1, in2;
            if (placed) {
                const rt_vec3 ft = rt_v3(f0.w, f1.w, f2.w);
                in1 = !rt_box_placed_apart(lo, hi, f4xyz(f0), f4xyz(f1), f4xyz(f2), ft, f4xyz(lo1), f4xyz(hi1), pad);
                in2 = !rt_box_placed_apart(lo, hi, f4xyz(f0), f4xyz(f1), f4xyz(f2), ft, f4xyz(lo2), f4xyz(hi2), pad);
            } else {
                in1 = !rt_box_apart(lo, hi, f4xyz(lo1), f4xyz(hi1));
                in2 = !rt_box_apart(lo, hi, f4xyz(lo2), f4xyz(hi2));
            }
            bl.nBox += 2;
            // (sp < STACK always: one sibling per level, and boxes_stack chose STACK >= the deepest leaf's depth; the test keeps
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

template <int STACK, bool GLIST>
__global__ __launch_bounds__(RT_BLOCK) void k_boxes_overlap(DevScene sc, BoxesArgs ba) {
    constexpr uint32_t LIST = RT_BOXES_MAX_K * RT_BOX_WORDS * RT_WAVE;   // words of a wave's lists
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * RT_WAVE];
    __shared__ uint32_t s_list[GLIST ? 1 : (RT_BLOCK / RT_WAVE) * LIST];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x / RT_WAVE, lane = threadIdx.x & (RT_WAVE - 1);
    const bool mine = gid < ba.n;
    BoxLane bl;
    bl.stack = s_stack + wave * STACK * RT_WAVE + lane;
    bl.list = GLIST ? ba.lists + ((size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * LIST + lane : s_list + wave * LIST + lane;
    bl.k = ba.k; bl.have = 0; bl.count = 0; bl.nBox = 0; bl.nTri = 0;
    // (a lane past the batch takes an inverted box: not valid, not searched)
    bl.lo = rt_v3(1.f, 1.f, 1.f); bl.hi = rt_v3(0.f, 0.f, 0.f);
    if (mine) {
        const size_t r = (size_t)gid * 3;
        bl.lo = rt_v3(ba.lo[r], ba.lo[r + 1], ba.lo[r + 2]); bl.hi = rt_v3(ba.hi[r], ba.hi[r + 1], ba.hi[r + 2]);
    }
    const bool searched = rt_box_valid(bl.lo, bl.hi);
    if (searched) {
        for (uint32_t i = 0; i < sc.sphereCount; i++) {
            const float4 s = sc.spheres[i];
            if (!rt_sphere_is_surface(s.w)) continue;
            if (!rt_box_sphere(bl.lo, bl.hi, f4xyz(s), s.w)) continue;
            bl.count++;
            bl.have = rt_box_insert(bl.list, RT_WAVE, bl.k, bl.have, rt_box_sphere_word(i), 0u);
        }
        for (uint32_t obj = 0; obj < sc.objectCount; obj++) {
            const float4 n0 = ba.objNear[3 * (size_t)obj], n1 = ba.objNear[3 * (size_t)obj + 1];
            const uint4 meta = sc.objMeta[obj];
            bl.nBox++;
            const bool placed = (meta.w & RT_OBJ_FWD_IDENTITY) == 0u;
            const float pad = rt_box_pad(ba.objNear[3 * (size_t)obj + 2].x);
            if (placed ? rt_box_object_apart(bl.lo, bl.hi, f4xyz(n0), f4xyz(n1), pad) : rt_box_apart(bl.lo, bl.hi, f4xyz(n0), f4xyz(n1))) continue;
            // The rows through a per-lane index: every lane reads the same three rows (threadIdx.y is 0 in this one-dimensional
            // launch), but as vector loads into vector registers, of which the kernel has plenty; as scalars the twelve numbers
            // live through the whole descent and the scalar file overflows (tests/test_boxes_budget.py)
            const float4* const fwd = rt_global(sc.objFwd) + 3 * (size_t)(obj + threadIdx.y);
            float4 f0 = make_float4(1.f, 0.f, 0.f, 0.f), f1 = make_float4(0.f, 1.f, 0.f, 0.f), f2 = make_float4(0.f, 0.f, 1.f, 0.f);
            if (placed) { f0 = fwd[0]; f1 = fwd[1]; f2 = fwd[2]; }
            boxes_descend<STACK>(sc, bl, obj, meta.x, meta.y, placed, f0, f1, f2, pad);
        }
    }
    if (mine) {
        ba.counts[gid] = bl.count;
        for (uint32_t e = 0; e < bl.k; e++) {
            const uint32_t* const le = bl.list + (size_t)e * RT_BOX_WORDS * RT_WAVE;
            RtOverlap rec = rt_box_no_member();
            if (e < bl.have) rec = rt_box_record(le[0], le[RT_WAVE]);
            ba.out[(size_t)gid * bl.k + e] = make_uint4(rec.found, rec.isSphere, rec.objectIndex, rec.triIndex);
        }
    }

    // one atomic per wave and counter
    const unsigned long long wb = wave_sum_u64(bl.nBox), wt = wave_sum_u64(bl.nTri);
    const uint32_t ws = wave_sum_u32(searched ? 1u : 0u), wf = wave_sum_u32(bl.count ? 1u : 0u);
    if (lane_id() == 0 && ws) {
        atomicAdd(&ba.counters->boxTests, wb);
        atomicAdd(&ba.counters->triTests, wt);
        atomicAdd(&ba.counters->raysTraced, (unsigned long long)ws);
        atomicAdd(&ba.counters->raysHit, (unsigned long long)wf);
    }
}
