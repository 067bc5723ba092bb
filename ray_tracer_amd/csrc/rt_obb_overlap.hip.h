// rt_obb_overlap.hip.h — k_obbs_overlap, the kernel of the oriented box queries (rt_query_oriented_boxes; DESIGN.md, "Oriented box
// queries").
//
// k_boxes_overlap's shape (rt_box_overlap.hip.h): one lane per box, wave64, 256-thread groups, no path state, the batch read from
// the caller's packed arrays; a sibling-only stack lane-interleaved in LDS (entry e of lane l at word e * 64 + l: conflict-free);
// the list of 8 entries of 2 words lane-interleaved the same way, in LDS beside a 24-entry stack (24 KB + 16 KB) and, GLIST, in a
// ctx buffer per wave where the 64-entry stack takes the whole 64 KB; the records written by the search itself, one 16-byte store
// each; one atomic per wave and counter. The rule is include/rt_obb_overlap.h, the very functions the exhaustive host loop
// compiles, so a pair's verdict is the same on both sides, and membership does not depend on the order of the visits.
// What is new is the descent. A member triangle passed stage 1 of rt_box_triangle on its fp32 frame corners, so a subtree goes
// only when a box that holds every such corner lies strictly apart from the local box [lo, hi] on one of ITS axes: the node's box
// is taken through a map G as G c +- |G| e (rt_obb_apart) and padded by rt_obb_pad of a magnitude computed per lane and object.
// For an identity object G is the frame F itself and the magnitude |F| |[w; 1]| over the object's root box; for a placed one
// G = fl(F M) is composed once per lane and object, so that a node's box is rounded out once, not twice, and a box in an
// object's own coordinates (F = M's inverse) prunes as an axis-aligned one does. An object is skipped by its world box
// (layout_nearest's; a placed one's grown by rt_box_pad of its scale, as k_boxes_overlap grows it) taken through F. The three
// world axes against the box's world extent are not tested: that needs the box's corners in world space, hence an inverse.
// The frame is read per lane (a shared frame through a per-lane zero), so its twelve numbers are vector loads into vector
// registers; k_boxes_overlap's comment on the forward rows says why.
#pragma once

#include "rt_kernels.hip.h"
#include "rt_obb_overlap.h"

struct ObbsArgs {
    const float* frames;      // 16 floats a box, or 16 in all (shared)
    const float* lo;          // n x 3, packed
    const float* hi;          // n x 3, packed
    uint32_t n, k, shared;
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    uint4* out;               // n x k RtOverlap records (NULL with k == 0)
    uint32_t* counts;         // n
    uint32_t* lists;          // GLIST: RT_BOXES_MAX_K x RT_BOX_WORDS x 64 words per wave of the grid
    DevCounters* counters;
};

// What a lane carries through a search: the box in its frame, its list and its tallies
struct ObbLane {
    RtObbFrame f;
    rt_vec3 lo, hi;
    uint32_t* stack;   // entry e at stack[e * RT_WAVE]
    uint32_t* list;    // entry e's word w at list[(e * RT_BOX_WORDS + w) * RT_WAVE]
    uint32_t k, have, count, nBox, nTri;
};

// The descent of one object's tree. g: the map from the node boxes' space to the frame (F, or F M of a placed object) and pad the
// pad of its magnitude; placed: the corners go through the forward rows m0..m2 first.
template <int STACK>
__device__ __forceinline__ void obbs_descend(const DevScene& sc, ObbLane& bl, uint32_t obj, uint32_t root, uint32_t rootCnt, bool placed, float4 m0, float4 m1, float4 m2, RtObbFrame g, float pad) {
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
                if (placed) { a = xform_point_rows(m0, m1, m2, a); b = xform_point_rows(m0, m1, m2, b); c = xform_point_rows(m0, m1, m2, c); }
                if (!rt_obb_triangle(bl.f, lo, hi, a, b, c)) continue;
                bl.count++;
                bl.have = rt_box_insert(bl.list, RT_WAVE, bl.k, bl.have, rt_box_triangle_word(obj), j);
            }
            have_node = false;
        } else {
            const float4* pr = sc.nodes + 2 * (size_t)curIdx;
            const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
            const bool in1 = !rt_obb_apart(lo, hi, g, f4xyz(lo1), f4xyz(hi1), pad);
            const bool in2 = !rt_obb_apart(lo, hi, g, f4xyz(lo2), f4xyz(hi2), pad);
            bl.nBox += 2;
            // (sp < STACK always: one sibling per level, and obbs_stack chose STACK >= the deepest leaf's depth; the test keeps
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
__global__ __launch_bounds__(RT_BLOCK) void k_obbs_overlap(DevScene sc, ObbsArgs ba) {
    constexpr uint32_t LIST = RT_BOXES_MAX_K * RT_BOX_WORDS * RT_WAVE;   // words of a wave's lists
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * RT_WAVE];
    __shared__ uint32_t s_list[GLIST ? 1 : (RT_BLOCK / RT_WAVE) * LIST];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x / RT_WAVE, lane = threadIdx.x & (RT_WAVE - 1);
    const bool mine = gid < ba.n;
    ObbLane bl;
    bl.stack = s_stack + wave * STACK * RT_WAVE + lane;
    bl.list = GLIST ? ba.lists + ((size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * LIST + lane : s_list + wave * LIST + lane;
    bl.k = ba.k; bl.have = 0; bl.count = 0; bl.nBox = 0; bl.nTri = 0;
    // (a lane past the batch takes an inverted box: not valid, not searched)
    bl.lo = rt_v3(1.f, 1.f, 1.f); bl.hi = rt_v3(0.f, 0.f, 0.f);
    bl.f = rt_obb_identity();
    if (mine) {
        const size_t r = (size_t)gid * 3;
        bl.lo = rt_v3(ba.lo[r], ba.lo[r + 1], ba.lo[r + 2]); bl.hi = rt_v3(ba.hi[r], ba.hi[r + 1], ba.hi[r + 2]);
        // a shared frame through a per-lane zero (threadIdx.y is 0 in this one-dimensional launch): vector loads either way
        bl.f = rt_obb_frame(rt_global(ba.frames) + (size_t)(ba.shared ? threadIdx.y : gid) * RT_OBB_FRAME_FLOATS);
    }
    const bool searched = rt_obb_valid(bl.f, bl.lo, bl.hi);
    if (searched) {
        const float scale = rt_obb_scale(bl.f);
        for (uint32_t i = 0; i < sc.sphereCount; i++) {
            const float4 s = sc.spheres[i];
            if (!rt_sphere_is_surface(s.w)) continue;
            if (!rt_obb_sphere(bl.f, scale, bl.lo, bl.hi, f4xyz(s), s.w)) continue;
            bl.count++;
            bl.have = rt_box_insert(bl.list, RT_WAVE, bl.k, bl.have, rt_box_sphere_word(i), 0u);
        }
        for (uint32_t obj = 0; obj < sc.objectCount; obj++) {
            const float4 n0 = ba.objNear[3 * (size_t)obj], n1 = ba.objNear[3 * (size_t)obj + 1];
            const float objMag = ba.objNear[3 * (size_t)obj + 2].x;
            const uint4 meta = sc.objMeta[obj];
            bl.nBox++;
            const bool placed = (meta.w & RT_OBJ_FWD_IDENTITY) == 0u;
            // the object's world box: exact for an identity object, grown by the pad of its scale for a placed one
            const float grow = placed ? rt_box_pad(objMag) : 0.f;
            const rt_vec3 olo = rt_v3(n0.x - grow, n0.y - grow, n0.z - grow), ohi = rt_v3(n1.x + grow, n1.y + grow, n1.z + grow);
            const float magF = rt_obb_mag(bl.f, olo, ohi);
            if (rt_obb_apart(bl.lo, bl.hi, bl.f, olo, ohi, rt_obb_pad(magF))) continue;
            // (the rows through a per-lane index: k_boxes_overlap's comment)
            const float4* const fwd = rt_global(sc.objFwd) + 3 * (size_t)(obj + threadIdx.y);
            float4 m0 = make_float4(1.f, 0.f, 0.f, 0.f), m1 = make_float4(0.f, 1.f, 0.f, 0.f), m2 = make_float4(0.f, 0.f, 1.f, 0.f);
            RtObbFrame g = bl.f;
            float pad = rt_obb_pad(magF);
            if (placed) {
                m0 = fwd[0]; m1 = fwd[1]; m2 = fwd[2];
                g = rt_obb_compose(bl.f, f4xyz(m0), f4xyz(m1), f4xyz(m2), rt_v3(m0.w, m1.w, m2.w));
                pad = rt_obb_pad(rt_obb_mag_placed(bl.f, objMag));
            }
            obbs_descend<STACK>(sc, bl, obj, meta.x, meta.y, placed, m0, m1, m2, g, pad);
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
