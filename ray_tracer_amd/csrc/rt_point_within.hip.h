// rt_point_within.hip.h — k_points_within and k_points_within_resolve, the kernels of the radius point queries (rt_query_within;
// DESIGN.md, "Radius point queries").
//
// k_points_within: one lane per point, wave64, 256-thread groups, no path state, points read from the caller's packed array: the
// shape of k_nearest_points. The rule is include/rt_point_within.h over rt_point_query.h, the very functions the exhaustive host
// loop compiles, so a primitive's squared distance has the same bits on both sides; and the bound is the constant R2, so the set
// of members does not depend on the order of the visits: whatever the descent discards holds no member (rt_nearest_threshold;
// DESIGN.md has the derivation), and what is left is the set the host loop finds. Per point: the sphere loop; then the objects in
// index order, each skipped when its world box is farther than the padded bound, else entered: the point goes to object space
// with the inverse rows (an identity object reuses it) and the object's tree is descended from the 64-byte child pairs with an
// explicit stack of siblings, a child entered when its squared box distance does not exceed the object's threshold. Both
// thresholds are computed once per object: the bound never moves, so a popped entry needs no second test and the stack holds
// references only. At a leaf the corners go forward to world space, and every triangle with rt_point_triangle < R2 bumps the
// lane's count and goes through rt_ray_hits.h's insertion into the lane's sorted list of at most k entries.
// The stack is lane-interleaved in LDS as trace_wave's (entry e of lane l at word e * 64 + l: conflict-free) and holds siblings
// only, one per level at most, so STACK >= the deepest leaf's depth is enough (point_within.h: within_stack). The list, 8 entries
// of 3 words, is lane-interleaved the same way: in LDS beside a 24-entry stack (24 KB + 24 KB), and, GLIST, in a ctx buffer per
// wave where the 64-entry stack takes the whole 64 KB: what k_ray_hits does. k == 0 keeps no list.
// The search leaves {d2, primitive word, triangle} in the first three words of each of the point's k output records;
// k_points_within_resolve, one lane per record, turns them into the RtNearest in place through the header's builders (the
// not-found record where the slot is empty).
#pragma once

#include "rt_kernels.hip.h"
#include "rt_point_within.h"

#define RT_NEAREST_WORDS (sizeof(RtNearest) / sizeof(uint32_t))

struct WithinArgs {
    const float* points;      // n x 3, packed
    const float* maxDist;     // n, or NULL: no reach, every surface is a member
    uint32_t n, k;
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    uint32_t* out;            // n x k RtNearest records (NULL with k == 0)
    uint32_t* counts;         // n
    uint32_t* lists;          // GLIST: RT_WITHIN_MAX_K x RT_HITS_WORDS x 64 words per wave of the grid
    DevCounters* counters;
};

template <int STACK, bool GLIST>
__global__ __launch_bounds__(RT_BLOCK) void k_points_within(DevScene sc, WithinArgs wa) {
    constexpr uint32_t LIST = RT_WITHIN_MAX_K * RT_HITS_WORDS * RT_WAVE;   // words of a wave's lists
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * RT_WAVE];
    __shared__ uint32_t s_list[GLIST ? 1 : (RT_BLOCK / RT_WAVE) * LIST];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x / RT_WAVE, lane = threadIdx.x & (RT_WAVE - 1);
    uint32_t* const stack = s_stack + wave * STACK * RT_WAVE + lane;
    uint32_t* const list = GLIST ? wa.lists + ((size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * LIST + lane : s_list + wave * LIST + lane;

    uint32_t nBox = 0, nTri = 0, searched = 0, count = 0;
    if (gid < wa.n) {
        const size_t r = (size_t)gid * 3;
        const rt_vec3 q = rt_v3(wa.points[r], wa.points[r + 1], wa.points[r + 2]);
        bool search;
        const float R2 = rt_nearest_start(wa.maxDist != nullptr, wa.maxDist ? wa.maxDist[gid] : 0.f, &search);
        const uint32_t k = wa.k;
        uint32_t have = 0;
        if (search) {
            searched = 1;
            for (uint32_t i = 0; i < sc.sphereCount; i++) {
                const float4 s = sc.spheres[i];
                if (!rt_sphere_is_surface(s.w)) continue;
                rt_vec3 p;
                const float d2 = rt_point_sphere(q, f4xyz(s), s.w, &p);
                if (!rt_within_member(d2, R2)) continue;
                count++;
                have = rt_hits_insert(list, RT_WAVE, k, have, d2, rt_within_sphere_word(i), 0u);
            }
            const float qmax = rt_max(rt_max(rt_abs(q.x), rt_abs(q.y)), rt_abs(q.z));
            for (uint32_t obj = 0; obj < sc.objectCount; obj++) {
                const float4 n0 = wa.objNear[3 * (size_t)obj], n1 = wa.objNear[3 * (size_t)obj + 1], n2 = wa.objNear[3 * (size_t)obj + 2];
                const float sMin = n0.w, eta = rt_nearest_eta(qmax, n2.x, n0.w, n1.w);
                nBox++;
                if (rt_point_box2(q, f4xyz(n0), f4xyz(n1)) > rt_nearest_threshold(R2, eta, 1.f)) continue;
                const uint4 meta = sc.objMeta[obj];
                const bool ident = (meta.w & RT_OBJ_FWD_IDENTITY) != 0u;
                float4 f0 = make_float4(1.f, 0.f, 0.f, 0.f), f1 = make_float4(0.f, 1.f, 0.f, 0.f), f2 = make_float4(0.f, 0.f, 1.f, 0.f);
                rt_vec3 qo = q;
                if (!ident) {
                    qo = xform_point_rows(sc.objInv[3 * (size_t)obj], sc.objInv[3 * (size_t)obj + 1], sc.objInv[3 * (size_t)obj + 2], q);
                    f0 = sc.objFwd[3 * (size_t)obj]; f1 = sc.objFwd[3 * (size_t)obj + 1]; f2 = sc.objFwd[3 * (size_t)obj + 2];
                }
                const float thr = rt_nearest_threshold(R2, eta, sMin);   // once: the bound never moves
                uint32_t sp = 0, curIdx = meta.x, curCnt = meta.y;
                if (curCnt) leaf_from_ref(sc, meta.x, curIdx, curCnt);
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
                        nTri += curCnt;
                        for (uint32_t j = curIdx; j < curIdx + curCnt; j++) {
                            rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)j]), b = f4xyz(sc.triPos[3 * (size_t)j + 1]), c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
                            if (!ident) { a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c); }
                            float u, v;
                            const float d2 = rt_point_triangle(q, a, b, c, &u, &v);
                            if (!rt_within_member(d2, R2)) continue;
                            count++;
                            have = rt_hits_insert(list, RT_WAVE, k, have, d2, rt_within_triangle_word(obj), j);
                        }
                        have_node = false;
                    } else {
                        const float4* pr = sc.nodes + 2 * (size_t)curIdx;
                        const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
                        const bool in1 = !(rt_point_box2(qo, f4xyz(lo1), f4xyz(hi1)) > thr);
                        const bool in2 = !(rt_point_box2(qo, f4xyz(lo2), f4xyz(hi2)) > thr);
                        nBox += 2;
                        // (sp < STACK always: one sibling per level, and within_stack chose STACK >= the deepest leaf's depth; the
                        // test keeps a table that broke that promise from writing outside the stack)
                        if (in1 && in2 && sp < (uint32_t)STACK) { stack[sp * RT_WAVE] = __float_as_uint(lo2.w); sp++; }
                        if (in1 || in2) {
                            const uint32_t w = __float_as_uint(in1 ? lo1.w : lo2.w), cnt = __float_as_uint(in1 ? hi1.w : hi2.w);
                            curIdx = w; curCnt = cnt;
                            if (cnt) leaf_from_ref(sc, w, curIdx, curCnt);
                        } else have_node = false;
                    }
                }
            }
        }
        wa.counts[gid] = count;
        for (uint32_t e = 0; e < k; e++) {
            uint32_t* const o = wa.out + ((size_t)gid * k + e) * RT_NEAREST_WORDS;
            const uint32_t* const le = list + (size_t)e * RT_HITS_WORDS * RT_WAVE;
            const bool held = e < have;
            o[0] = held ? le[0] : 0u;
            o[1] = held ? le[RT_WAVE] : RT_HITS_EMPTY;
            o[2] = held ? le[2 * RT_WAVE] : 0u;
        }
    }

    // one atomic per wave and counter
    const unsigned long long wb = wave_sum_u64(nBox), wt = wave_sum_u64(nTri);
    const uint32_t ws = wave_sum_u32(searched), wf = wave_sum_u32(count ? 1u : 0u);
    if (lane_id() == 0 && ws) {
        atomicAdd(&wa.counters->boxTests, wb);
        atomicAdd(&wa.counters->triTests, wt);
        atomicAdd(&wa.counters->raysTraced, (unsigned long long)ws);
        atomicAdd(&wa.counters->raysHit, (unsigned long long)wf);
    }
}

// One lane per output record: {d2, primitive word, triangle} as the search left them -> the RtNearest, in place, three 16-byte stores
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_points_within_resolve(DevScene sc, WithinArgs wa) {
    const size_t slot = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (slot >= (size_t)wa.n * wa.k) return;
    const size_t point = slot / wa.k;
    uint32_t* const w = wa.out + slot * RT_NEAREST_WORDS;
    const float d2 = __uint_as_float(w[0]);
    const uint32_t prim = w[1], tri = w[2];
    RtNearest rec = rt_within_not_found();
    if (prim != RT_HITS_EMPTY) {
        const rt_vec3 q = rt_v3(wa.points[3 * point], wa.points[3 * point + 1], wa.points[3 * point + 2]);
        if (rt_hits_is_sphere(prim)) {
            const uint32_t i = rt_hits_sphere_index(prim);
            const float4 s = rt_global(sc.spheres)[i];
            rec = rt_within_sphere_record(q, f4xyz(s), s.w, i, d2);
        } else {
            rt_vec3 a = f4xyz(rt_global(sc.triPos)[3 * (size_t)tri]), b = f4xyz(rt_global(sc.triPos)[3 * (size_t)tri + 1]), c = f4xyz(rt_global(sc.triPos)[3 * (size_t)tri + 2]);
            if (!(rt_global(sc.objMeta)[prim].w & RT_OBJ_FWD_IDENTITY)) {
                const float4 f0 = rt_global(sc.objFwd)[3 * (size_t)prim], f1 = rt_global(sc.objFwd)[3 * (size_t)prim + 1], f2 = rt_global(sc.objFwd)[3 * (size_t)prim + 2];
                a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c);
            }
            rec = rt_within_triangle_record(q, a, b, c, prim, tri, d2);
        }
    }
    float4* const o = (float4*)w;
    o[0] = make_float4(rec.dst, __uint_as_float(rec.found), __uint_as_float(rec.isSphere), __uint_as_float(rec.objectIndex));
    o[1] = make_float4(__uint_as_float(rec.triIndex), rec.uv[0], rec.uv[1], rec.point[0]);
    o[2] = make_float4(rec.point[1], rec.point[2], 0.f, 0.f);
}
