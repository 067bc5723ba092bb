// rt_ray_hits.hip.h — k_ray_hits and k_ray_hits_resolve, the kernels of the all-hit ray queries (rt_query_hits; DESIGN.md,
// "All-hit ray queries").
//
// k_ray_hits: one lane per ray, wave64, 256-thread groups, no path state, rays read from the caller's packed arrays: the shape of
// k_trace and k_nearest_points. The rule is include/rt_ray_hits.h, the very functions the host walk compiles, so a candidate's
// distance has the same bits on both sides; and the bound is the constant T, so the set of candidates does not depend on the
// order of the visits: the device's node numbering and its near-child-first descent find the set the host's walk finds. Per ray:
// the sphere loop (both roots); then the objects in index order, each entered (no mask, no object hierarchy, no world-box skip:
// those shortcuts are proven against the shrinking search only): the ray goes to object space with the inverse rows and the
// object's tree is descended from the 64-byte child pairs with an explicit stack of far siblings, a child entered when its slab
// distance is < T; at a leaf every triangle that says didHit with dst < T, and that its alpha texel does not cut out, bumps the
// lane's count and goes through the header's insertion into the lane's sorted list of at most k entries.
// The stack is lane-interleaved in LDS as trace_wave's (entry e of lane l at word e * 64 + l: conflict-free) and holds far
// siblings only, one per level at most, so STACK >= the deepest leaf's depth is enough (ray_hits.h: hits_stack). The list, 8
// entries of 3 words, is lane-interleaved the same way: in LDS beside a 24-entry stack (24 KB + 24 KB), and, GLIST, in a ctx
// buffer per wave where the 64-entry stack takes the whole 64 KB. k == 0 keeps no list.
// The search leaves {dst, primitive word, triangle} in the first three words of each of the ray's k output records;
// k_ray_hits_resolve, one lane per record, turns them into the RtHit in place (reconstruct_hit<true>; a sphere root from the
// header's own function; the miss record where the slot is empty).
#pragma once

#include "rt_kernels.hip.h"
#include "rt_ray_hits.h"

#define RT_HIT_WORDS (sizeof(RtHit) / sizeof(uint32_t))

struct RayHitsArgs {
    const float* origins;     // n x 3, packed
    const float* dirs;
    const float* tmax;        // n, or NULL: RT_MISS_DST
    uint32_t n, k;
    uint32_t* hits;           // n x k RtHit records (NULL with k == 0)
    uint32_t* counts;         // n
    uint32_t* lists;          // GLIST: RT_HITS_MAX_K x RT_HITS_WORDS x 64 words per wave of the grid
    DevCounters* counters;
};

template <int STACK, bool GLIST>
__global__ __launch_bounds__(RT_BLOCK) void k_ray_hits(DevScene sc, RayHitsArgs ha) {
    constexpr uint32_t LIST = RT_HITS_MAX_K * RT_HITS_WORDS * RT_WAVE;   // words of a wave's lists
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * RT_WAVE];
    __shared__ uint32_t s_list[GLIST ? 1 : (RT_BLOCK / RT_WAVE) * LIST];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x / RT_WAVE, lane = threadIdx.x & (RT_WAVE - 1);
    uint32_t* const stack = s_stack + wave * STACK * RT_WAVE + lane;
    uint32_t* const list = GLIST ? ha.lists + ((size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * LIST + lane : s_list + wave * LIST + lane;

    uint32_t nBox = 0, nTri = 0, searched = 0, count = 0;
    if (gid < ha.n) {
        const size_t r = (size_t)gid * 3;
        const rt_vec3 ro = rt_v3(ha.origins[r], ha.origins[r + 1], ha.origins[r + 2]), rd = rt_v3(ha.dirs[r], ha.dirs[r + 1], ha.dirs[r + 2]);
        bool search;
        const float T = rt_hits_start(ha.tmax != nullptr, ha.tmax ? ha.tmax[gid] : 0.f, &search);
        const uint32_t k = ha.k;
        const bool alpha = (sc.mapFlags & RT_MAP_ALPHA) != 0u;
        uint32_t have = 0;
        if (search) {
            searched = 1;
            for (uint32_t i = 0; i < sc.sphereCount; i++) {
                const float4 s = sc.spheres[i];
                float tEntry, tExit;
                if (!rt_hits_sphere_roots(f4xyz(s), s.w, ro, rd, &tEntry, &tExit)) continue;
                if (rt_hits_accepts(tEntry, T)) { count++; have = rt_hits_insert(list, RT_WAVE, k, have, tEntry, rt_hits_sphere_word(i, false), 0u); }
                if (rt_hits_accepts(tExit, T)) { count++; have = rt_hits_insert(list, RT_WAVE, k, have, tExit, rt_hits_sphere_word(i, true), 0u); }
            }
            for (uint32_t obj = 0; obj < sc.objectCount; obj++) {
                const float4 r0 = sc.objInv[3 * (size_t)obj], r1 = sc.objInv[3 * (size_t)obj + 1], r2 = sc.objInv[3 * (size_t)obj + 2];
                const uint4 meta = sc.objMeta[obj];
                const rt_vec3 trd = xform_dir_rows(r0, r1, r2, rd), tro = xform_point_rows(r0, r1, r2, ro);
                const rt_vec3 inv = rt_v3(1.f / trd.x, 1.f / trd.y, 1.f / trd.z);
                uint32_t sp = 0, curIdx = meta.x, curCnt = meta.y;   // the root, untested
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
                            const float4 a = sc.triPos[3 * (size_t)j], b = sc.triPos[3 * (size_t)j + 1], c = sc.triPos[3 * (size_t)j + 2];
                            const RtHitsTri h = rt_hits_triangle(tro, trd, f4xyz(a), f4xyz(b), f4xyz(c), __float_as_uint(a.w) != 0u);
                            if (!h.didHit || !(h.dst < T)) continue;
                            if (alpha) {
                                TriHit th;
                                th.didHit = true; th.frontFace = h.frontFace; th.dst = h.dst; th.u = h.u; th.v = h.v; th.w = h.w;
                                if (alpha_cut(sc, obj, j, th)) continue;
                            }
                            count++;
                            have = rt_hits_insert(list, RT_WAVE, k, have, h.dst, obj, j);
                        }
                        have_node = false;
                    } else {
                        const float4* pr = sc.nodes + 2 * (size_t)curIdx;
                        const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
                        const bool in1 = rt_hits_box(f4xyz(lo1), f4xyz(hi1), tro, inv) < T;
                        const bool in2 = rt_hits_box(f4xyz(lo2), f4xyz(hi2), tro, inv) < T;
                        nBox += 2;
                        // (sp < STACK always: one far sibling per level, and hits_stack chose STACK >= the deepest leaf's depth; the
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
        ha.counts[gid] = count;
        for (uint32_t e = 0; e < k; e++) {
            uint32_t* const o = ha.hits + ((size_t)gid * k + e) * RT_HIT_WORDS;
            const uint32_t* const le = list + (size_t)e * RT_HITS_WORDS * RT_WAVE;
            const bool held = e < have;
            o[0] = held ? le[0] : __float_as_uint(RT_MISS_DST);
            o[1] = held ? le[RT_WAVE] : RT_HITS_EMPTY;
            o[2] = held ? le[2 * RT_WAVE] : 0u;
        }
    }

    // one atomic per wave and counter
    const unsigned long long wb = wave_sum_u64(nBox), wt = wave_sum_u64(nTri);
    const uint32_t ws = wave_sum_u32(searched), wf = wave_sum_u32(count ? 1u : 0u);
    if (lane_id() == 0 && ws) {
        atomicAdd(&ha.counters->boxTests, wb);
        atomicAdd(&ha.counters->triTests, wt);
        atomicAdd(&ha.counters->raysTraced, (unsigned long long)ws);
        atomicAdd(&ha.counters->raysHit, (unsigned long long)wf);
    }
}

// One lane per output record: {dst, primitive word, triangle} as the search left them -> the RtHit, in place
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_ray_hits_resolve(DevScene sc, RayHitsArgs ha) {
    const size_t slot = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (slot >= (size_t)ha.n * ha.k) return;
    const size_t ray = slot / ha.k;
    uint32_t* const w = ha.hits + slot * RT_HIT_WORDS;
    const float dst = __uint_as_float(w[0]);
    const uint32_t prim = w[1], tri = w[2];
    RtHit h;
    memset(&h, 0, sizeof(h));
    h.dst = RT_MISS_DST;
    if (prim != RT_HITS_EMPTY) {
        const rt_vec3 ro = rt_v3(ha.origins[3 * ray], ha.origins[3 * ray + 1], ha.origins[3 * ray + 2]);
        const rt_vec3 rd = rt_v3(ha.dirs[3 * ray], ha.dirs[3 * ray + 1], ha.dirs[3 * ray + 2]);
        rt_vec3 p, nrm;
        h.dst = dst;
        h.didHit = 1;
        if (rt_hits_is_sphere(prim)) {
            const uint32_t i = rt_hits_sphere_index(prim);
            const float4 s = rt_global(sc.spheres)[i];
            float tEntry, tExit;
            (void)rt_hits_sphere_roots(f4xyz(s), s.w, ro, rd, &tEntry, &tExit);
            const bool front = !rt_hits_sphere_exit(prim);
            p = rt_add(ro, rt_scale(rd, front ? tEntry : tExit));
            nrm = rt_scale(rt_normalize(rt_sub(p, f4xyz(s))), front ? 1.f : -1.f);
            h.isSphere = 1; h.objectHitIndex = i; h.materialIndex = rt_global(sc.sphereMat)[i]; h.frontFace = front ? 1u : 0u;
        } else {
            const FullHit f = reconstruct_hit<true>(sc, ro, rd, prim, tri);
            p = f.hitPoint; nrm = f.normal;
            h.objectHitIndex = prim; h.triHitIndex = tri; h.materialIndex = f.materialIndex; h.frontFace = f.frontFace ? 1u : 0u;
        }
        h.hitPoint[0] = p.x; h.hitPoint[1] = p.y; h.hitPoint[2] = p.z;
        h.normal[0] = nrm.x; h.normal[1] = nrm.y; h.normal[2] = nrm.z;
    }
    ((RtHit*)ha.hits)[slot] = h;
}
