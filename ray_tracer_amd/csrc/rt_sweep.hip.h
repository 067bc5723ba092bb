// rt_sweep.hip.h — k_sweep_spheres, the kernel of the sphere sweeps (rt_query_sweep; DESIGN.md, "Sphere sweeps").
//
// One lane per ray, wave64, 256-thread groups, no path state, rays read from the caller's packed arrays: the shape of
// k_nearest_points. The rule is include/rt_sweep.h over rt_point_query.h, the very functions the exhaustive host loop compiles, so a
// primitive's contact time has the same bits on both sides; the key {t, primitive word, triangle} is total, so the least of it
// over the primitives the descent visits equals the least over all of them as long as nothing that holds a contact at or below
// the bound is discarded (rt_sweep_box_open on boxes grown by rt_sweep_pad; DESIGN.md has the derivation).
// Per ray: the sphere loop; then the objects in index order through the objNear table, each skipped when the ray's interval with
// its grown world box is closed, else entered: the ray goes to object space with the inverse rows (the origin as a point, the
// direction through the 3x3; an identity object reuses both) and the object's tree is descended in order of the grown boxes'
// entry times with an explicit stack of far siblings — at an interior node both children from the 64-byte child pair, the nearer
// one next, the farther one pushed if it is open; a popped entry is tested again against the bound as it stands then (RETEST: its
// entry time rides in the stack next to it); at a leaf the corners go forward to world space and rt_sweep_triangle decides. Both
// pads are computed once per object: they do not depend on the bound.
// The stack is lane-interleaved in LDS as k_nearest_points' (entry e of lane l at word e * 64 + l: conflict-free) and holds far
// siblings only, one per level at most, so STACK >= the deepest leaf's depth is enough (sweep_queries.h: sweep_stack).
#pragma once

#include "rt_kernels.hip.h"
#include "rt_sweep.h"

struct SweepArgs {
    const float* origins;     // n x 3, packed
    const float* dirs;        // n x 3
    const float* radius;      // n
    const float* tmax;        // n, or NULL: no limit
    uint32_t n;
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    float4* out;              // 4 x float4 per ray: the RtSweep records
    DevCounters* counters;
};

template <int STACK, bool RETEST>
__global__ __launch_bounds__(RT_BLOCK) void k_sweep_spheres(DevScene sc, SweepArgs sa) {
    constexpr int WORDS = RETEST ? 2 : 1;   // per entry: the reference, and with RETEST the entry time it was pushed with
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * WORDS * RT_WAVE];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    uint32_t* const stack = s_stack + (threadIdx.x / RT_WAVE) * STACK * WORDS * RT_WAVE + (threadIdx.x & (RT_WAVE - 1));

    // the four counters are adjacent: lanes 0..3 of a wave add one each, in one atomic instruction, through an address that is a
    // lane value from the start (held in scalar registers to the end, the block's address is one more pair than there are)
    static_assert(offsetof(DevCounters, triTests) == 8 && offsetof(DevCounters, raysTraced) == 16 && offsetof(DevCounters, raysHit) == 24, "four adjacent counters");
    unsigned long long* const counter = &sa.counters->boxTests + (lane_id() & 3u);

    uint32_t nBox = 0, nTri = 0, searched = 0, found = 0;
    const bool live = gid < sa.n;
    {
        const uint32_t ray = live ? gid : 0u;   // a lane past the batch reads ray 0 (n > 0), searches nothing and writes nothing
        const size_t r = (size_t)ray * 3;
        float4* const w = sa.out + 4 * (size_t)ray;   // (a lane value from here on)
        const rt_vec3 o = rt_v3(sa.origins[r], sa.origins[r + 1], sa.origins[r + 2]);
        const rt_vec3 d = rt_v3(sa.dirs[r], sa.dirs[r + 1], sa.dirs[r + 2]);
        const float R = sa.radius[ray], dd = rt_dot(d, d);
        bool search;
        const float T = rt_sweep_start(d, R, sa.tmax != nullptr, sa.tmax ? sa.tmax[ray] : 0.f, &search);
        search = search && live;
        float best = T;
        uint32_t bestPrim = RT_HITS_EMPTY, bestTri = 0;
        float4 bestSphere = make_float4(0.f, 0.f, 0.f, 0.f);   // the sphere that holds the answer, for its record
        searched = search ? 1u : 0u;
        // A lane that does not search runs neither loop: its indices start past the end. That also makes them lane values, so
        // what they index (the pruning record, the rows) is fetched per lane into vector registers: held in scalar ones through
        // the descent, beside the saved masks of the rule's nested branches, they do not fit.
        {
            for (uint32_t i = search ? 0u : sc.sphereCount; i < sc.sphereCount; i++) {
                const float4 s = sc.spheres[i];
                if (!rt_sphere_is_surface(s.w)) continue;
                float t, d2;
                if (!rt_sweep_sphere(o, d, dd, R, f4xyz(s), s.w, &t, &d2)) continue;
                const uint32_t word = rt_hits_sphere_word(i, false);
                if (rt_sweep_replaces(t, word, 0u, T, best, bestPrim, bestTri)) { best = t; bestPrim = word; bestTri = 0; bestSphere = s; }
            }
            const float omax = rt_max3abs(o);
            const rt_vec3 inv = rt_sweep_inv(d);
            const uint32_t firstObj = search ? 0u : sc.objectCount;
            const float4* nearOf = sa.objNear + 3 * (size_t)firstObj;   // (walked, not indexed: the table's address need not outlive this line)
            for (uint32_t obj = firstObj; obj < sc.objectCount; obj++, nearOf += 3) {
                const float4 n0 = nearOf[0], n1 = nearOf[1], n2 = nearOf[2];
                float entry, exit;
                nBox++;
                rt_sweep_box(f4xyz(n0), f4xyz(n1), o, inv, rt_sweep_pad(R, omax, n2.x, n0.w, n1.w, 1.f), &entry, &exit);
                if (!rt_sweep_box_open(entry, exit, best)) continue;
                const uint4 meta = sc.objMeta[obj];
                const bool ident = (meta.w & RT_OBJ_FWD_IDENTITY) != 0u;
                float4 f0 = make_float4(1.f, 0.f, 0.f, 0.f), f1 = make_float4(0.f, 1.f, 0.f, 0.f), f2 = make_float4(0.f, 0.f, 1.f, 0.f);
                rt_vec3 oo = o, od = d, oinv = inv;
                if (!ident) {
                    const float4 i0 = sc.objInv[3 * (size_t)obj], i1 = sc.objInv[3 * (size_t)obj + 1], i2 = sc.objInv[3 * (size_t)obj + 2];
                    oo = xform_point_rows(i0, i1, i2, o);
                    od = xform_dir_rows(i0, i1, i2, d);
                    oinv = rt_sweep_inv(od);
                    f0 = sc.objFwd[3 * (size_t)obj]; f1 = sc.objFwd[3 * (size_t)obj + 1]; f2 = sc.objFwd[3 * (size_t)obj + 2];
                }
                const float g = rt_sweep_pad(R, omax, n2.x, n0.w, n1.w, n0.w);   // once: it does not depend on the bound
                uint32_t sp = 0, curIdx = meta.x, curCnt = meta.y;
                if (curCnt) leaf_from_ref(sc, meta.x, curIdx, curCnt);
                bool have = true;
                for (;;) {
                    if (!have) {
                        if (sp == 0) break;
                        --sp;
                        const uint32_t ref = stack[sp * RT_WAVE];
                        if (RETEST && __uint_as_float(stack[(STACK + sp) * RT_WAVE]) * RT_SWEEP_TDOWN > best) continue;   // the bound has come down since the push
                        if (ref & RT_LEAF_BIT) leaf_from_ref(sc, ref, curIdx, curCnt);
                        else { curIdx = ref; curCnt = 0; }
                        have = true;
                    }
                    if (curCnt != 0) {
                        nTri += curCnt;
                        for (uint32_t j = curIdx; j < curIdx + curCnt; j++) {
                            rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)j]), b = f4xyz(sc.triPos[3 * (size_t)j + 1]), c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
                            if (!ident) { a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c); }
                            float t, d2, u, v;
                            if (!rt_sweep_triangle(o, d, dd, R, a, b, c, &t, &d2, &u, &v)) continue;
                            if (rt_sweep_replaces(t, obj, j, T, best, bestPrim, bestTri)) { best = t; bestPrim = obj; bestTri = j; }
                        }
                        have = false;
                    } else {
                        const float4* pr = sc.nodes + 2 * (size_t)curIdx;
                        const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
                        float e1, x1, e2, x2;
                        rt_sweep_box(f4xyz(lo1), f4xyz(hi1), oo, oinv, g, &e1, &x1);
                        rt_sweep_box(f4xyz(lo2), f4xyz(hi2), oo, oinv, g, &e2, &x2);
                        nBox += 2;
                        const bool open1 = rt_sweep_box_open(e1, x1, best), open2 = rt_sweep_box_open(e2, x2, best);
                        const bool nearA = open1 && (!open2 || !(e2 < e1));
                        const bool openNear = nearA ? open1 : open2, openFar = nearA ? open2 : open1;
                        const float eFar = nearA ? e2 : e1;
                        const uint32_t nW = __float_as_uint(nearA ? lo1.w : lo2.w), nCnt = __float_as_uint(nearA ? hi1.w : hi2.w);
                        const uint32_t fW = __float_as_uint(nearA ? lo2.w : lo1.w);
                        // (sp < STACK always: one far sibling per level, and sweep_stack chose STACK >= the deepest leaf's depth;
                        // the test keeps a table that broke that promise from writing outside the stack)
                        if (openNear && openFar && sp < (uint32_t)STACK) {
                            stack[sp * RT_WAVE] = fW;
                            if (RETEST) stack[(STACK + sp) * RT_WAVE] = __float_as_uint(eFar);
                            sp++;
                        }
                        if (openNear) {
                            curIdx = nW; curCnt = nCnt;
                            if (nCnt) leaf_from_ref(sc, nW, curIdx, curCnt);
                        } else have = false;
                    }
                }
            }
        }

        // the record: four 16-byte stores
        RtSweep rec = rt_sweep_not_found();
        if (bestPrim != RT_HITS_EMPTY) {
            found = 1;
            if (rt_hits_is_sphere(bestPrim)) {
                rec = rt_sweep_sphere_record(o, d, best, f4xyz(bestSphere), bestSphere.w, rt_hits_sphere_index(bestPrim));
            } else {
                rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)bestTri]), b = f4xyz(sc.triPos[3 * (size_t)bestTri + 1]), c = f4xyz(sc.triPos[3 * (size_t)bestTri + 2]);
                if (!(sc.objMeta[bestPrim].w & RT_OBJ_FWD_IDENTITY)) {
                    const float4 f0 = sc.objFwd[3 * (size_t)bestPrim], f1 = sc.objFwd[3 * (size_t)bestPrim + 1], f2 = sc.objFwd[3 * (size_t)bestPrim + 2];
                    a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c);
                }
                rec = rt_sweep_triangle_record(o, d, best, a, b, c, bestPrim, bestTri);
            }
        }
        if (live) {
        w[0] = make_float4(rec.t, __uint_as_float(rec.found), __uint_as_float(rec.isSphere), __uint_as_float(rec.objectIndex));
        w[1] = make_float4(__uint_as_float(rec.triIndex), rec.uv[0], rec.uv[1], rec.gap);
        w[2] = make_float4(rec.point[0], rec.point[1], rec.point[2], __uint_as_float(rec.startsInContact));
        w[3] = make_float4(rec.normal[0], rec.normal[1], rec.normal[2], 0.f);
        }
    }

    // one atomic instruction per wave
    const unsigned long long wb = wave_sum_u64(nBox), wt = wave_sum_u64(nTri);
    const uint32_t ws = wave_sum_u32(searched), wf = wave_sum_u32(found);
    const uint32_t l = lane_id();
    if (l < 4u && ws) atomicAdd(counter, l == 0u ? wb : l == 1u ? wt : (unsigned long long)(l == 2u ? ws : wf));
}
