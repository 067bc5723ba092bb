// rt_nearest.hip.h — k_nearest_points, the kernel of the point queries (rt_query_nearest; DESIGN.md, "Point queries").
//
// One lane per point, wave64, 256-thread groups, no path state. The rule is include/rt_point_query.h, the very functions the
// exhaustive host loop compiles, so a primitive's squared distance has the same bits on both sides and the minimum over the
// primitives the traversal visits equals the minimum over all of them as long as nothing nearer than the bound is discarded.
// Per point: the sphere loop; then the objects in index order, each skipped when its world box is farther than the padded bound,
// else entered: the point goes to object space with the inverse rows (an identity object reuses it), and the object's tree is
// descended best first with an explicit stack of far siblings — at an interior node the squared box distances of both children
// from the 64-byte child pair, the nearer one next, the farther one pushed if it survives the bound; a popped entry is tested
// again against the bound as it stands then (RETEST: its squared distance rides in the stack next to it); at a leaf the corners
// go forward to world space and rt_point_triangle decides. A subtree is discarded only when its squared box distance exceeds
// rt_nearest_threshold(best2, eta, sMin), recomputed only when best2 changes.
// The stack is lane-interleaved in LDS as trace_wave's (entry e of lane l at word e * 64 + l: conflict-free) and holds far
// siblings only, one per level at most, so STACK >= the deepest leaf's depth is enough (point_queries.h: nearest_stack).
#pragma once

#include "rt_kernels.hip.h"
#include "rt_point_query.h"

struct NearestArgs {
    const float* points;      // n x 3, packed
    const float* maxDist;     // n, or NULL: no limit
    uint32_t n;
    const float4* objNear;    // 3 x float4 per object (point_queries.h: layout_nearest)
    float4* out;              // 3 x float4 per point: the RtNearest records
    DevCounters* counters;
};

template <int STACK, bool RETEST>
__global__ __launch_bounds__(RT_BLOCK) void k_nearest_points(DevScene sc, NearestArgs na) {
    constexpr int WORDS = RETEST ? 2 : 1;   // per entry: the reference, and with RETEST the squared box distance it was pushed with
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * STACK * WORDS * RT_WAVE];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    uint32_t* const stack = s_stack + (threadIdx.x / RT_WAVE) * STACK * WORDS * RT_WAVE + (threadIdx.x & (RT_WAVE - 1));

    uint32_t nBox = 0, nTri = 0, searched = 0, found = 0;
    if (gid < na.n) {
        const size_t r = (size_t)gid * 3;
        const rt_vec3 q = rt_v3(na.points[r], na.points[r + 1], na.points[r + 2]);
        bool search;
        float best2 = rt_nearest_start(na.maxDist != nullptr, na.maxDist ? na.maxDist[gid] : 0.f, &search);
        uint32_t bestObj = RT_HIT_NONE, bestTri = 0;
        float bestU = 0.f, bestV = 0.f;
        if (search) {
            searched = 1;
            for (uint32_t i = 0; i < sc.sphereCount; i++) {
                const float4 s = sc.spheres[i];
                if (!rt_sphere_is_surface(s.w)) continue;
                rt_vec3 p;
                const float d2 = rt_point_sphere(q, f4xyz(s), s.w, &p);
                if (d2 < best2) { best2 = d2; bestObj = RT_HIT_SPHERE | i; }
            }
            const float qmax = rt_max(rt_max(rt_abs(q.x), rt_abs(q.y)), rt_abs(q.z));
            for (uint32_t obj = 0; obj < sc.objectCount; obj++) {
                const float4 n0 = na.objNear[3 * (size_t)obj], n1 = na.objNear[3 * (size_t)obj + 1], n2 = na.objNear[3 * (size_t)obj + 2];
                const float sMin = n0.w, eta = rt_nearest_eta(qmax, n2.x, n0.w, n1.w);
                nBox++;
                if (rt_point_box2(q, f4xyz(n0), f4xyz(n1)) > rt_nearest_threshold(best2, eta, 1.f)) continue;
                const uint4 meta = sc.objMeta[obj];
                const bool ident = (meta.w & RT_OBJ_FWD_IDENTITY) != 0u;
                float4 f0 = make_float4(1.f, 0.f, 0.f, 0.f), f1 = make_float4(0.f, 1.f, 0.f, 0.f), f2 = make_float4(0.f, 0.f, 1.f, 0.f);
                rt_vec3 qo = q;
                if (!ident) {
                    qo = xform_point_rows(sc.objInv[3 * (size_t)obj], sc.objInv[3 * (size_t)obj + 1], sc.objInv[3 * (size_t)obj + 2], q);
                    f0 = sc.objFwd[3 * (size_t)obj]; f1 = sc.objFwd[3 * (size_t)obj + 1]; f2 = sc.objFwd[3 * (size_t)obj + 2];
                }
                float thr = rt_nearest_threshold(best2, eta, sMin);
                uint32_t sp = 0, curIdx = meta.x, curCnt = meta.y;
                if (curCnt) leaf_from_ref(sc, meta.x, curIdx, curCnt);
                bool have = true;
                for (;;) {
                    if (!have) {
                        if (sp == 0) break;
                        --sp;
                        const uint32_t ref = stack[sp * RT_WAVE];
                        if (RETEST && __uint_as_float(stack[(STACK + sp) * RT_WAVE]) > thr) continue;   // the bound has come down since the push
                        if (ref & RT_LEAF_BIT) leaf_from_ref(sc, ref, curIdx, curCnt);
                        else { curIdx = ref; curCnt = 0; }
                        have = true;
                    }
                    if (curCnt != 0) {
                        nTri += curCnt;
                        for (uint32_t j = curIdx; j < curIdx + curCnt; j++) {
                            rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)j]), b = f4xyz(sc.triPos[3 * (size_t)j + 1]), c = f4xyz(sc.triPos[3 * (size_t)j + 2]);
                            if (!ident) { a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c); }
                            float u, v;
                            const float d2 = rt_point_triangle(q, a, b, c, &u, &v);
                            if (d2 < best2) {
                                best2 = d2; bestObj = obj; bestTri = j; bestU = u; bestV = v;
                                thr = rt_nearest_threshold(best2, eta, sMin);
                            }
                        }
                        have = false;
                    } else {
                        const float4* pr = sc.nodes + 2 * (size_t)curIdx;
                        const float4 lo1 = pr[0], hi1 = pr[1], lo2 = pr[2], hi2 = pr[3];
                        const float d1 = rt_point_box2(qo, f4xyz(lo1), f4xyz(hi1));
                        const float d2 = rt_point_box2(qo, f4xyz(lo2), f4xyz(hi2));
                        nBox += 2;
                        const bool nearA = d1 <= d2;
                        const float dNear = nearA ? d1 : d2, dFar = nearA ? d2 : d1;
                        const uint32_t nW = __float_as_uint(nearA ? lo1.w : lo2.w), nCnt = __float_as_uint(nearA ? hi1.w : hi2.w);
                        const uint32_t fW = __float_as_uint(nearA ? lo2.w : lo1.w);
                        // (sp < STACK always: one far sibling per level, and nearest_stack chose STACK >= the deepest leaf's depth;
                        // the test keeps a table that broke that promise from writing outside the stack)
                        if (!(dFar > thr) && sp < (uint32_t)STACK) {
                            stack[sp * RT_WAVE] = fW;
                            if (RETEST) stack[(STACK + sp) * RT_WAVE] = __float_as_uint(dFar);
                            sp++;
                        }
                        if (!(dNear > thr)) {
                            curIdx = nW; curCnt = nCnt;
                            if (nCnt) leaf_from_ref(sc, nW, curIdx, curCnt);
                        } else have = false;
                    }
                }
            }
        }

        // the record: three 16-byte stores
        float dst = RT_MISS_DST, u = 0.f, v = 0.f;
        uint32_t isSphere = 0, objIdx = 0, triIdx = 0;
        rt_vec3 p = rt_v3(0.f, 0.f, 0.f);
        if (bestObj != RT_HIT_NONE) {
            found = 1;
            dst = rt_sqrt(best2);
            if (bestObj & RT_HIT_SPHERE) {
                isSphere = 1; objIdx = bestObj & ~RT_HIT_SPHERE;
                const float4 s = sc.spheres[objIdx];
                (void)rt_point_sphere(q, f4xyz(s), s.w, &p);
            } else {
                objIdx = bestObj; triIdx = bestTri; u = bestU; v = bestV;
                rt_vec3 a = f4xyz(sc.triPos[3 * (size_t)bestTri]), b = f4xyz(sc.triPos[3 * (size_t)bestTri + 1]), c = f4xyz(sc.triPos[3 * (size_t)bestTri + 2]);
                if (!(sc.objMeta[bestObj].w & RT_OBJ_FWD_IDENTITY)) {
                    const float4 f0 = sc.objFwd[3 * (size_t)bestObj], f1 = sc.objFwd[3 * (size_t)bestObj + 1], f2 = sc.objFwd[3 * (size_t)bestObj + 2];
                    a = xform_point_rows(f0, f1, f2, a); b = xform_point_rows(f0, f1, f2, b); c = xform_point_rows(f0, f1, f2, c);
                }
                p = rt_bary_point(a, b, c, u, v);
            }
        }
        float4* const o = na.out + 3 * (size_t)gid;
        o[0] = make_float4(dst, __uint_as_float(found), __uint_as_float(isSphere), __uint_as_float(objIdx));
        o[1] = make_float4(__uint_as_float(triIdx), u, v, p.x);
        o[2] = make_float4(p.y, p.z, 0.f, 0.f);
    }

    // one atomic per wave and counter
    const unsigned long long wb = wave_sum_u64(nBox), wt = wave_sum_u64(nTri);
    const uint32_t ws = wave_sum_u32(searched), wf = wave_sum_u32(found);
    if (lane_id() == 0 && ws) {
        atomicAdd(&na.counters->boxTests, wb);
        atomicAdd(&na.counters->triTests, wt);
        atomicAdd(&na.counters->raysTraced, (unsigned long long)ws);
        atomicAdd(&na.counters->raysHit, (unsigned long long)wf);
    }
}
