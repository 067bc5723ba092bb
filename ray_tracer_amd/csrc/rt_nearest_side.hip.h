// rt_nearest_side.hip.h — k_nearest_side, the side pass of the signed point queries (rt_query_nearest_signed; DESIGN.md, "Signed
// point queries"). It runs after k_nearest_points on the same stream and reads what that wrote.
//
// One lane per point, wave64, 256-thread groups, no LDS, no stack. The rule is include/rt_point_side.h, the very functions
// rt_nearest_side_host compiles, read through DevSideAcc: a lane loads its point and its 48-byte record, the three corners of the
// reported triangle (placed by the object's forward rows exactly as k_nearest_points placed them), classifies the feature, loads
// the triangle's one row of the topology table and only the neighbours the feature needs — none for a face, one for an edge, the
// fan for a vertex — and writes one byte. A pass of its own and not a template flag of k_nearest_points: the fan walk's registers
// must not cost the search its occupancy. The group size is a template parameter so that the kernel is an instantiation: the
// compiler emits instantiations behind the plain kernels, at the point of their first use, so this one lands behind
// k_nearest_points and no kernel a render or the bench runs moves in the code object.
#pragma once

#include "rt_kernels.hip.h"
#include "rt_point_side.h"

struct SideArgs {
    const float* points;      // n x 3, packed
    uint32_t n;
    const float4* recs;       // 3 x float4 per point: the RtNearest records k_nearest_points wrote
    const uint4* topo;        // one row per triangle (mesh_topology.h)
    const int32_t* orient;    // one per object: +1, -1, 0
    int8_t* side;             // n bytes
    DevCounters* counters;
};

struct DevSideAcc {
    const float4* triPos;
    const uint4* topo;
    float4 f0, f1, f2;
    bool ident;
    __device__ __forceinline__ rt_topo_row row(uint32_t tri) const {
        const uint4 w = topo[tri];
        rt_topo_row r;
        r.n[0] = w.x; r.n[1] = w.y; r.n[2] = w.z; r.flags = w.w;
        return r;
    }
    __device__ __forceinline__ void corners(uint32_t tri, rt_vec3* a, rt_vec3* b, rt_vec3* c) const {
        *a = f4xyz(triPos[3 * (size_t)tri]); *b = f4xyz(triPos[3 * (size_t)tri + 1]); *c = f4xyz(triPos[3 * (size_t)tri + 2]);
        if (!ident) { *a = xform_point_rows(f0, f1, f2, *a); *b = xform_point_rows(f0, f1, f2, *b); *c = xform_point_rows(f0, f1, f2, *c); }
    }
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_nearest_side(DevScene sc, SideArgs sa) {
    const uint32_t gid = blockIdx.x * THREADS + threadIdx.x;
    uint32_t isSigned = 0;
    if (gid < sa.n) {
        const size_t r = (size_t)gid * 3;
        const rt_vec3 q = rt_v3(sa.points[r], sa.points[r + 1], sa.points[r + 2]);
        const float4 r0 = sa.recs[r], r1 = sa.recs[r + 1];
        const uint32_t found = __float_as_uint(r0.y), isSphere = __float_as_uint(r0.z), obj = __float_as_uint(r0.w), tri = __float_as_uint(r1.x);
        int side = 0;
        if (found && isSphere) {
            if (obj < sc.sphereCount) {
                const float4 s = sc.spheres[obj];
                side = rt_point_side_sphere(q, f4xyz(s), s.w);
            }
        } else if (found && obj < sc.objectCount && tri < sc.triCount) {   // (the record is k_nearest_points' own: the test is a guard)
            DevSideAcc acc;
            acc.triPos = sc.triPos; acc.topo = sa.topo;
            acc.ident = (sc.objMeta[obj].w & RT_OBJ_FWD_IDENTITY) != 0u;
            acc.f0 = make_float4(1.f, 0.f, 0.f, 0.f); acc.f1 = make_float4(0.f, 1.f, 0.f, 0.f); acc.f2 = make_float4(0.f, 0.f, 1.f, 0.f);
            if (!acc.ident) { acc.f0 = sc.objFwd[3 * (size_t)obj]; acc.f1 = sc.objFwd[3 * (size_t)obj + 1]; acc.f2 = sc.objFwd[3 * (size_t)obj + 2]; }
            int feature;
            uint32_t fan;
            side = rt_point_side_triangle(acc, q, tri, r1.y, r1.z, (int)sa.orient[obj], &feature, &fan);
        }
        sa.side[gid] = (int8_t)side;
        isSigned = side != 0 ? 1u : 0u;
    }
    // one atomic per wave
    const uint32_t ws = wave_sum_u32(isSigned);
    if (lane_id() == 0 && ws) atomicAdd(&sa.counters->segments, (unsigned long long)ws);
}
