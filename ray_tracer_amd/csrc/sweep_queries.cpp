// sweep_queries.cpp — see sweep_queries.h. Host only: compiled into the library by hipcc and into tests/sweep_check.cpp by g++.
#include "sweep_queries.h"

#include <vector>

#include "point_queries.h"
#include "rt_sweep.h"

std::string check_sweep_query(const char* fn, bool sceneUploaded, const RtSweepBatch* batch, const void* out) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!batch) return f + ": the batch is NULL";
    if (batch->n == 0) return "";
    if (!batch->origins || !batch->dirs || !batch->radius || !out) return f + ": origins, dirs, radius and the output are required";
    if (batch->n >= (uint32_t)RT_SWEEP_MAX_RAYS) return f + ": a batch of " + std::to_string(batch->n) + " rays does not fit the 30 bits of a slot id";
    return "";
}

SweepShape sweep_shape(uint32_t n, uint32_t threads) {
    SweepShape s;
    s.blocks = (uint32_t)(((uint64_t)n + threads - 1) / threads);
    s.vecBytes = (size_t)n * 3 * sizeof(float);
    s.scalarBytes = (size_t)n * sizeof(float);
    s.outBytes = (size_t)n * sizeof(RtSweep);
    return s;
}

uint32_t sweep_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    static_assert((int)RT_SWEEP_STACK == (int)RT_NEAREST_STACK && (int)RT_SWEEP_STACK_DEEP == (int)RT_NEAREST_STACK_DEEP, "one rule for both stacks");
    const uint32_t stack = nearest_stack(fn, maxLeafDepth, error);
    if (!stack && error) {
        const std::string theirs = "k_nearest_points";
        const size_t at = error->find(theirs);
        if (at != std::string::npos) error->replace(at, theirs.size(), "k_sweep_spheres");
    }
    return stack;
}

extern "C" {

int rt_sweep_exhaustive_host(const RtSceneArrays* s, const RtSweepBatch* batch, RtSweep* out) {
    static_assert(sizeof(RtSweep) == 64, "four 16-byte stores");
    if (!s || !batch) return -1;
    const uint32_t n = batch->n;
    if (n == 0) return 0;
    if (!batch->origins || !batch->dirs || !batch->radius || !out || n >= (uint32_t)RT_SWEEP_MAX_RAYS) return -1;
    if ((s->sphereCount && !s->spheres) || (s->objectCount && (!s->objects || !s->bvhNodes)) || (s->triangleCount && (!s->triangles || !s->triPoints))) return -1;
    std::vector<TriangleRanges> rangesOf;
    if (!object_triangle_ranges(*s, &rangesOf)) return -1;
    std::vector<bool> identity(s->objectCount);
    for (uint32_t o = 0; o < s->objectCount; o++) identity[o] = matrix_rows_identity(s->objects[o].transformMatrix);
    // the world corners of triangle t under object o, as k_nearest_points places them
    auto corners = [&](uint32_t o, uint32_t t, rt_vec3* a, rt_vec3* b, rt_vec3* c) {
        const Triangle& tr = s->triangles[t];
        const float *pa = s->triPoints[tr.v0].position, *pb = s->triPoints[tr.v1].position, *pc = s->triPoints[tr.v2].position;
        *a = rt_v3(pa[0], pa[1], pa[2]); *b = rt_v3(pb[0], pb[1], pb[2]); *c = rt_v3(pc[0], pc[1], pc[2]);
        if (!identity[o]) {
            const float* m = s->objects[o].transformMatrix;
            *a = rt_xform_point(m, *a); *b = rt_xform_point(m, *b); *c = rt_xform_point(m, *c);
        }
    };
    for (uint32_t i = 0; i < n; i++) {
        const size_t r = (size_t)i * 3;
        const rt_vec3 o = rt_v3(batch->origins[r], batch->origins[r + 1], batch->origins[r + 2]);
        const rt_vec3 d = rt_v3(batch->dirs[r], batch->dirs[r + 1], batch->dirs[r + 2]);
        const float R = batch->radius[i], dd = rt_dot(d, d);
        bool search;
        const float T = rt_sweep_start(d, R, batch->tmax != nullptr, batch->tmax ? batch->tmax[i] : 0.f, &search);
        float best = T;
        uint32_t bestPrim = RT_HITS_EMPTY, bestTri = 0;
        if (search) {
            for (uint32_t j = 0; j < s->sphereCount; j++) {
                const Sphere& sp = s->spheres[j];
                if (!rt_sphere_is_surface(sp.radius)) continue;
                float t, d2;
                if (!rt_sweep_sphere(o, d, dd, R, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius, &t, &d2)) continue;
                const uint32_t word = rt_hits_sphere_word(j, false);
                if (rt_sweep_replaces(t, word, 0u, T, best, bestPrim, bestTri)) { best = t; bestPrim = word; bestTri = 0; }
            }
            for (uint32_t k = 0; k < s->objectCount; k++)
                for (const auto& range : rangesOf[k])
                    for (uint32_t tr = range.first; tr < range.first + range.second; tr++) {
                        rt_vec3 a, b, c;
                        corners(k, tr, &a, &b, &c);
                        float t, d2, u, v;
                        if (!rt_sweep_triangle(o, d, dd, R, a, b, c, &t, &d2, &u, &v)) continue;
                        if (rt_sweep_replaces(t, k, tr, T, best, bestPrim, bestTri)) { best = t; bestPrim = k; bestTri = tr; }
                    }
        }
        if (bestPrim == RT_HITS_EMPTY) { out[i] = rt_sweep_not_found(); continue; }
        if (rt_hits_is_sphere(bestPrim)) {
            const uint32_t j = rt_hits_sphere_index(bestPrim);
            const Sphere& sp = s->spheres[j];
            out[i] = rt_sweep_sphere_record(o, d, best, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius, j);
        } else {
            rt_vec3 a, b, c;
            corners(bestPrim, bestTri, &a, &b, &c);
            out[i] = rt_sweep_triangle_record(o, d, best, a, b, c, bestPrim, bestTri);
        }
    }
    return 0;
}

}  // extern "C"
