// point_within.cpp — see point_within.h. Host only: compiled into the library by hipcc and into tests/point_within_check.cpp by g++.
#include "point_within.h"

#include <vector>

#include "point_queries.h"
#include "rt_point_within.h"

std::string check_within_query(const char* fn, bool sceneUploaded, const RtPointBatch* points, uint32_t k, const void* out, const void* counts) {
    const std::string f(fn);
    // check_point_query's first tests on one point of the batch (the size comes last), the outputs being this function's business
    RtPointBatch one{};
    if (points) one = RtPointBatch{points->points, points->maxDist, points->n ? 1u : 0u};
    const std::string first = check_point_query(fn, sceneUploaded, points ? &one : nullptr, fn);
    if (!first.empty() || !sceneUploaded || !points || points->n == 0) return first;
    if (k > (uint32_t)RT_WITHIN_MAX_K) return f + ": k = " + std::to_string(k) + " is above RT_WITHIN_MAX_K = " + std::to_string((int)RT_WITHIN_MAX_K);
    if (!counts || (!out && k > 0)) return f + ": counts and, with k > 0, the output are required";
    return check_point_query(fn, sceneUploaded, points, counts);
}

WithinShape within_shape(uint32_t n, uint32_t k, uint32_t threads) {
    WithinShape s;
    s.searchBlocks = (uint32_t)(((uint64_t)n + threads - 1) / threads);
    s.resolveBlocks = (uint32_t)(((uint64_t)n * k + threads - 1) / threads);
    s.pointBytes = (size_t)n * 3 * sizeof(float);
    s.limitBytes = (size_t)n * sizeof(float);
    s.outBytes = sizeof(RtNearest) * (size_t)n * k;
    s.countBytes = (size_t)n * sizeof(uint32_t);
    s.listBytes = (size_t)s.searchBlocks * threads * RT_WITHIN_MAX_K * RT_HITS_WORDS * sizeof(uint32_t);
    return s;
}

uint32_t within_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    static_assert((int)RT_WITHIN_STACK == (int)RT_NEAREST_STACK && (int)RT_WITHIN_STACK_DEEP == (int)RT_NEAREST_STACK_DEEP, "one rule for both stacks");
    const uint32_t stack = nearest_stack(fn, maxLeafDepth, error);
    if (!stack && error) {
        const std::string theirs = "k_nearest_points";
        const size_t at = error->find(theirs);
        if (at != std::string::npos) error->replace(at, theirs.size(), "k_points_within");
    }
    return stack;
}

extern "C" {

int rt_within_exhaustive_host(const RtSceneArrays* s, const RtPointBatch* points, uint32_t k, RtNearest* out, uint32_t* counts) {
    if (!s || !points || k > (uint32_t)RT_WITHIN_MAX_K) return -1;
    const uint32_t n = points->n;
    if (n == 0) return 0;
    if (!points->points || !counts || (!out && k > 0) || n >= (uint32_t)RT_NEAREST_MAX_POINTS) return -1;
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
        const rt_vec3 q = rt_v3(points->points[(size_t)i * 3], points->points[(size_t)i * 3 + 1], points->points[(size_t)i * 3 + 2]);
        bool search;
        const float R2 = rt_nearest_start(points->maxDist != nullptr, points->maxDist ? points->maxDist[i] : 0.f, &search);
        uint32_t list[RT_WITHIN_MAX_K * RT_HITS_WORDS], have = 0, count = 0;
        if (search) {
            for (uint32_t j = 0; j < s->sphereCount; j++) {
                const Sphere& sp = s->spheres[j];
                if (!rt_sphere_is_surface(sp.radius)) continue;
                rt_vec3 p;
                const float d2 = rt_point_sphere(q, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius, &p);
                if (!rt_within_member(d2, R2)) continue;
                count++;
                have = rt_hits_insert(list, 1, k, have, d2, rt_within_sphere_word(j), 0u);
            }
            for (uint32_t o = 0; o < s->objectCount; o++)
                for (const auto& range : rangesOf[o])
                    for (uint32_t t = range.first; t < range.first + range.second; t++) {
                        rt_vec3 a, b, c;
                        corners(o, t, &a, &b, &c);
                        float u, v;
                        const float d2 = rt_point_triangle(q, a, b, c, &u, &v);
                        if (!rt_within_member(d2, R2)) continue;
                        count++;
                        have = rt_hits_insert(list, 1, k, have, d2, rt_within_triangle_word(o), t);
                    }
        }
        counts[i] = count;
        for (uint32_t e = 0; e < k; e++) {
            RtNearest& r = out[(size_t)i * k + e];
            if (e >= have) { r = rt_within_not_found(); continue; }
            const float d2 = rt_u2f(list[e * RT_HITS_WORDS]);
            const uint32_t prim = list[e * RT_HITS_WORDS + 1], tri = list[e * RT_HITS_WORDS + 2];
            if (rt_hits_is_sphere(prim)) {
                const uint32_t j = rt_hits_sphere_index(prim);
                const Sphere& sp = s->spheres[j];
                r = rt_within_sphere_record(q, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius, j, d2);
            } else {
                rt_vec3 a, b, c;
                corners(prim, tri, &a, &b, &c);
                r = rt_within_triangle_record(q, a, b, c, prim, tri, d2);
            }
        }
    }
    return 0;
}

}  // extern "C"
