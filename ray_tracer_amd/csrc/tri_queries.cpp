// tri_queries.cpp — see tri_queries.h. Host only: compiled into the library by hipcc and into tests/tri_queries_check.cpp by g++.
#include "tri_queries.h"

#include <vector>

#include "box_queries.h"
#include "point_queries.h"
#include "rt_tri_overlap.h"

std::string check_tris_query(const char* fn, bool sceneUploaded, const RtTriangleBatch* tris, uint32_t k, const void* out, const void* counts) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!tris) return f + ": the batch is NULL";
    if (tris->n == 0) return "";
    if (!tris->corners) return f + ": corners are required";
    if (k > (uint32_t)RT_BOXES_MAX_K) return f + ": k = " + std::to_string(k) + " is above RT_BOXES_MAX_K = " + std::to_string((int)RT_BOXES_MAX_K);
    if (!counts || (!out && k > 0)) return f + ": counts and, with k > 0, the output are required";
    if (tris->n >= (uint32_t)RT_TRIS_MAX_TRIS) return f + ": a batch of " + std::to_string(tris->n) + " triangles does not fit the 30 bits of a slot id";
    return "";
}

TrisShape tris_shape(uint32_t n, uint32_t k, uint32_t threads) {
    const BoxesShape b = boxes_shape(n, k, threads);
    TrisShape s;
    s.blocks = b.blocks;
    s.cornerBytes = (size_t)n * 9 * sizeof(float);
    s.outBytes = b.outBytes;
    s.countBytes = b.countBytes;
    s.listBytes = b.listBytes;
    return s;
}

uint32_t tris_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    const uint32_t stack = boxes_stack(fn, maxLeafDepth, error);
    if (!stack && error) {
        const std::string theirs = "k_boxes_overlap";
        const size_t at = error->find(theirs);
        if (at != std::string::npos) error->replace(at, theirs.size(), "k_tris_overlap");
    }
    return stack;
}

extern "C" {

int rt_tris_exhaustive_host(const RtSceneArrays* s, const RtTriangleBatch* tris, uint32_t k, RtOverlap* out, uint32_t* counts) {
    if (!s || !tris || k > (uint32_t)RT_BOXES_MAX_K) return -1;
    const uint32_t n = tris->n;
    if (n == 0) return 0;
    if (!tris->corners || !counts || (!out && k > 0) || n >= (uint32_t)RT_TRIS_MAX_TRIS) return -1;
    if ((s->sphereCount && !s->spheres) || (s->objectCount && (!s->objects || !s->bvhNodes)) || (s->triangleCount && (!s->triangles || !s->triPoints))) return -1;
    std::vector<TriangleRanges> rangesOf;
    if (!object_triangle_ranges(*s, &rangesOf)) return -1;
    std::vector<bool> identity(s->objectCount);
    for (uint32_t o = 0; o < s->objectCount; o++) identity[o] = matrix_rows_identity(s->objects[o].transformMatrix);
    for (uint32_t i = 0; i < n; i++) {
        const float* pc = tris->corners + (size_t)i * 9;
        const rt_vec3 p = rt_v3(pc[0], pc[1], pc[2]), q = rt_v3(pc[3], pc[4], pc[5]), r = rt_v3(pc[6], pc[7], pc[8]);
        uint32_t list[RT_BOXES_MAX_K * RT_BOX_WORDS], have = 0, count = 0;
        if (rt_tri_valid(p, q, r)) {
            const RtTriQuery tq = rt_tri_prepare(p, q, r);   // rt_tri_triangle's own first step, once per query
            for (uint32_t j = 0; j < s->sphereCount; j++) {
                const Sphere& sp = s->spheres[j];
                if (!rt_sphere_is_surface(sp.radius)) continue;
                if (!rt_tri_sphere(p, q, r, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius)) continue;
                count++;
                have = rt_box_insert(list, 1, k, have, rt_box_sphere_word(j), 0u);
            }
            for (uint32_t o = 0; o < s->objectCount; o++)
                for (const auto& range : rangesOf[o])
                    for (uint32_t t = range.first; t < range.first + range.second; t++) {
                        const Triangle& tr = s->triangles[t];
                        const float *pa = s->triPoints[tr.v0].position, *pb = s->triPoints[tr.v1].position, *pcn = s->triPoints[tr.v2].position;
                        rt_vec3 a = rt_v3(pa[0], pa[1], pa[2]), b = rt_v3(pb[0], pb[1], pb[2]), c = rt_v3(pcn[0], pcn[1], pcn[2]);
                        if (!identity[o]) {   // the world corners, as k_tris_overlap places them
                            const float* m = s->objects[o].transformMatrix;
                            a = rt_xform_point(m, a); b = rt_xform_point(m, b); c = rt_xform_point(m, c);
                        }
                        if (!rt_tri_triangle_prepared(&tq, a, b, c)) continue;
                        count++;
                        have = rt_box_insert(list, 1, k, have, rt_box_triangle_word(o), t);
                    }
        }
        counts[i] = count;
        for (uint32_t e = 0; e < k; e++)
            out[(size_t)i * k + e] = e < have ? rt_box_record(list[e * RT_BOX_WORDS], list[e * RT_BOX_WORDS + 1]) : rt_box_no_member();
    }
    return 0;
}

}  // extern "C"
