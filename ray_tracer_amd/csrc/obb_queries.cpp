// obb_queries.cpp — see obb_queries.h. Host only: compiled into the library by hipcc and into tests/obb_queries_check.cpp by g++.
#include "obb_queries.h"

#include <vector>

#include "point_queries.h"
#include "rt_obb_overlap.h"

std::string check_obbs_query(const char* fn, bool sceneUploaded, const RtObbBatch* batch, uint32_t k, const void* out, const void* counts) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!batch) return f + ": the batch is NULL";
    if (batch->n == 0) return "";
    if (!batch->frames || !batch->lo || !batch->hi) return f + ": frames, lo and hi are required";
    if (k > (uint32_t)RT_BOXES_MAX_K) return f + ": k = " + std::to_string(k) + " is above RT_BOXES_MAX_K = " + std::to_string((int)RT_BOXES_MAX_K);
    if (batch->sharedFrame > 1u) return f + ": sharedFrame = " + std::to_string(batch->sharedFrame) + " is neither 0 nor 1";
    if (!counts || (!out && k > 0)) return f + ": counts and, with k > 0, the output are required";
    if (batch->n >= (uint32_t)RT_BOXES_MAX_BOXES) return f + ": a batch of " + std::to_string(batch->n) + " boxes does not fit the 30 bits of a slot id";
    return "";
}

ObbShape obbs_shape(uint32_t n, uint32_t k, bool sharedFrame, uint32_t threads) {
    const BoxesShape b = boxes_shape(n, k, threads);
    ObbShape s;
    s.blocks = b.blocks;
    s.frameBytes = n == 0 ? 0 : (sharedFrame ? 1 : (size_t)n) * RT_OBB_FRAME_FLOATS * sizeof(float);
    s.cornerBytes = b.cornerBytes;
    s.outBytes = b.outBytes;
    s.countBytes = b.countBytes;
    s.listBytes = b.listBytes;
    return s;
}

uint32_t obbs_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    const uint32_t stack = boxes_stack(fn, maxLeafDepth, error);
    if (!stack && error) {
        const std::string theirs = "k_boxes_overlap";
        const size_t at = error->find(theirs);
        if (at != std::string::npos) error->replace(at, theirs.size(), "k_obbs_overlap");
    }
    return stack;
}

extern "C" {

int rt_object_frames_host(const RtSceneArrays* s, const uint32_t* objects, uint32_t n, float* frames) {
    if (!s || (n && (!objects || !frames || !s->objects))) return -1;
    for (uint32_t i = 0; i < n; i++)
        if (objects[i] >= s->objectCount) return -1;
    for (uint32_t i = 0; i < n; i++) rt_mat4_inverse(s->objects[objects[i]].transformMatrix, frames + (size_t)i * RT_OBB_FRAME_FLOATS);
    return 0;
}

int rt_obbs_exhaustive_host(const RtSceneArrays* s, const RtObbBatch* batch, uint32_t k, RtOverlap* out, uint32_t* counts) {
    if (!s || !batch || k > (uint32_t)RT_BOXES_MAX_K) return -1;
    const uint32_t n = batch->n;
    if (n == 0) return 0;
    if (!batch->frames || !batch->lo || !batch->hi || batch->sharedFrame > 1u || !counts || (!out && k > 0) || n >= (uint32_t)RT_BOXES_MAX_BOXES) return -1;
    if ((s->sphereCount && !s->spheres) || (s->objectCount && (!s->objects || !s->bvhNodes)) || (s->triangleCount && (!s->triangles || !s->triPoints))) return -1;
    std::vector<TriangleRanges> rangesOf;
    if (!object_triangle_ranges(*s, &rangesOf)) return -1;
    std::vector<bool> identity(s->objectCount);
    for (uint32_t o = 0; o < s->objectCount; o++) identity[o] = matrix_rows_identity(s->objects[o].transformMatrix);
    for (uint32_t i = 0; i < n; i++) {
        const float *pl = batch->lo + (size_t)i * 3, *ph = batch->hi + (size_t)i * 3;
        const rt_vec3 lo = rt_v3(pl[0], pl[1], pl[2]), hi = rt_v3(ph[0], ph[1], ph[2]);
        const RtObbFrame f = rt_obb_frame(batch->frames + (batch->sharedFrame ? 0 : (size_t)i * RT_OBB_FRAME_FLOATS));
        uint32_t list[RT_BOXES_MAX_K * RT_BOX_WORDS], have = 0, count = 0;
        if (rt_obb_valid(f, lo, hi)) {
            const float scale = rt_obb_scale(f);
            for (uint32_t j = 0; j < s->sphereCount; j++) {
                const Sphere& sp = s->spheres[j];
                if (!rt_sphere_is_surface(sp.radius)) continue;
                if (!rt_obb_sphere(f, scale, lo, hi, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius)) continue;
                count++;
                have = rt_box_insert(list, 1, k, have, rt_box_sphere_word(j), 0u);
            }
            for (uint32_t o = 0; o < s->objectCount; o++)
                for (const auto& range : rangesOf[o])
                    for (uint32_t t = range.first; t < range.first + range.second; t++) {
                        const Triangle& tr = s->triangles[t];
                        const float *pa = s->triPoints[tr.v0].position, *pb = s->triPoints[tr.v1].position, *pc = s->triPoints[tr.v2].position;
                        rt_vec3 a = rt_v3(pa[0], pa[1], pa[2]), b = rt_v3(pb[0], pb[1], pb[2]), c = rt_v3(pc[0], pc[1], pc[2]);
                        if (!identity[o]) {   // the world corners, as k_obbs_overlap places them
                            const float* m = s->objects[o].transformMatrix;
                            a = rt_xform_point(m, a); b = rt_xform_point(m, b); c = rt_xform_point(m, c);
                        }
                        if (!rt_obb_triangle(f, lo, hi, a, b, c)) continue;
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
