// cut_queries.cpp — see cut_queries.h. Host only: compiled into the library by hipcc and into tests/cut_queries_check.cpp by g++.
#include "cut_queries.h"

#include <vector>

#include "point_queries.h"
#include "rt_tri_cut.h"

CutsShape cuts_shape(uint32_t n, uint32_t k, uint32_t threads) {
    const TrisShape t = tris_shape(n, k, threads);
    CutsShape s;
    s.blocks = t.blocks;
    s.cornerBytes = t.cornerBytes;
    s.outBytes = (size_t)n * k * sizeof(RtCut);
    s.countBytes = t.countBytes;
    s.listBytes = t.listBytes;
    return s;
}

uint32_t cuts_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    const uint32_t stack = tris_stack(fn, maxLeafDepth, error);
    if (!stack && error) {
        const std::string theirs = "k_tris_overlap";
        const size_t at = error->find(theirs);
        if (at != std::string::npos) error->replace(at, theirs.size(), "k_tris_cut");
    }
    return stack;
}

extern "C" {

int rt_cuts_exhaustive_host(const RtSceneArrays* s, const RtTriangleBatch* tris, uint32_t k, RtCut* out, uint32_t* counts) {
    if (!s || !tris || k > (uint32_t)RT_BOXES_MAX_K) return -1;
    const uint32_t n = tris->n;
    if (n == 0) return 0;
    if (!tris->corners || !counts || (!out && k > 0) || n >= (uint32_t)RT_TRIS_MAX_TRIS) return -1;
    if ((s->sphereCount && !s->spheres) || (s->objectCount && (!s->objects || !s->bvhNodes)) || (s->triangleCount && (!s->triangles || !s->triPoints))) return -1;
    std::vector<TriangleRanges> rangesOf;
    if (!object_triangle_ranges(*s, &rangesOf)) return -1;
    std::vector<bool> identity(s->objectCount);
    for (uint32_t o = 0; o < s->objectCount; o++) identity[o] = matrix_rows_identity(s->objects[o].transformMatrix);
    // the world corners of triangle t of object o, as k_tris_cut places them
    auto corners = [&](uint32_t o, uint32_t t, rt_vec3* a, rt_vec3* b, rt_vec3* c) {
        const Triangle& tr = s->triangles[t];
        const float *pa = s->triPoints[tr.v0].position, *pb = s->triPoints[tr.v1].position, *pcn = s->triPoints[tr.v2].position;
        *a = rt_v3(pa[0], pa[1], pa[2]); *b = rt_v3(pb[0], pb[1], pb[2]); *c = rt_v3(pcn[0], pcn[1], pcn[2]);
        if (!identity[o]) {
            const float* m = s->objects[o].transformMatrix;
            *a = rt_xform_point(m, *a); *b = rt_xform_point(m, *b); *c = rt_xform_point(m, *c);
        }
    };
    for (uint32_t i = 0; i < n; i++) {
        const float* pc = tris->corners + (size_t)i * 9;
        const rt_vec3 p = rt_v3(pc[0], pc[1], pc[2]), q = rt_v3(pc[3], pc[4], pc[5]), r = rt_v3(pc[6], pc[7], pc[8]);
        uint32_t list[RT_BOXES_MAX_K * RT_BOX_WORDS], have = 0, count = 0;
        const RtTriQuery tq = rt_tri_prepare(p, q, r);   // (of a triangle that is not valid: never used)
        if (rt_tri_valid(p, q, r)) {
            for (uint32_t o = 0; o < s->objectCount; o++)
                for (const auto& range : rangesOf[o])
                    for (uint32_t t = range.first; t < range.first + range.second; t++) {
                        rt_vec3 a, b, c;
                        RtCutSeg seg;
                        corners(o, t, &a, &b, &c);
                        if (!rt_tri_cut_prepared(&tq, a, b, c, &seg)) continue;
                        count++;
                        have = rt_box_insert(list, 1, k, have, rt_box_triangle_word(o), t);
                    }
        }
        counts[i] = count;
        // the list holds keys; a cut is a function of the pair, so the kept ones are computed again, as the kernel does
        for (uint32_t e = 0; e < k; e++) {
            RtCut rec = rt_cut_no_member();
            if (e < have) {
                const uint32_t o = list[e * RT_BOX_WORDS], t = list[e * RT_BOX_WORDS + 1];
                rt_vec3 a, b, c;
                RtCutSeg seg;
                corners(o, t, &a, &b, &c);
                if (rt_tri_cut_prepared(&tq, a, b, c, &seg)) rec = rt_cut_record(&seg, o, t);
            }
            out[(size_t)i * k + e] = rec;
        }
    }
    return 0;
}

}  // extern "C"
