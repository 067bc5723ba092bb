// ray_hits.cpp — see ray_hits.h. Host only: compiled into the library by hipcc and into tests/ray_hits_check.cpp by g++.
#include "ray_hits.h"

#include <cstring>
#include <vector>

#include "point_queries.h"
#include "ray_queries.h"
#include "rt_ray_hits.h"

std::string check_hits_query(const char* fn, bool sceneUploaded, const RtRayBatch* rays, uint32_t k, const void* hits, const void* counts) {
    const std::string f(fn);
    // check_ray_query's first tests on one ray of the batch (the size comes last), the outputs being this function's business
    RtRayBatch one{};
    if (rays) one = RtRayBatch{rays->origins, rays->dirs, rays->tmax, rays->n ? 1u : 0u};
    const std::string first = check_ray_query(fn, sceneUploaded, rays ? &one : nullptr, fn);
    if (!first.empty() || !sceneUploaded || !rays || rays->n == 0) return first;
    if (k > (uint32_t)RT_HITS_MAX_K) return f + ": k = " + std::to_string(k) + " is above RT_HITS_MAX_K = " + std::to_string((int)RT_HITS_MAX_K);
    if (!counts || (!hits && k > 0)) return f + ": counts and, with k > 0, hits are required";
    return check_ray_query(fn, sceneUploaded, rays, counts);
}

HitsShape hits_shape(uint32_t n, uint32_t k, uint32_t threads) {
    HitsShape s;
    s.searchBlocks = (uint32_t)(((uint64_t)n + threads - 1) / threads);
    s.resolveBlocks = (uint32_t)(((uint64_t)n * k + threads - 1) / threads);
    s.vecBytes = (size_t)n * 3 * sizeof(float);
    s.tmaxBytes = (size_t)n * sizeof(float);
    s.hitBytes = sizeof(RtHit) * (size_t)n * k;
    s.countBytes = (size_t)n * sizeof(uint32_t);
    s.listBytes = (size_t)s.searchBlocks * threads * RT_HITS_MAX_K * RT_HITS_WORDS * sizeof(uint32_t);
    return s;
}

uint32_t hits_stack(const char* fn, uint32_t maxLeafDepth, std::string* error) {
    static_assert((int)RT_HITS_STACK == (int)RT_NEAREST_STACK && (int)RT_HITS_STACK_DEEP == (int)RT_NEAREST_STACK_DEEP, "one rule for both stacks");
    const uint32_t stack = nearest_stack(fn, maxLeafDepth, error);
    if (!stack && error) {
        const std::string theirs = "k_nearest_points";
        const size_t at = error->find(theirs);
        if (at != std::string::npos) error->replace(at, theirs.size(), "k_ray_hits");
    }
    return stack;
}

namespace {
// map_red8 (rt_kernels.hip.h) on the host's texture table
uint32_t red8(const RtTexture& t, bool clampEdge, float u, float v, bool dx, bool dy) {
    uint32_t x = rt_tex_index(u, t.width, clampEdge), y = rt_tex_index(1.f - v, t.height, clampEdge);
    if (dx) x = rt_tex_next(x, t.width, clampEdge);
    if (dy) y = rt_tex_next(y, t.height, clampEdge);
    return t.rgba8[((size_t)y * t.width + x) * 4];
}

struct Walk {
    const RtSceneArrays* s;
    const RtTexture* tex;
    uint32_t nTex;
    std::vector<float> inv;   // 16 floats per object: rt_mat4_inverse of its matrix

    rt_vec3 corner(uint32_t point) const {
        const float* p = s->triPoints[point].position;
        return rt_v3(p[0], p[1], p[2]);
    }
    // hit.uv (raytrace.comp:249-256) and the uv differences of the corners: hit_uv of the kernels
    void hit_uv(const Triangle& tr, float bu, float bv, float bw, float* u, float* v, float* d) const {
        const TrianglePoint &p0 = s->triPoints[tr.v0], &p1 = s->triPoints[tr.v1], &p2 = s->triPoints[tr.v2];
        const float u0 = p0.position[3], v0 = p0.normal[3], u1 = p1.position[3], v1 = p1.normal[3], u2 = p2.position[3], v2 = p2.normal[3];
        *u = (bw * u0 + bu * u1) + bv * u2;
        *v = (bw * v0 + bu * v1) + bv * v2;
        if ((u0 == u1 && v0 == v1) || (u1 == u2 && v1 == v2) || (u2 == u0 && v2 == v0)) { *u = 0.5f; *v = 0.5f; }
        d[0] = u1 - u0; d[1] = v1 - v0; d[2] = u2 - u0; d[3] = v2 - v0;
    }
    bool clamp_edge(uint32_t obj) const { return (s->objects[obj].samplerIndex & 0xffffu) == 1u; }
    // alpha_cut of the kernels: the object's material binds an alpha map and the texel's red byte is below the cut
    bool alpha_cut(uint32_t obj, const Triangle& tr, const RtHitsTri& h) const {
        const int32_t slot = s->materials[s->objects[obj].materialIndex].alphaIndex;
        if (slot < 0 || (uint32_t)slot >= nTex) return false;
        float u, v, d[4];
        hit_uv(tr, h.u, h.v, h.w, &u, &v, d);
        return red8(tex[slot], s->objects[obj].samplerIndex == 1u, u, v, false, false) < RT_ALPHA_CUT_BYTE;
    }
    void object_ray(uint32_t obj, rt_vec3 ro, rt_vec3 rd, rt_vec3* tro, rt_vec3* trd) const {
        const float* m = inv.data() + 16 * (size_t)obj;
        *trd = rt_xform_dir(m, rd);
        *tro = rt_xform_point(m, ro);
    }

    // the RtHit of a list entry: what k_query_hits and reconstruct_hit<true> build for the primitive (k_ray_hits_resolve)
    RtHit record(rt_vec3 ro, rt_vec3 rd, float dst, uint32_t prim, uint32_t tri) const {
        RtHit r;
        memset(&r, 0, sizeof r);
        r.dst = dst;
        r.didHit = 1;
        rt_vec3 p, n;
        if (rt_hits_is_sphere(prim)) {
            const uint32_t i = rt_hits_sphere_index(prim);
            const Sphere& sp = s->spheres[i];
            const rt_vec3 c = rt_v3(sp.position[0], sp.position[1], sp.position[2]);
            const bool front = !rt_hits_sphere_exit(prim);
            p = rt_add(ro, rt_scale(rd, dst));
            n = rt_scale(rt_normalize(rt_sub(p, c)), front ? 1.f : -1.f);
            r.isSphere = 1; r.objectHitIndex = i; r.materialIndex = sp.materialIndex; r.frontFace = front ? 1u : 0u;
        } else {
            const RenderObject& o = s->objects[prim];
            const Triangle& tr = s->triangles[tri];
            rt_vec3 tro, trd;
            object_ray(prim, ro, rd, &tro, &trd);
            const rt_vec3 a = corner(tr.v0), b = corner(tr.v1), c = corner(tr.v2);
            const RtHitsTri h = rt_hits_triangle(tro, trd, a, b, c, tr.frontOnly != 0u);
            const float *na = s->triPoints[tr.v0].normal, *nb = s->triPoints[tr.v1].normal, *nc = s->triPoints[tr.v2].normal;
            rt_vec3 ni = rt_add(rt_add(rt_scale(rt_v3(na[0], na[1], na[2]), h.w), rt_scale(rt_v3(nb[0], nb[1], nb[2]), h.u)), rt_scale(rt_v3(nc[0], nc[1], nc[2]), h.v));
            const int32_t bump = s->materials[o.materialIndex].bumpIndex;
            if (bump >= 0 && (uint32_t)bump < nTex) {
                float u, v, d[4];
                hit_uv(tr, h.u, h.v, h.w, &u, &v, d);
                const bool ce = clamp_edge(prim);
                const float h0 = rt_srgb8_to_linear(red8(tex[bump], ce, u, v, false, false));
                const float hx = rt_srgb8_to_linear(red8(tex[bump], ce, u, v, true, false)) - h0;
                const float hy = rt_srgb8_to_linear(red8(tex[bump], ce, u, v, false, true)) - h0;
                ni = rt_bump_normal(ni, rt_sub(b, a), rt_sub(c, a), d[0], d[1], d[2], d[3], hx, hy);
            }
            ni = rt_scale(ni, h.frontFace ? 1.f : -1.f);
            const rt_vec3 op = rt_add(tro, rt_scale(trd, h.dst));
            n = rt_normalize(rt_xform_dir(o.transformMatrix, ni));
            p = rt_xform_point(o.transformMatrix, op);
            r.objectHitIndex = prim; r.triHitIndex = tri; r.materialIndex = o.materialIndex; r.frontFace = h.frontFace ? 1u : 0u;
        }
        r.hitPoint[0] = p.x; r.hitPoint[1] = p.y; r.hitPoint[2] = p.z;
        r.normal[0] = n.x; r.normal[1] = n.y; r.normal[2] = n.z;
        return r;
    }
};

// every index the walk follows stays inside its array
bool arrays_in_range(const RtSceneArrays& s, uint32_t sphereCount, uint32_t objectCount) {
    if (sphereCount > s.sphereCount || objectCount > s.objectCount) return false;
    if ((sphereCount && !s.spheres) || (objectCount && (!s.objects || !s.bvhNodes || !s.materials))) return false;
    if (s.triangleCount >= (1u << 30) || (s.triangleCount && (!s.triangles || !s.triPoints))) return false;
    for (uint32_t i = 0; i < objectCount; i++)
        if (s.objects[i].bvhIndex >= s.bvhNodeCount || s.objects[i].materialIndex >= s.materialCount) return false;
    for (uint32_t i = 0; i < s.bvhNodeCount; i++) {
        const BVHNode& b = s.bvhNodes[i];
        if (b.triCount ? (uint64_t)b.index + b.triCount > s.triangleCount : (uint64_t)b.index + 1 >= s.bvhNodeCount) return false;
    }
    for (uint32_t t = 0; t < s.triangleCount; t++)
        if (s.triangles[t].v0 >= s.triPointCount || s.triangles[t].v1 >= s.triPointCount || s.triangles[t].v2 >= s.triPointCount) return false;
    return true;
}
}  // namespace

extern "C" {

int rt_hits_walk_host(const RtSceneArrays* s, uint32_t sphereCount, uint32_t objectCount, const RtTexture* textures, uint32_t nTextures,
                      const RtRayBatch* rays, uint32_t k, RtHit* hits, uint32_t* counts) {
    if (!s || !rays || k > (uint32_t)RT_HITS_MAX_K) return -1;
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    if (!rays->origins || !rays->dirs || !counts || (!hits && k > 0) || n >= (1u << 30)) return -1;
    if (nTextures && !textures) return -1;
    for (uint32_t t = 0; t < nTextures; t++)
        if (!textures[t].rgba8 || !textures[t].width || !textures[t].height) return -1;
    if (!arrays_in_range(*s, sphereCount, objectCount)) return -1;

    Walk w{s, textures, nTextures, std::vector<float>((size_t)objectCount * 16)};
    for (uint32_t i = 0; i < objectCount; i++) rt_mat4_inverse(s->objects[i].transformMatrix, w.inv.data() + 16 * (size_t)i);

    std::vector<uint32_t> stack;
    for (uint32_t i = 0; i < n; i++) {
        const rt_vec3 ro = rt_v3(rays->origins[(size_t)i * 3], rays->origins[(size_t)i * 3 + 1], rays->origins[(size_t)i * 3 + 2]);
        const rt_vec3 rd = rt_v3(rays->dirs[(size_t)i * 3], rays->dirs[(size_t)i * 3 + 1], rays->dirs[(size_t)i * 3 + 2]);
        bool search;
        const float T = rt_hits_start(rays->tmax != nullptr, rays->tmax ? rays->tmax[i] : 0.f, &search);
        uint32_t list[RT_HITS_MAX_K * RT_HITS_WORDS], have = 0, count = 0;
        if (search) {
            for (uint32_t j = 0; j < sphereCount; j++) {
                const Sphere& sp = s->spheres[j];
                float tEntry, tExit;
                if (!rt_hits_sphere_roots(rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius, ro, rd, &tEntry, &tExit)) continue;
                if (rt_hits_accepts(tEntry, T)) { count++; have = rt_hits_insert(list, 1, k, have, tEntry, rt_hits_sphere_word(j, false), 0); }
                if (rt_hits_accepts(tExit, T)) { count++; have = rt_hits_insert(list, 1, k, have, tExit, rt_hits_sphere_word(j, true), 0); }
            }
            for (uint32_t obj = 0; obj < objectCount; obj++) {
                rt_vec3 tro, trd;
                w.object_ray(obj, ro, rd, &tro, &trd);
                const rt_vec3 inv = rt_v3(1.f / trd.x, 1.f / trd.y, 1.f / trd.z);
                stack.assign(1, s->objects[obj].bvhIndex);   // the root, untested
                size_t visited = 0;
                while (!stack.empty()) {
                    if (++visited > (size_t)s->bvhNodeCount) return -1;   // not a tree
                    const BVHNode& b = s->bvhNodes[stack.back()];
                    stack.pop_back();
                    if (b.triCount) {
                        for (uint32_t t = b.index; t < b.index + b.triCount; t++) {
                            const Triangle& tr = s->triangles[t];
                            const RtHitsTri h = rt_hits_triangle(tro, trd, w.corner(tr.v0), w.corner(tr.v1), w.corner(tr.v2), tr.frontOnly != 0u);
                            if (!h.didHit || !(h.dst < T) || w.alpha_cut(obj, tr, h)) continue;
                            count++;
                            have = rt_hits_insert(list, 1, k, have, h.dst, obj, t);
                        }
                        continue;
                    }
                    for (uint32_t c = b.index; c < b.index + 2; c++) {
                        const BVHNode& ch = s->bvhNodes[c];
                        const float d = rt_hits_box(rt_v3(ch.boundsX[0], ch.boundsY[0], ch.boundsZ[0]), rt_v3(ch.boundsX[1], ch.boundsY[1], ch.boundsZ[1]), tro, inv);
                        if (d < T) stack.push_back(c);
                    }
                }
            }
        }
        counts[i] = count;
        for (uint32_t e = 0; e < k; e++) {
            RtHit& out = hits[(size_t)i * k + e];
            if (e < have) {
                out = w.record(ro, rd, rt_u2f(list[e * RT_HITS_WORDS]), list[e * RT_HITS_WORDS + 1], list[e * RT_HITS_WORDS + 2]);
            } else {
                memset(&out, 0, sizeof out);
                out.dst = RT_MISS_DST;
            }
        }
    }
    return 0;
}

}  // extern "C"
