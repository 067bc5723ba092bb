// scene_layout.cpp — the device scene tables derived on the host (scene_layout.h). Host only: plain arithmetic on the ABI structs.

#include "scene_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>

#include "rt_det_math.h"

namespace {

float4 with_w(float x, float y, float z, uint32_t w) {
    float4 v = make_float4(x, y, z, 0.f);
    memcpy(&v.w, &w, 4);
    return v;
}

// rows 0..2 of a column-major mat4
void rows_of(const float* m, float4* out) {
    for (int r = 0; r < 3; r++) out[r] = make_float4(m[0 + r], m[4 + r], m[8 + r], m[12 + r]);
}

bool rows_are_identity(const float4* rows) {
    static const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    bool is = true;
    for (int r = 0; r < 3; r++) {
        const float q[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
        for (int k = 0; k < 4; k++) is = is && (q[k] == ident[r * 4 + k]);
    }
    return is;
}

template <typename L> L refused(const char* message) {
    L l;
    l.error = message;
    return l;
}

}  // namespace

MeshLayout layout_meshes(const RtSceneArrays& s) {
    MeshLayout l;
    const auto fail = refused<MeshLayout>;
    const uint32_t nNodes = s.bvhNodeCount, nTris = s.triangleCount;

    // ---- mesh segmentation: every distinct object.bvhIndex starts a mesh
    std::vector<uint32_t> roots;
    for (uint32_t i = 0; i < s.objectCount; i++) {
        if (s.objects[i].bvhIndex >= nNodes) return fail("object.bvhIndex out of range");
        roots.push_back(s.objects[i].bvhIndex);
    }
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());

    // ---- device node numbering: shift each mesh so its child pairs (which
    // follow the root in twos) start on an even index = 64-byte boundary
    // The child pairs of the top levels of every mesh come first (breadth first over all roots, level by level, at most
    // RT_HOT_PAIRS of them): k_trace_pw<HOT> keeps exactly those in LDS (DevScene::hotNodes).
    l.nodeRemap.assign(nNodes, 0xffffffffu);
    {
        std::vector<uint32_t> level = roots, next;
        uint32_t hot = 0;
        for (int depth = 0; depth < 8 && !level.empty() && hot < RT_HOT_PAIRS; depth++) {
            next.clear();
            for (uint32_t nidx : level) {
                const BVHNode& b = s.bvhNodes[nidx];
                if (b.triCount != 0 || hot >= RT_HOT_PAIRS) continue;
                if (b.index + 1 >= nNodes) return fail("BVH child index out of range");
                if (l.nodeRemap[b.index] != 0xffffffffu) continue;  // (a malformed BVH that shares children)
                l.nodeRemap[b.index] = 2 * hot;
                l.nodeRemap[b.index + 1] = 2 * hot + 1;
                hot++;
                next.push_back(b.index);
                next.push_back(b.index + 1);
            }
            level.swap(next);
        }
        l.hotNodes = 2 * hot;
        uint32_t pos = 2 * hot;
        size_t r = 0;
        for (uint32_t nidx = 0; nidx < nNodes; nidx++) {
            const bool isRoot = r < roots.size() && roots[r] == nidx;
            if (isRoot) r++;
            if (l.nodeRemap[nidx] != 0xffffffffu) continue;  // a hot pair's node
            if (isRoot && (pos & 1u) == 0u) pos++;             // root on an odd slot: the pairs that follow it in twos start even
            l.nodeRemap[nidx] = pos++;
        }
        l.nodeCount = pos;
    }
    const uint32_t devCount = l.nodeCount;

    l.nodes.assign((size_t)std::max(devCount, 2u) * 2, make_float4(0.f, 0.f, 0.f, 0.f));
    l.leafFirst.assign(std::max(devCount, 1u), 0u);
    auto node_word = [&](uint32_t nidx) -> uint32_t {
        const BVHNode& b = s.bvhNodes[nidx];
        if (b.triCount == 0) return l.nodeRemap[b.index];
        if (b.triCount <= 7u && b.index + b.triCount <= 0x0ffffff0u) return RT_LEAF_BIT | (b.triCount << RT_LEAF_CNT_SHIFT) | b.index;
        return RT_LEAF_BIT | l.nodeRemap[nidx];
    };
    if (devCount > 0x0ffffff0u) return fail("BVH too large (node index needs more than 28 bits)");
    for (uint32_t nidx = 0; nidx < nNodes; nidx++) {
        const BVHNode& b = s.bvhNodes[nidx];
        if (b.triCount == 0) {
            if (b.index + 1 >= nNodes) return fail("BVH child index out of range");
            if (l.nodeRemap[b.index] & 1u) return fail("internal: child pair not 64-byte aligned (BVH not built in pairs)");
        } else if ((uint64_t)b.index + b.triCount > nTris) {
            return fail("BVH leaf triangle range out of bounds");
        }
        l.nodes[2 * (size_t)l.nodeRemap[nidx]] = with_w(b.boundsX[0], b.boundsY[0], b.boundsZ[0], node_word(nidx));
        l.nodes[2 * (size_t)l.nodeRemap[nidx] + 1] = with_w(b.boundsX[1], b.boundsY[1], b.boundsZ[1], b.triCount);
        l.leafFirst[l.nodeRemap[nidx]] = b.triCount ? b.index : 0u;
    }

    l.nodesPk.assign(l.nodes.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t p = 0; p + 1 < (size_t)devCount; p += 2) {
        const float4 lo1 = l.nodes[2 * p], hi1 = l.nodes[2 * p + 1], lo2 = l.nodes[2 * p + 2], hi2 = l.nodes[2 * p + 3];
        l.nodesPk[2 * p] = make_float4(lo1.x, lo1.y, hi1.x, hi1.y);
        l.nodesPk[2 * p + 1] = make_float4(lo2.x, lo2.y, hi2.x, hi2.y);
        l.nodesPk[2 * p + 2] = make_float4(lo1.z, hi1.z, lo2.z, hi2.z);
        l.nodesPk[2 * p + 3] = make_float4(lo1.w, lo2.w, 0.f, 0.f);
    }

    // ---- per mesh: its root, its triangle range, its deepest leaf (which decides the LDS stack size)
    l.rootOf.assign(nNodes, RootInfo{0xffffffffu, 0, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0u, 0u});
    std::vector<std::pair<uint32_t, uint32_t>> st;
    for (uint32_t root : roots) {
        const BVHNode& rb = s.bvhNodes[root];
        l.rootOf[root] = RootInfo{node_word(root), rb.triCount, {rb.boundsX[0], rb.boundsY[0], rb.boundsZ[0]}, {rb.boundsX[1], rb.boundsY[1], rb.boundsZ[1]}, 0u, 0u};
        st.clear();
        st.emplace_back(root, 0u);
        size_t visited = 0;
        uint64_t triLo = ~0ull, triHi = 0, triSum = 0;  // the mesh's triangles: the leaves' ranges, one contiguous run as the builder leaves them
        while (!st.empty()) {
            auto [nidx, d] = st.back();
            st.pop_back();
            if (++visited > (size_t)nNodes + 1) return fail("BVH has a cycle");
            const BVHNode& b = s.bvhNodes[nidx];
            if (b.triCount) {
                l.maxLeafDepth = std::max(l.maxLeafDepth, d);
                triLo = std::min<uint64_t>(triLo, b.index); triHi = std::max<uint64_t>(triHi, (uint64_t)b.index + b.triCount); triSum += b.triCount;
                continue;
            }
            st.emplace_back(b.index, d + 1);
            st.emplace_back(b.index + 1, d + 1);
        }
        l.rootOf[root].triFirst = (uint32_t)triLo;
        l.rootOf[root].triTotal = (triSum == triHi - triLo) ? (uint32_t)triSum : 0xffffffffu;
    }
    if (l.maxLeafDepth > 64) return fail("BVH deeper than 64 levels (the reference's builder caps at 64)");

    // ---- triangles: positions hot, normals and uvs cold, all in the reference's order
    // (TrianglePoint: u in position.w, v in normal.w, src/vk_engine.h:64-67)
    l.triPos.resize((size_t)std::max(nTris, 1u) * 3);
    l.triNrm.resize((size_t)std::max(nTris, 1u) * 3);
    l.triUV.assign((size_t)std::max(nTris, 1u) * 2, make_float4(0.f, 0.f, 0.f, 0.f));
    for (uint32_t t = 0; t < nTris; t++) {
        const Triangle& tr = s.triangles[t];
        const uint32_t vi[3] = {tr.v0, tr.v1, tr.v2};
        for (int k = 0; k < 3; k++) {
            if (vi[k] >= s.triPointCount) return fail("triangle point index out of range");
            const TrianglePoint& p = s.triPoints[vi[k]];
            l.triPos[3 * (size_t)t + k] = with_w(p.position[0], p.position[1], p.position[2], (k == 0 && tr.frontOnly) ? 1u : 0u);
            l.triNrm[3 * (size_t)t + k] = make_float4(p.normal[0], p.normal[1], p.normal[2], 0.f);
        }
        const TrianglePoint &p0 = s.triPoints[tr.v0], &p1 = s.triPoints[tr.v1], &p2 = s.triPoints[tr.v2];
        l.triUV[2 * (size_t)t] = make_float4(p0.position[3], p0.normal[3], p1.position[3], p1.normal[3]);
        l.triUV[2 * (size_t)t + 1] = make_float4(p2.position[3], p2.normal[3], 0.f, 0.f);
    }
    return l;
}

// objects: inverse computed once on the host with the shared
// rt_mat4_inverse, root metadata resolved against the uploaded BVH.
ObjectLayout layout_objects(const RenderObject* o, uint32_t n, const std::vector<RootInfo>& rootOf, uint32_t materialCount,
                            int objTreeMin, int maskIdentity) {
    ObjectLayout l;
    const auto fail = refused<ObjectLayout>;
    l.inv.resize((size_t)std::max(n, 1u) * 3);
    l.fwd.resize((size_t)std::max(n, 1u) * 3);
    l.meta.resize(std::max(n, 1u));
    l.box.assign((size_t)std::max(n, 1u) * 2, make_float4(0.f, 0.f, 0.f, 0.f));
    uint32_t nGeneral = 0;
    double minScale = 1e300;  // smallest size-and-position scale among the padded boxes
    for (uint32_t i = 0; i < n; i++) {
        float4 *inv = &l.inv[3 * (size_t)i], *fwd = &l.fwd[3 * (size_t)i], *box = &l.box[2 * (size_t)i];
        float im[16];
        rt_mat4_inverse(o[i].transformMatrix, im);
        rows_of(im, inv);
        rows_of(o[i].transformMatrix, fwd);
        if (o[i].bvhIndex >= rootOf.size()) return fail("object.bvhIndex out of range");
        const RootInfo& r = rootOf[o[i].bvhIndex];
        if (r.idx == 0xffffffffu) return fail("object.bvhIndex does not point at a mesh root of the uploaded BVH");
        if (o[i].materialIndex >= std::max(materialCount, 1u)) return fail("object.materialIndex out of range");
        const bool isIdent = rows_are_identity(inv);  // exact identity inverse: the traversal may reuse the world-space ray (k_trace_pw)
        // World-space box of the object, padded: a ray that cannot reach it before its current closest hit cannot reach the
        // object's root box in object space either, so the object is worth exactly the reference's two box tests on the root's
        // children (or the root leaf's triangle tests) and no set-up. Padding 1e-3 of the box's size and position: four
        // orders of magnitude above what the fp32 inverse and the two slab tests can disagree by.
        uint32_t flags = isIdent ? RT_OBJ_IDENTITY : 0u;
        nGeneral += isIdent ? 0u : 1u;
        if (!isIdent) {
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            bool finite = true;
            for (int corner = 0; corner < 8; corner++) {
                const double p[3] = {(corner & 1) ? r.hi[0] : r.lo[0], (corner & 2) ? r.hi[1] : r.lo[1], (corner & 4) ? r.hi[2] : r.lo[2]};
                for (int d = 0; d < 3; d++) {
                    const float* m = o[i].transformMatrix;
                    const double w = (double)m[0 * 4 + d] * p[0] + (double)m[1 * 4 + d] * p[1] + (double)m[2 * 4 + d] * p[2] + (double)m[3 * 4 + d];
                    finite = finite && std::isfinite(w);
                    lo[d] = std::min(lo[d], w); hi[d] = std::max(hi[d], w);
                }
            }
            for (int k = 0; k < 12; k++) finite = finite && std::isfinite((&inv[0].x)[k]);
            if (finite) {
                double pad = 1e-6;
                for (int d = 0; d < 3; d++) pad = std::max(pad, 1e-3 * std::max(hi[d] - lo[d], std::max(std::fabs(lo[d]), std::fabs(hi[d]))));
                minScale = std::min(minScale, pad * 1e3);
                box[0] = make_float4((float)(lo[0] - pad), (float)(lo[1] - pad), (float)(lo[2] - pad), 0.f);
                box[1] = make_float4((float)(hi[0] + pad), (float)(hi[1] + pad), (float)(hi[2] + pad), 0.f);
                flags |= RT_OBJ_BOX | RT_OBJ_MASKABLE;  // the rays' creators may rule the object out as well
            }
        }
        if (isIdent && maskIdentity) {  // exact root box: the rays' creators could rule the object out with the traversal's own
            box[0] = make_float4(r.lo[0], r.lo[1], r.lo[2], 0.f);   // slab test. Off by default: measured, the rounds
            box[1] = make_float4(r.hi[0], r.hi[1], r.hi[2], 0.f);   // this saves are the cheap ones (profiles/README.md)
            flags |= RT_OBJ_MASKABLE;
        }
        if (isIdent && rows_are_identity(fwd)) flags |= RT_OBJ_FWD_IDENTITY;
        l.meta[i] = make_uint4(r.idx, r.cnt, o[i].materialIndex, flags | ((o[i].samplerIndex & RT_OBJ_SAMPLER_MASK) << RT_OBJ_SAMPLER_SHIFT));
        // flags and root triangle count ride in the box's w components (one fetch per object in the skipping loop)
        memcpy(&box[0].w, &flags, 4);
        memcpy(&box[1].w, &r.cnt, 4);
    }
    // the objects a ray's creator tests for the ray's object mask. The mask has 32 bits; its window starts at the first object
    // that can be ruled out at all, so that a scene like C5 (26 identity groups, then sixteen placed dragons) has all its
    // placed objects under the mask
    l.maskBox.assign(64, make_float4(0.f, 0.f, 0.f, 0.f));
    while (l.maskBase < n && !(l.meta[l.maskBase].w & RT_OBJ_MASKABLE)) l.maskBase++;
    if (l.maskBase >= n) l.maskBase = 0;
    for (uint32_t i = l.maskBase; i < std::min(n, l.maskBase + 32u); i++)
        if (l.meta[i].w & RT_OBJ_MASKABLE) {
            const uint32_t k = l.reachCount++, w = i - l.maskBase;
            l.maskBox[2 * k] = l.box[2 * (size_t)i]; l.maskBox[2 * k + 1] = l.box[2 * (size_t)i + 1];
            memcpy(&l.maskBox[2 * k].w, &w, 4);
        }
    // one general-transform object among identity ones (Sponza's emitter) does not pay for either mechanism: measured +3 % and
    // +8..19 % on that scene; from two on they do (Cornell + model: -5..-13 %)
    // The padding dominates the rounding of the world-space slab test and of the object-space ray only while the ray's
    // origin is not much farther out than the objects are big: both errors grow like 6e-8 * |origin|. Rays
    // that start beyond 1e3 object scales take the reference's own route through every object.
    l.cullOriginLimit = minScale < 1e300 ? (float)(minScale * 1e3) : 0.f;
    l.cull = nGeneral >= 2 || (maskIdentity && l.reachCount);
    if (!l.cull) l.reachCount = 0;
    // what the reference spends on objects [0, i) when a ray misses them all: two box tests per interior root, the root's
    // triangles per leaf root. A run of skipped objects costs the difference of two entries (trace_wave: fetch_next_meta);
    // skipCost is the same over the mask's window, from its start.
    l.cost.assign((size_t)n + 1, make_uint2(0u, 0u));
    for (uint32_t i = 0; i < n; i++) {
        l.cost[i + 1] = l.cost[i];
        if (l.meta[i].y == 0u) l.cost[i + 1].x += 2u; else l.cost[i + 1].y += l.meta[i].y;
    }
    l.skipCost.assign(33, make_uint2(0u, 0u));
    for (uint32_t w = 1; w <= 32u; w++) {
        const uint2 &from = l.cost[l.maskBase], &to = l.cost[std::min(l.maskBase + w, n)];
        l.skipCost[w] = make_uint2(to.x - from.x, to.y - from.y);
    }
    // the hierarchy over runs of general-transform objects with a padded box, for scenes with many of them: measured on 256
    // separated bunny instances (tools/heuristics_table.py) against 7 % lost on C5's sixteen overlapping dragons, which stay
    // below the threshold (and inside the rays' object masks anyway)
    if (objTreeMin > 0 && nGeneral >= (uint32_t)objTreeMin) {
        auto skippable = [&](uint32_t i) { return i < n && (l.meta[i].w & (RT_OBJ_IDENTITY | RT_OBJ_BOX)) == RT_OBJ_BOX; };
        for (uint32_t k = 1; k <= (uint32_t)RT_OBJTREE_LEVELS; k++) {
            l.treeOff[k] = (uint32_t)(l.tree.size() / 2);
            const uint32_t nb = (n + (1u << k) - 1) >> k;
            for (uint32_t b = 0; b < nb; b++) {
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                bool ok = true;
                for (uint32_t i = b << k; i < ((b + 1) << k); i++) {
                    if (!skippable(i)) { ok = false; break; }
                    const float4 &bl = l.box[2 * (size_t)i], &bh = l.box[2 * (size_t)i + 1];
                    lo[0] = std::min(lo[0], bl.x); lo[1] = std::min(lo[1], bl.y); lo[2] = std::min(lo[2], bl.z);
                    hi[0] = std::max(hi[0], bh.x); hi[1] = std::max(hi[1], bh.y); hi[2] = std::max(hi[2], bh.z);
                }
                l.tree.push_back(ok ? make_float4(lo[0], lo[1], lo[2], 1.f) : make_float4(0.f, 0.f, 0.f, 0.f));
                l.tree.push_back(ok ? make_float4(hi[0], hi[1], hi[2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f));
            }
        }
        l.treeLevels = (uint32_t)RT_OBJTREE_LEVELS;
    }
    if (l.tree.empty()) l.tree.assign(2, make_float4(0.f, 0.f, 0.f, 0.f));
    return l;
}

SceneLayout layout_scene(const RtSceneArrays& s, int objTreeMin, int maskIdentity) {
    SceneLayout l;
    l.meshes = layout_meshes(s);
    if (!(l.error = l.meshes.error).empty()) return l;
    if (s.materialCount == 0) { l.error = "scene needs at least one material"; return l; }
    for (uint32_t i = 0; i < s.sphereCount; i++)
        if (s.spheres[i].materialIndex >= s.materialCount) { l.error = "sphere.materialIndex out of range"; return l; }
    l.objects = layout_objects(s.objects, s.objectCount, l.meshes.rootOf, s.materialCount, objTreeMin, maskIdentity);
    l.error = l.objects.error;
    return l;
}

void dump_object_tree(const ObjectLayout& l, uint32_t n) {
    for (uint32_t k = 1; k <= l.treeLevels; k++) {
        const uint32_t nb = (n + (1u << k) - 1) >> k;
        uint32_t valid = 0;
        for (uint32_t b = 0; b < nb; b++) valid += l.tree[2 * (size_t)(l.treeOff[k] + b)].w != 0.f;
        const float4 &lo = l.tree[2 * (size_t)(l.treeOff[k] + std::min(1u, nb - 1))], &hi = l.tree[2 * (size_t)(l.treeOff[k] + std::min(1u, nb - 1)) + 1];
        fprintf(stderr, "[objtree] level %u: %u blocks, %u valid; block 1: (%g %g %g)-(%g %g %g)\n", k, nb, valid, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    }
    for (uint32_t i = 0; i < std::min(n, 6u); i++) {
        const float4 &lo = l.box[2 * i], &hi = l.box[2 * i + 1];
        fprintf(stderr, "[objtree] object %u flags %x box (%g %g %g)-(%g %g %g)\n", i, l.meta[i].w, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
    }
}

std::vector<float4> layout_materials(const RayMaterial* m, uint32_t n) {
    std::vector<float4> out((size_t)std::max(n, 1u) * 3);
    for (uint32_t i = 0; i < n; i++) {
        out[3 * i + 0] = make_float4(m[i].albedo[0], m[i].albedo[1], m[i].albedo[2], m[i].reflectance);
        out[3 * i + 1] = make_float4(m[i].emissionColor[0], m[i].emissionColor[1], m[i].emissionColor[2], m[i].emissionStrength);
        float ai, mi, bi;   // bits of the ints; -1 = no texture
        memcpy(&ai, &m[i].albedoIndex, 4);
        memcpy(&mi, &m[i].metalnessIndex, 4);
        memcpy(&bi, &m[i].bumpIndex, 4);
        out[3 * i + 2] = make_float4(m[i].ior, ai, mi, bi);
    }
    return out;
}

SphereLayout layout_spheres(const Sphere* s, uint32_t n) {
    SphereLayout l;
    l.spheres.resize(std::max(n, 1u));
    l.mat.resize(std::max(n, 1u));
    for (uint32_t i = 0; i < n; i++) {
        l.spheres[i] = make_float4(s[i].position[0], s[i].position[1], s[i].position[2], s[i].radius);
        l.mat[i] = s[i].materialIndex;
    }
    for (uint32_t i = 0; i < std::min(n, 32u); i++) {
        bool repeat = false;
        for (uint32_t k = 0; k < i && !repeat; k++) repeat = memcmp(&l.spheres[i], &l.spheres[k], sizeof(float4)) == 0;
        if (!repeat) l.testMask |= 1u << i;
    }
    return l;
}

TextureLayout layout_textures(const RtTexture* tex, uint32_t n) {
    TextureLayout l;
    if (n > (uint32_t)RT_MAX_TEXTURES) { l.error = "more than RT_MAX_TEXTURES textures"; return l; }
    l.info.assign(std::max(n, 1u), make_uint4(0u, 1u, 1u, 0u));
    size_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!tex[i].rgba8 || tex[i].width == 0 || tex[i].height == 0) { l.error = "texture " + std::to_string(i) + " is empty"; return l; }
        if ((uint64_t)tex[i].width * tex[i].height > (1ull << 28) || total + (size_t)tex[i].width * tex[i].height > 0xffffffffull) { l.error = "textures too large"; return l; }
        l.info[i] = make_uint4((uint32_t)total, tex[i].width, tex[i].height, 0u);
        total += (size_t)tex[i].width * tex[i].height;
    }
    l.texels.assign(std::max<size_t>(total, 1), 0u);
    for (uint32_t i = 0; i < n; i++) memcpy(&l.texels[l.info[i].x], tex[i].rgba8, (size_t)tex[i].width * tex[i].height * 4);
    return l;
}

// The metalness, alpha and bump maps (declared semantics, include/rt_det_math.h): which of them the scene binds at all (the
// kernels that read them are separate ones, picked by these bits), and every object's alpha map for the traversal.
MapLayout layout_maps(const SceneSources& src, uint32_t texCount) {
    MapLayout l;
    const uint32_t n = (uint32_t)src.objMat.size();
    auto bound = [&](int32_t index) { return index >= 0 && (uint32_t)index < texCount; };
    l.objAlpha.assign(std::max(n, 1u), RT_OBJALPHA_NONE);
    for (uint32_t i = 0; i < n; i++) {
        if (src.objMat[i] >= src.mats.size()) continue;
        const RayMaterial& m = src.mats[src.objMat[i]];
        if (bound(m.metalnessIndex)) l.mapFlags |= RT_MAP_METALNESS;
        if (bound(m.bumpIndex)) l.mapFlags |= RT_MAP_BUMP;
        if (bound(m.alphaIndex)) { l.mapFlags |= RT_MAP_ALPHA; l.objAlpha[i] = (uint32_t)m.alphaIndex | (src.objSampler[i] == 1u ? RT_OBJALPHA_CLAMP : 0u); }
    }
    return l;
}

// The shortcut is only taken when it is cheap (at most RT_EMIT_MAX_TRIS triangles) and exact: the NEE term of a query that
// is answered "not emissive" is emission * 0, which is 0 only while every material's emissionColor * emissionStrength is finite.
EmitterLayout layout_emitters(const SceneSources& src, const std::vector<RootInfo>& rootOf, uint32_t texCount) {
    const EmitterLayout none;
    EmitterLayout l;
    if (src.mats.empty()) return none;
    auto emissive = [&](uint32_t m) { return m < src.mats.size() && !(src.mats[m].emissionStrength == 0.f); };
    for (const RayMaterial& m : src.mats)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(m.emissionColor[k] * m.emissionStrength)) return none;
    for (size_t i = 0; i < src.sphereMat.size() && i < 32; i++)
        if (emissive(src.sphereMat[i])) l.sphereMask |= 1u << i;
    for (size_t i = 32; i < src.sphereMat.size(); i++)
        if (emissive(src.sphereMat[i])) return none;  // beyond the mask (the reference has ten spheres)
    for (size_t i = 0; i < src.objMat.size(); i++) {
        if (!emissive(src.objMat[i])) continue;
        { const int32_t ai = src.mats[src.objMat[i]].alphaIndex; if (ai >= 0 && (uint32_t)ai < texCount) return none; }  // an emitter with holes: its list entries would need the map
        const RootInfo& r = rootOf[src.objRoot[i]];
        if (r.triTotal == 0xffffffffu || l.tris.size() + r.triTotal > (size_t)RT_EMIT_MAX_TRIS) return none;
        for (uint32_t t = 0; t < r.triTotal; t++) l.tris.push_back(make_uint2((uint32_t)i, r.triFirst + t));
    }
    l.mode = 1;
    return l;
}
