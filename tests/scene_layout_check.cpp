// scene_layout_check.cpp — the device scene tables (ray_tracer_amd/csrc/scene_layout.h) checked on the CPU against the scene they
// are derived from: node numbering, node tables, roots, per-object tables, the object hierarchy, spheres, emitters, maps, and
// every refusal. Driven by tests/test_scene_layout.py:  scene_layout_check <assets dir>
#include "scene_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <vector>

#include "rt_det_math.h"
#include "check.h"

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same3(const float4& v, float x, float y, float z) { return bits(v.x) == bits(x) && bits(v.y) == bits(y) && bits(v.z) == bits(z); }
static bool same4(const float4& a, const float4& b) { return memcmp(&a, &b, 16) == 0; }

struct Walk { uint32_t depth = 0; uint64_t lo = ~0ull, hi = 0, sum = 0; };
static void walk(const BVHNode* nodes, uint32_t n, uint32_t d, Walk& w) {
    const BVHNode& b = nodes[n];
    if (b.triCount) {
        w.depth = std::max(w.depth, d);
        w.lo = std::min<uint64_t>(w.lo, b.index); w.hi = std::max<uint64_t>(w.hi, (uint64_t)b.index + b.triCount); w.sum += b.triCount;
        return;
    }
    walk(nodes, b.index, d + 1, w);
    walk(nodes, b.index + 1, d + 1, w);
}

static void check_meshes(const RtSceneArrays& a, const MeshLayout& m) {
    CHECK(m.error.empty(), "%s", m.error.c_str());
    if (!m.error.empty()) return;
    const uint32_t nNodes = a.bvhNodeCount;
    std::set<uint32_t> roots;
    for (uint32_t i = 0; i < a.objectCount; i++) roots.insert(a.objects[i].bvhIndex);

    // ---- numbering
    CHECK(m.nodeRemap.size() == nNodes, "%zu", m.nodeRemap.size());
    std::set<uint32_t> used;
    for (uint32_t n = 0; n < nNodes; n++) {
        CHECK(m.nodeRemap[n] < m.nodeCount, "node %u -> %u of %u", n, m.nodeRemap[n], m.nodeCount);
        CHECK(used.insert(m.nodeRemap[n]).second, "node %u shares device slot %u", n, m.nodeRemap[n]);
        const BVHNode& b = a.bvhNodes[n];
        if (b.triCount == 0) {
            CHECK(m.nodeRemap[b.index + 1] == m.nodeRemap[b.index] + 1, "children of node %u are not adjacent", n);
            CHECK((m.nodeRemap[b.index] & 1u) == 0u, "first child of node %u on odd slot %u", n, m.nodeRemap[b.index]);
        }
    }
    for (uint32_t r : roots) CHECK((m.nodeRemap[r] & 1u) || m.nodeRemap[r] < m.hotNodes, "root %u on slot %u", r, m.nodeRemap[r]);
    CHECK(m.hotNodes <= 2 * RT_HOT_PAIRS && m.hotNodes % 2 == 0, "%u", m.hotNodes);
    {   // the hot pairs: breadth first over the roots, the children of nodes at depth < 8
        std::deque<std::pair<uint32_t, int>> queue;
        for (uint32_t r : roots) queue.emplace_back(r, 0);
        uint32_t pair = 0;
        while (!queue.empty()) {
            auto [n, depth] = queue.front();
            queue.pop_front();
            const BVHNode& b = a.bvhNodes[n];
            if (b.triCount || depth >= 8) continue;
            if (pair < m.hotNodes / 2) CHECK(m.nodeRemap[b.index] == 2 * pair, "pair %u of the breadth-first order is at slot %u", pair, m.nodeRemap[b.index]);
            else CHECK(m.nodeRemap[b.index] >= m.hotNodes, "pair %u beyond the hot ones at slot %u", pair, m.nodeRemap[b.index]);
            pair++;
            queue.emplace_back(b.index, depth + 1);
            queue.emplace_back(b.index + 1, depth + 1);
        }
        CHECK(m.hotNodes / 2 == std::min(pair, RT_HOT_PAIRS), "%u hot pairs of %u candidates", m.hotNodes / 2, pair);
    }

    // ---- node tables
    CHECK(m.nodes.size() == (size_t)std::max(m.nodeCount, 2u) * 2 && m.nodesPk.size() == m.nodes.size() && m.leafFirst.size() == std::max(m.nodeCount, 1u), "sizes");
    for (uint32_t n = 0; n < nNodes; n++) {
        const BVHNode& b = a.bvhNodes[n];
        const uint32_t d = m.nodeRemap[n];
        const float4 &lo = m.nodes[2 * (size_t)d], &hi = m.nodes[2 * (size_t)d + 1];
        CHECK(same3(lo, b.boundsX[0], b.boundsY[0], b.boundsZ[0]) && same3(hi, b.boundsX[1], b.boundsY[1], b.boundsZ[1]), "bounds of node %u", n);
        CHECK(bits(hi.w) == b.triCount, "triCount of node %u", n);
        const uint32_t w0 = bits(lo.w);
        if (b.triCount == 0) {
            CHECK(w0 == m.nodeRemap[b.index], "W0 of interior node %u: %x", n, w0);
        } else if (b.triCount <= 7) {
            CHECK((w0 & RT_LEAF_BIT) && ((w0 >> RT_LEAF_CNT_SHIFT) & 7u) == b.triCount && (w0 & RT_LEAF_IDX_MASK) == b.index, "W0 of leaf %u: %x", n, w0);
        } else {
            CHECK(w0 == (RT_LEAF_BIT | d), "W0 of big leaf %u: %x", n, w0);
            CHECK(m.leafFirst[d] == b.index, "leafFirst of big leaf %u", n);
        }
    }
    for (size_t p = 0; p + 1 < m.nodeCount; p += 2) {
        const float4 lo1 = m.nodes[2 * p], hi1 = m.nodes[2 * p + 1], lo2 = m.nodes[2 * p + 2], hi2 = m.nodes[2 * p + 3];
        const float4 want[4] = {make_float4(lo1.x, lo1.y, hi1.x, hi1.y), make_float4(lo2.x, lo2.y, hi2.x, hi2.y),
                                make_float4(lo1.z, hi1.z, lo2.z, hi2.z), make_float4(lo1.w, lo2.w, 0.f, 0.f)};
        CHECK(memcmp(&m.nodesPk[2 * p], want, sizeof want) == 0, "nodesPk of pair %zu", p);
    }

    // ---- roots, depth
    uint32_t depth = 0;
    CHECK(m.rootOf.size() == nNodes, "%zu", m.rootOf.size());
    for (uint32_t n = 0; n < nNodes; n++) {
        const RootInfo& r = m.rootOf[n];
        CHECK((r.idx != 0xffffffffu) == (roots.count(n) == 1), "rootOf[%u].idx = %x", n, r.idx);
        if (!roots.count(n)) continue;
        const BVHNode& b = a.bvhNodes[n];
        Walk w;
        walk(a.bvhNodes, n, 0, w);
        depth = std::max(depth, w.depth);
        CHECK(r.idx == bits(m.nodes[2 * (size_t)m.nodeRemap[n]].w) && r.cnt == b.triCount, "root %u word", n);
        CHECK(bits(r.lo[0]) == bits(b.boundsX[0]) && bits(r.lo[1]) == bits(b.boundsY[0]) && bits(r.lo[2]) == bits(b.boundsZ[0]) &&
              bits(r.hi[0]) == bits(b.boundsX[1]) && bits(r.hi[1]) == bits(b.boundsY[1]) && bits(r.hi[2]) == bits(b.boundsZ[1]), "root %u box", n);
        CHECK(r.triFirst == (uint32_t)w.lo, "root %u triFirst %u", n, r.triFirst);
        CHECK(r.triTotal == (w.sum == w.hi - w.lo ? (uint32_t)w.sum : 0xffffffffu), "root %u triTotal %u", n, r.triTotal);
    }
    CHECK(m.maxLeafDepth == depth, "%u, the checker walks %u", m.maxLeafDepth, depth);

    // ---- triangles
    for (uint32_t t = 0; t < a.triangleCount; t++) {
        const Triangle& tr = a.triangles[t];
        const TrianglePoint* p[3] = {&a.triPoints[tr.v0], &a.triPoints[tr.v1], &a.triPoints[tr.v2]};
        for (int k = 0; k < 3; k++) {
            CHECK(same3(m.triPos[3 * (size_t)t + k], p[k]->position[0], p[k]->position[1], p[k]->position[2]) &&
                  bits(m.triPos[3 * (size_t)t + k].w) == ((k == 0 && tr.frontOnly) ? 1u : 0u), "triPos %u.%d", t, k);
            CHECK(same3(m.triNrm[3 * (size_t)t + k], p[k]->normal[0], p[k]->normal[1], p[k]->normal[2]), "triNrm %u.%d", t, k);
        }
        CHECK(same4(m.triUV[2 * (size_t)t], make_float4(p[0]->position[3], p[0]->normal[3], p[1]->position[3], p[1]->normal[3])) &&
              same4(m.triUV[2 * (size_t)t + 1], make_float4(p[2]->position[3], p[2]->normal[3], 0.f, 0.f)), "triUV %u", t);
    }
}

struct ObjectFacts { uint32_t general = 0, maskBase = 0, beyondWindow = 0; };

static ObjectFacts check_objects(const RtSceneArrays& a, const std::vector<RenderObject>& o, const MeshLayout& m, int treeMin, int maskIdentity) {
    const uint32_t n = (uint32_t)o.size();
    const ObjectLayout l = layout_objects(o.data(), n, m.rootOf, a.materialCount, treeMin, maskIdentity);
    ObjectFacts facts;
    CHECK(l.error.empty(), "%s", l.error.c_str());
    if (!l.error.empty()) return facts;
    static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(l.inv.size() == (size_t)std::max(n, 1u) * 3 && l.fwd.size() == l.inv.size() && l.meta.size() == std::max(n, 1u) && l.box.size() == (size_t)std::max(n, 1u) * 2 &&
          l.maskBox.size() == 64 && l.skipCost.size() == 33 && l.cost.size() == (size_t)n + 1, "sizes");
    std::vector<bool> general(n), boxed(n), maskable(n);
    for (uint32_t i = 0; i < n; i++) {
        const float* fm = o[i].transformMatrix;
        float im[16];
        rt_mat4_inverse(fm, im);
        bool invIdent = true, fwdIdent = true;
        for (int k = 0; k < 16; k++) {
            if (k % 4 == 3) continue;  // rows 0..2 of the column-major matrices are what the tables carry
            invIdent = invIdent && im[k] == ident[k];
            fwdIdent = fwdIdent && fm[k] == ident[k];
        }
        for (int r = 0; r < 3; r++) {
            CHECK(same4(l.inv[3 * (size_t)i + r], make_float4(im[r], im[4 + r], im[8 + r], im[12 + r])), "inverse row %d of object %u", r, i);
            CHECK(same4(l.fwd[3 * (size_t)i + r], make_float4(fm[r], fm[4 + r], fm[8 + r], fm[12 + r])), "matrix row %d of object %u", r, i);
        }
        const RootInfo& root = m.rootOf[o[i].bvhIndex];
        const uint4 meta = l.meta[i];
        const float4 &lo = l.box[2 * (size_t)i], &hi = l.box[2 * (size_t)i + 1];
        CHECK(meta.x == root.idx && meta.y == root.cnt && meta.z == o[i].materialIndex, "meta of object %u", i);
        CHECK((meta.w >> RT_OBJ_SAMPLER_SHIFT) == (o[i].samplerIndex & RT_OBJ_SAMPLER_MASK), "sampler of object %u", i);
        CHECK((meta.w & 0xffffu) == bits(lo.w) && bits(hi.w) == root.cnt, "box words of object %u: %x %x", i, meta.w, bits(lo.w));
        CHECK(((meta.w & RT_OBJ_IDENTITY) != 0) == invIdent, "identity flag of object %u", i);
        CHECK(((meta.w & RT_OBJ_FWD_IDENTITY) != 0) == (invIdent && fwdIdent), "matrix identity flag of object %u", i);
        CHECK(((meta.w & RT_OBJ_BOX) != 0) == !invIdent, "box flag of object %u (every transform here is finite)", i);
        CHECK(((meta.w & RT_OBJ_MASKABLE) != 0) == (!invIdent || maskIdentity), "mask flag of object %u", i);
        CHECK((meta.w & 0xfff0u) == 0u, "unknown flags of object %u: %x", i, meta.w);
        general[i] = !invIdent; boxed[i] = (meta.w & (RT_OBJ_IDENTITY | RT_OBJ_BOX)) == RT_OBJ_BOX; maskable[i] = meta.w & RT_OBJ_MASKABLE;
        facts.general += general[i];
        if (meta.w & RT_OBJ_BOX) {
            for (int corner = 0; corner < 8; corner++) {
                const double p[3] = {(corner & 1) ? root.hi[0] : root.lo[0], (corner & 2) ? root.hi[1] : root.lo[1], (corner & 4) ? root.hi[2] : root.lo[2]};
                for (int d = 0; d < 3; d++) {
                    const double w = (double)fm[d] * p[0] + (double)fm[4 + d] * p[1] + (double)fm[8 + d] * p[2] + (double)fm[12 + d];
                    CHECK((double)(&lo.x)[d] < w && w < (double)(&hi.x)[d], "corner %d of object %u outside its padded box on axis %d", corner, i, d);
                }
            }
        } else if (meta.w & RT_OBJ_MASKABLE) {
            CHECK(same3(lo, root.lo[0], root.lo[1], root.lo[2]) && same3(hi, root.hi[0], root.hi[1], root.hi[2]), "exact root box of identity object %u", i);
        } else {
            CHECK(same3(lo, 0.f, 0.f, 0.f) && same3(hi, 0.f, 0.f, 0.f), "box of object %u without a box flag", i);
        }
    }

    // ---- the mask window
    uint32_t base = 0;
    while (base < n && !maskable[base]) base++;
    if (base >= n) base = 0;
    CHECK(l.maskBase == base, "%u, expected %u", l.maskBase, base);
    uint32_t k = 0;
    for (uint32_t i = base; i < std::min(n, base + 32u); i++) {
        if (!maskable[i]) continue;
        const float4 &lo = l.box[2 * (size_t)i], &hi = l.box[2 * (size_t)i + 1];
        CHECK(same3(l.maskBox[2 * k], lo.x, lo.y, lo.z) && bits(l.maskBox[2 * k].w) == i - base && same3(l.maskBox[2 * k + 1], hi.x, hi.y, hi.z), "maskBox entry %u (object %u)", k, i);
        k++;
    }
    for (uint32_t e = 2 * k; e < 64; e++) CHECK(same4(l.maskBox[e], make_float4(0.f, 0.f, 0.f, 0.f)), "maskBox[%u] beyond the %u entries", e, k);
    const bool cull = facts.general >= 2 || (maskIdentity && k);
    CHECK(l.cull == cull, "cull %d with %u general objects, maskIdentity %d, %u under the mask", (int)l.cull, facts.general, maskIdentity, k);
    CHECK(l.reachCount == (cull ? k : 0u), "reachCount %u", l.reachCount);
    CHECK((l.cullOriginLimit > 0.f) == (facts.general > 0), "cullOriginLimit %g", l.cullOriginLimit);
    facts.maskBase = base;
    for (uint32_t i = base + 32u; i < n; i++) facts.beyondWindow += general[i];

    // ---- what a missed object costs the reference
    CHECK(l.cost[0].x == 0 && l.cost[0].y == 0, "cost[0]");
    for (uint32_t i = 0; i < n; i++) {
        const BVHNode& root = a.bvhNodes[o[i].bvhIndex];
        CHECK(l.cost[i + 1].x - l.cost[i].x == (root.triCount ? 0u : 2u) && l.cost[i + 1].y - l.cost[i].y == root.triCount, "cost of object %u", i);
    }
    for (uint32_t w = 0; w <= 32; w++) {
        const uint2 from = l.cost[base], to = l.cost[std::min(base + w, n)];
        CHECK(l.skipCost[w].x == to.x - from.x && l.skipCost[w].y == to.y - from.y, "skipCost[%u]", w);
    }

    // ---- the hierarchy
    const uint32_t levels = (treeMin > 0 && facts.general >= (uint32_t)treeMin) ? (uint32_t)RT_OBJTREE_LEVELS : 0u;
    CHECK(l.treeLevels == levels, "%u levels with %u general objects and objTreeMin %d", l.treeLevels, facts.general, treeMin);
    uint32_t off = 0;
    for (uint32_t lv = 1; lv <= l.treeLevels; lv++) {
        CHECK(l.treeOff[lv] == off, "treeOff[%u] = %u, expected %u", lv, l.treeOff[lv], off);
        const uint32_t nb = (n + (1u << lv) - 1) >> lv;
        for (uint32_t b = 0; b < nb; b++) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            bool valid = true;
            for (uint32_t i = b << lv; i < ((b + 1) << lv); i++) {
                valid = valid && i < n && boxed[i];
                if (!valid) break;
                for (int d = 0; d < 3; d++) { lo[d] = std::min(lo[d], (&l.box[2 * (size_t)i].x)[d]); hi[d] = std::max(hi[d], (&l.box[2 * (size_t)i + 1].x)[d]); }
            }
            const float4 &tl = l.tree[2 * (size_t)(off + b)], &th = l.tree[2 * (size_t)(off + b) + 1];
            if (valid) CHECK(same4(tl, make_float4(lo[0], lo[1], lo[2], 1.f)) && same4(th, make_float4(hi[0], hi[1], hi[2], 0.f)), "level %u block %u is not the union of its boxes", lv, b);
            else CHECK(same4(tl, make_float4(0.f, 0.f, 0.f, 0.f)) && same4(th, make_float4(0.f, 0.f, 0.f, 0.f)), "level %u block %u marked valid", lv, b);
        }
        off += nb;
    }
    CHECK(l.tree.size() == 2 * (size_t)std::max(off, 1u), "tree size %zu", l.tree.size());
    return facts;
}

// every objTreeMin with and without identity objects under the mask
static ObjectFacts check_objects_all(const RtSceneArrays& a, const std::vector<RenderObject>& o, const MeshLayout& m) {
    ObjectFacts f;
    for (int treeMin : {0, 2, 48})
        for (int maskIdentity : {1, 0}) f = check_objects(a, o, m, treeMin, maskIdentity);
    return f;   // (of the default: identity objects outside the mask)
}

// ---------------------------------------------------------------- hand-built scenes
struct Built {
    std::vector<Sphere> spheres;
    std::vector<RayMaterial> mats;
    std::vector<TrianglePoint> points;
    std::vector<Triangle> tris;
    std::vector<RenderObject> objects;
    std::vector<BVHNode> nodes;
    RtSceneArrays arrays() const {
        return RtSceneArrays{spheres.data(), (uint32_t)spheres.size(), mats.data(), (uint32_t)mats.size(), points.data(), (uint32_t)points.size(),
                             tris.data(), (uint32_t)tris.size(), objects.data(), (uint32_t)objects.size(), nodes.data(), (uint32_t)nodes.size()};
    }
};
static BVHNode node(uint32_t index, uint32_t triCount, float lo = -1.f, float hi = 1.f) { return BVHNode{{lo, hi}, {lo, hi}, {lo, hi}, index, triCount}; }
static RenderObject object(uint32_t bvhIndex, uint32_t material = 0) {
    RenderObject o{};
    o.transformMatrix[0] = o.transformMatrix[5] = o.transformMatrix[10] = o.transformMatrix[15] = 1.f;
    o.bvhIndex = bvhIndex; o.materialIndex = material;
    return o;
}
// nTris triangles over three points, one material, one sphere, no nodes or objects yet
static Built base(uint32_t nTris) {
    Built b;
    b.spheres.assign(1, Sphere{});
    RayMaterial m;
    rt_material_default(&m);
    b.mats.assign(1, m);
    b.points.assign(3, TrianglePoint{});
    b.points[1].position[0] = b.points[2].position[1] = 1.f;
    Triangle t{};
    t.v1 = 1; t.v2 = 2;
    b.tris.assign(nTris, t);
    return b;
}
// a root over two leaves of one triangle each
static Built small_tree() {
    Built b = base(2);
    b.nodes = {node(1, 0), node(0, 1), node(1, 1)};
    b.objects = {object(0)};
    return b;
}

static void expect_refusal(const char* what, const Built& b, const char* message) {
    g_where = std::string("refusal: ") + what;
    const SceneLayout l = layout_scene(b.arrays(), 48, 0);
    CHECK(l.error == message, "got \"%s\", expected \"%s\"", l.error.c_str(), message);
}

static void check_refusals() {
    { Built b = small_tree(); b.nodes[0].index = 5; expect_refusal("child index out of range", b, "BVH child index out of range"); }
    { Built b = small_tree(); b.nodes[0].index = 2; expect_refusal("second child out of range", b, "BVH child index out of range"); }
    {   // two interior nodes with the same children: the walk meets more nodes than the BVH has
        Built b = base(2);
        b.nodes = {node(1, 0), node(3, 0), node(3, 0), node(0, 1), node(1, 1)};
        b.objects = {object(0)};
        expect_refusal("shared children", b, "BVH has a cycle");
    }
    { Built b = small_tree(); b.nodes[1] = node(1, 0); expect_refusal("cycle", b, "BVH has a cycle"); }
    { Built b = small_tree(); b.nodes[2].triCount = 2; expect_refusal("leaf range out of bounds", b, "BVH leaf triangle range out of bounds"); }
    {   // a chain: every interior node has a leaf and the next interior node; the last leaves sit at depth 66
        Built b = base(1);
        b.nodes.push_back(node(1, 0));
        for (uint32_t d = 0; d < 65; d++) { b.nodes.push_back(node(0, 1)); b.nodes.push_back(node((uint32_t)b.nodes.size() + 1, 0)); }
        b.nodes.push_back(node(0, 1)); b.nodes.push_back(node(0, 1));
        b.objects = {object(0)};
        expect_refusal("depth above 64", b, "BVH deeper than 64 levels (the reference's builder caps at 64)");
        b.nodes.resize(b.nodes.size() - 4);   // one level less: depth 64 exactly is accepted
        b.nodes[b.nodes.size() - 1] = node(0, 1);
        g_where = "depth 64";
        const MeshLayout m = layout_meshes(b.arrays());
        CHECK(m.error.empty() && m.maxLeafDepth == 64, "\"%s\", depth %u", m.error.c_str(), m.maxLeafDepth);
        if (m.error.empty()) check_meshes(b.arrays(), m);
    }
    { Built b = small_tree(); b.objects[0].bvhIndex = 3; expect_refusal("bvhIndex >= nodeCount", b, "object.bvhIndex out of range"); }
    { Built b = small_tree(); b.objects[0].materialIndex = 1; expect_refusal("material index out of range", b, "object.materialIndex out of range"); }
    { Built b = small_tree(); b.tris[1].v2 = 3; expect_refusal("triangle point index out of range", b, "triangle point index out of range"); }
    { Built b = small_tree(); b.mats.clear(); expect_refusal("zero materials", b, "scene needs at least one material"); }
    { Built b = small_tree(); b.spheres[0].materialIndex = 1; expect_refusal("sphere material", b, "sphere.materialIndex out of range"); }
    {   // rt_update_objects' own refusals, against an accepted scene
        const Built b = small_tree();
        const MeshLayout m = layout_meshes(b.arrays());
        g_where = "refusal: object list";
        CHECK(m.error.empty(), "%s", m.error.c_str());
        RenderObject o = object(1);
        CHECK(layout_objects(&o, 1, m.rootOf, 1, 48, 0).error == "object.bvhIndex does not point at a mesh root of the uploaded BVH", "bvhIndex at a leaf");
        o = object(3);
        CHECK(layout_objects(&o, 1, m.rootOf, 1, 48, 0).error == "object.bvhIndex out of range", "bvhIndex past the nodes");
        o = object(0, 1);
        CHECK(layout_objects(&o, 1, m.rootOf, 1, 48, 0).error == "object.materialIndex out of range", "material 1 of 1");
        CHECK(layout_objects(&o, 1, m.rootOf, 0, 48, 0).error == "object.materialIndex out of range", "material 1 of none");
        o = object(0);
        CHECK(layout_objects(&o, 1, m.rootOf, 0, 48, 0).error.empty(), "material 0 before any material is uploaded");
    }
}

static void check_hand_built_meshes() {
    {   // a root that is a leaf of nine triangles: the reference goes through leafFirst
        g_where = "big leaf";
        Built b = base(9);
        b.nodes = {node(0, 9)};
        b.objects = {object(0)};
        const MeshLayout m = layout_meshes(b.arrays());
        check_meshes(b.arrays(), m);
        CHECK(m.error.empty() && bits(m.nodes[2 * (size_t)m.nodeRemap[0]].w) == (RT_LEAF_BIT | m.nodeRemap[0]) && m.rootOf[0].triTotal == 9, "big leaf root");
        check_objects_all(b.arrays(), b.objects, m);
    }
    {   // a big leaf below an interior node, next to a small one whose range does not touch it
        g_where = "non-contiguous mesh";
        Built b = base(12);
        b.nodes = {node(1, 0), node(0, 8), node(10, 2)};
        b.objects = {object(0)};
        const MeshLayout m = layout_meshes(b.arrays());
        check_meshes(b.arrays(), m);
        CHECK(m.error.empty() && m.rootOf[0].triFirst == 0 && m.rootOf[0].triTotal == 0xffffffffu, "triTotal %u", m.error.empty() ? m.rootOf[0].triTotal : 0u);
    }
}

// ---------------------------------------------------------------- spheres, emitters, maps, materials, textures
static void check_small_tables() {
    g_where = "spheres";
    {
        std::vector<Sphere> s(36, Sphere{});
        for (uint32_t i = 0; i < 36; i++) { s[i].position[0] = (float)(i % 5); s[i].radius = 0.5f; s[i].materialIndex = i % 3; }  // spheres 5.. repeat 0..4
        s[7].position[1] = -0.f;    // equal to sphere 2 as a number, not bit for bit: still tested
        s[9].radius = 0.25f;
        const SphereLayout l = layout_spheres(s.data(), 36);
        uint32_t want = 0;
        for (uint32_t i = 0; i < 32; i++) {
            bool repeat = false;
            for (uint32_t k = 0; k < i; k++) repeat = repeat || (memcmp(s[i].position, s[k].position, 12) == 0 && bits(s[i].radius) == bits(s[k].radius));
            if (!repeat) want |= 1u << i;
        }
        CHECK(l.testMask == want && want == (0x1fu | 1u << 7 | 1u << 9), "sphereTestMask %x, expected %x", l.testMask, want);
        for (uint32_t i = 0; i < 36; i++) CHECK(same4(l.spheres[i], make_float4(s[i].position[0], s[i].position[1], s[i].position[2], s[i].radius)) && l.mat[i] == s[i].materialIndex, "sphere %u", i);
        const SphereLayout none = layout_spheres(nullptr, 0);
        CHECK(none.testMask == 0 && none.spheres.size() == 1 && none.mat.size() == 1, "no spheres");
    }

    g_where = "emitters";
    {
        // materials: 0 plain, 1 emissive, 2 emissive. Meshes: root 0 with 30 triangles from 4, root 1 with 3 from 40, root 2 not contiguous
        std::vector<RootInfo> rootOf(3, RootInfo{0, 0, {0, 0, 0}, {0, 0, 0}, 0, 0});
        rootOf[0].triFirst = 4; rootOf[0].triTotal = 30;
        rootOf[1].triFirst = 40; rootOf[1].triTotal = 3;
        rootOf[2].triTotal = 0xffffffffu;
        SceneSources src;
        RayMaterial plain, glow;
        rt_material_default(&plain);
        glow = plain;
        glow.emissionColor[0] = glow.emissionColor[1] = glow.emissionColor[2] = 1.f; glow.emissionStrength = 2.f;
        src.mats = {plain, glow, glow};
        src.sphereMat = {0, 1, 0, 2};
        src.objMat = {0, 1, 0}; src.objRoot = {1, 0, 0}; src.objSampler = {0, 0, 0};
        EmitterLayout e = layout_emitters(src, rootOf, 0);
        CHECK(e.mode == 1 && e.sphereMask == 0xau && e.tris.size() == 30, "mode %u mask %x, %zu triangles", e.mode, e.sphereMask, e.tris.size());
        for (size_t k = 0; k < e.tris.size(); k++) CHECK(e.tris[k].x == 1 && e.tris[k].y == 4 + k, "entry %zu", k);
        SceneSources s2 = src;
        s2.objMat[0] = 2;   // 3 more triangles: 33 > RT_EMIT_MAX_TRIS
        e = layout_emitters(s2, rootOf, 0);
        CHECK(RT_EMIT_MAX_TRIS == 32 && e.mode == 0 && e.tris.empty() && e.sphereMask == 0, "more than RT_EMIT_MAX_TRIS triangles: mode %u", e.mode);
        s2 = src; s2.objMat = {2, 0, 0}; s2.objRoot = {1, 0, 0};   // the three-triangle mesh alone
        e = layout_emitters(s2, rootOf, 0);
        CHECK(e.mode == 1 && e.tris.size() == 3 && e.tris[0].x == 0 && e.tris[0].y == 40, "small emitter: mode %u, %zu", e.mode, e.tris.size());
        s2 = src; s2.objRoot[1] = 2;   // an emitter whose triangles are not one range
        CHECK(layout_emitters(s2, rootOf, 0).mode == 0, "non-contiguous emitter");
        s2 = src; s2.mats[0].emissionColor[1] = 3e38f; s2.mats[0].emissionStrength = 10.f;   // the product overflows, on a material nothing uses
        CHECK(layout_emitters(s2, rootOf, 0).mode == 0, "non-finite emission product");
        s2 = src; s2.mats[0].emissionColor[2] = NAN;
        CHECK(layout_emitters(s2, rootOf, 0).mode == 0, "NaN emission");
        s2 = src; s2.sphereMat.assign(33, 0); s2.sphereMat[31] = 1;
        e = layout_emitters(s2, rootOf, 0);
        CHECK(e.mode == 1 && e.sphereMask == 0x80000000u, "emissive sphere 31: mode %u mask %x", e.mode, e.sphereMask);
        s2.sphereMat[32] = 1;
        CHECK(layout_emitters(s2, rootOf, 0).mode == 0, "emissive sphere 32");
        s2 = src; s2.mats[1].alphaIndex = 1;
        CHECK(layout_emitters(s2, rootOf, 2).mode == 0, "emitter with a bound alpha map");
        CHECK(layout_emitters(s2, rootOf, 1).mode == 1, "emitter whose alpha slot is beyond the texture table");
        s2 = src; s2.mats.clear();
        CHECK(layout_emitters(s2, rootOf, 0).mode == 0, "no materials");
    }

    g_where = "maps";
    {
        SceneSources src;
        RayMaterial m;
        rt_material_default(&m);
        src.mats.assign(4, m);
        src.mats[0].alphaIndex = 0; src.mats[1].metalnessIndex = 1; src.mats[2].bumpIndex = 2; src.mats[3].alphaIndex = 2;
        src.objMat = {0, 1, 2, 3, 0, 9}; src.objRoot.assign(6, 0); src.objSampler = {0, 0, 0, 1, 1, 0};
        const uint32_t wantFlags[4] = {0u, RT_MAP_ALPHA, RT_MAP_ALPHA | RT_MAP_METALNESS, RT_MAP_ALPHA | RT_MAP_METALNESS | RT_MAP_BUMP};
        for (uint32_t texCount = 0; texCount <= 3; texCount++) {
            const MapLayout l = layout_maps(src, texCount);
            CHECK(l.mapFlags == wantFlags[texCount], "mapFlags %x with %u textures", l.mapFlags, texCount);
            const uint32_t want[6] = {texCount > 0 ? 0u : RT_OBJALPHA_NONE, RT_OBJALPHA_NONE, RT_OBJALPHA_NONE, texCount > 2 ? (2u | RT_OBJALPHA_CLAMP) : RT_OBJALPHA_NONE,
                                      texCount > 0 ? (0u | RT_OBJALPHA_CLAMP) : RT_OBJALPHA_NONE, RT_OBJALPHA_NONE};
            for (int i = 0; i < 6; i++) CHECK(l.objAlpha[i] == want[i], "objAlpha[%d] = %x with %u textures", i, l.objAlpha[i], texCount);
        }
        CHECK(layout_maps(SceneSources{}, 4).objAlpha == std::vector<uint32_t>(1, RT_OBJALPHA_NONE), "no objects");
    }

    g_where = "materials";
    {
        RayMaterial m[2];
        rt_material_default(&m[0]);
        m[1] = m[0];
        m[1].albedo[1] = 0.25f; m[1].reflectance = 0.5f; m[1].emissionColor[2] = 3.f; m[1].emissionStrength = 4.f; m[1].ior = 1.5f;
        m[1].albedoIndex = 3; m[1].metalnessIndex = -1; m[1].bumpIndex = 7; m[1].alphaIndex = 5;
        const std::vector<float4> t = layout_materials(m, 2);
        CHECK(t.size() == 6 && same4(t[3], make_float4(m[1].albedo[0], 0.25f, m[1].albedo[2], 0.5f)) && same4(t[4], make_float4(m[1].emissionColor[0], m[1].emissionColor[1], 3.f, 4.f)) &&
              bits(t[5].x) == bits(1.5f) && bits(t[5].y) == 3u && bits(t[5].z) == 0xffffffffu && bits(t[5].w) == 7u, "material rows");
        CHECK(layout_materials(nullptr, 0).size() == 3, "no materials");
    }

    g_where = "textures";
    {
        std::vector<uint8_t> px(4 * 6 + 4 * 2);
        for (size_t i = 0; i < px.size(); i++) px[i] = (uint8_t)(i * 7 + 1);
        RtTexture tex[2] = {{3, 2, px.data()}, {1, 2, px.data() + 24}};
        TextureLayout l = layout_textures(tex, 2);
        CHECK(l.error.empty() && l.info.size() == 2 && l.texels.size() == 8 && memcmp(l.texels.data(), px.data(), px.size()) == 0, "texels");
        CHECK(l.info[0].x == 0 && l.info[0].y == 3 && l.info[0].z == 2 && l.info[1].x == 6 && l.info[1].y == 1 && l.info[1].z == 2, "texInfo");
        tex[1].height = 0;
        CHECK(layout_textures(tex, 2).error == "texture 1 is empty", "empty texture");
        CHECK(layout_textures(tex, RT_MAX_TEXTURES + 1).error == "more than RT_MAX_TEXTURES textures", "too many");
        l = layout_textures(nullptr, 0);
        CHECK(l.error.empty() && l.info.size() == 1 && l.texels.size() == 1, "no textures");
    }
}

int main(int argc, char** argv) {
    const std::string assets = argc > 1 ? argv[1] : "assets";

    {
        g_where = "cornell";
        rt_scene* s = nullptr;
        RtSceneArrays a;
        if (rt_scene_create(&s) || rt_scene_prepare_default(s, assets.c_str()) || rt_scene_get_arrays(s, &a)) { fprintf(stderr, "no Cornell scene: %s\n", s ? rt_scene_last_error(s) : ""); return 2; }
        const MeshLayout m = layout_meshes(a);
        check_meshes(a, m);
        const std::vector<RenderObject> o(a.objects, a.objects + a.objectCount);
        const ObjectFacts f = check_objects_all(a, o, m);
        printf("cornell: %u objects, %u general, %u nodes (%u hot), depth %u\n", a.objectCount, f.general, m.nodeCount, m.hotNodes, m.maxLeafDepth);
        rt_scene_destroy(s);
    }
    {
        g_where = "cornell + 70 placed";
        rt_scene* s = nullptr;
        if (rt_scene_create(&s) || rt_scene_prepare_default(s, assets.c_str())) return 2;
        float cube[12 * 9], cubeN[12 * 9];
        {   // two triangles per face of [-1, 1]^3
            int t = 0;
            for (int axis = 0; axis < 3; axis++)
                for (int side = -1; side <= 1; side += 2) {
                    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
                    const float q[4][2] = {{-1, -1}, {1, -1}, {1, 1}, {-1, 1}};
                    static const int corners[2][3] = {{0, 1, 2}, {0, 2, 3}};
                    for (const auto& c : corners) {
                        for (int k = 0; k < 3; k++) {
                            float* p = &cube[(t * 3 + k) * 3];
                            p[axis] = (float)side; p[u] = q[c[k]][0]; p[v] = q[c[k]][1];
                            float* nn = &cubeN[(t * 3 + k) * 3];
                            nn[axis] = (float)side; nn[u] = 0.f; nn[v] = 0.f;
                        }
                        t++;
                    }
                }
        }
        const float tri[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, triN[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
        RtPlacement identity;
        rt_placement_default(&identity);
        // identity placements first, so that the mask window starts behind them
        for (int k = 0; k < 4; k++)
            if (rt_scene_add_mesh(s, k % 2 ? "tri" : "cube", k % 2 ? tri : cube, k % 2 ? triN : cubeN, nullptr, k % 2 ? 1 : 12, &identity, k) < 0) { fprintf(stderr, "add_mesh: %s\n", rt_scene_last_error(s)); return 2; }
        for (int k = 0; k < 70; k++) {
            RtPlacement p = identity;
            p.position[0] = -0.8f + 0.023f * k; p.position[1] = 0.3f - 0.011f * k; p.position[2] = 0.1f * (k % 7);
            p.rotation[0] = 11.f * k; p.rotation[1] = 7.f * k + 3.f; p.rotation[2] = 29.f * k;
            p.scale[0] = 0.05f + 0.001f * k; p.scale[1] = 0.07f; p.scale[2] = 0.04f + 0.002f * (k % 5);
            p.samplerIndex = k % 2;
            if (rt_scene_add_mesh(s, k % 3 == 2 ? "tri" : "cube", k % 3 == 2 ? tri : cube, k % 3 == 2 ? triN : cubeN, nullptr, k % 3 == 2 ? 1 : 12, &p, k % 6) < 0) { fprintf(stderr, "add_mesh: %s\n", rt_scene_last_error(s)); return 2; }
        }
        RtSceneArrays a;
        if (rt_scene_get_arrays(s, &a)) return 2;
        const MeshLayout m = layout_meshes(a);
        check_meshes(a, m);
        // identity transforms first, then the placed objects: the mask window starts at object 4 and ends inside the placed ones
        std::vector<RenderObject> o(a.objects, a.objects + a.objectCount);
        std::stable_partition(o.begin(), o.end(), [](const RenderObject& r) {
            static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            return memcmp(r.transformMatrix, ident, sizeof ident) == 0;
        });
        const ObjectFacts f = check_objects_all(a, o, m);
        uint32_t leafRoots = 0;
        for (const RenderObject& r : o) leafRoots += a.bvhNodes[r.bvhIndex].triCount != 0;
        printf("cornell + 70 placed: %u objects, %u general, maskBase %u, %u general beyond the window, %u leaf roots, %u nodes (%u hot)\n",
               a.objectCount, f.general, f.maskBase, f.beyondWindow, leafRoots, m.nodeCount, m.hotNodes);
        CHECK(f.maskBase == 4 && f.beyondWindow > 0 && f.general >= 70 && leafRoots > 0 && (a.objectCount & 1u), "the scene does not reach the cases it is built for");
        {   // ... and as the scene has them
            g_where = "cornell + 70 placed, scene order";
            check_objects_all(a, std::vector<RenderObject>(a.objects, a.objects + a.objectCount), m);
        }
        rt_scene_destroy(s);
    }
    check_hand_built_meshes();
    check_refusals();
    check_small_tables();

    return check_finish("scene layout ok");
}
