// mesh_refit_check.cpp — deforming meshes in place (ray_tracer_amd/csrc/mesh_refit.h) checked on the CPU: the refit rule against the
// builder's own boxes, the refit plan against the device numbering, rt_scene_update_points against the vertices it was given, and
// every refusal. It also writes, per deformed case, the arrays before and after into <out dir>, where tests/test_mesh_refit_host.py
// restates the rule in numpy and compares bit for bit.   mesh_refit_check <assets dir> <out dir>
#include "mesh_refit.h"
#include "scene_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>
#include "check.h"

static std::string g_assets, g_out;

// the four scenes: 0 Cornell, 1 Cornell + cube.obj, 2 Cornell + bunny.obj, 3 one mesh (the bunny) used by two objects
static const char* kSceneNames[4] = {"cornell", "cornell_cube", "cornell_bunny", "two_bunnies"};
static rt_scene* make_scene(int which) {
    rt_scene* s = nullptr;
    if (rt_scene_create(&s) || rt_scene_prepare_default(s, g_assets.c_str())) { fprintf(stderr, "no Cornell scene: %s\n", s ? rt_scene_last_error(s) : ""); exit(2); }
    RtPlacement p;
    rt_placement_default(&p);
    p.position[1] = 0.53f; p.scale[0] = p.scale[1] = p.scale[2] = 0.7f; p.rotation[1] = 25.f;
    int rc = 0;
    if (which == 1) rc = rt_scene_read_obj(s, (g_assets + "/cube.obj").c_str(), &p, 1);
    if (which >= 2) rc = rt_scene_read_obj(s, (g_assets + "/bunny.obj").c_str(), &p, 1);
    if (which == 3 && rc == 0) { p.position[0] = 0.4f; p.rotation[2] = 40.f; p.scale[1] = 0.4f; rc = rt_scene_read_obj(s, (g_assets + "/bunny.obj").c_str(), &p, 2); }
    if (rc != 0) { fprintf(stderr, "read_obj: %d %s\n", rc, rt_scene_last_error(s)); exit(2); }
    return s;
}
static RtSceneArrays arrays_of(const rt_scene* s) {
    RtSceneArrays a;
    if (rt_scene_get_arrays(s, &a)) exit(2);
    return a;
}

static bool same_box_value(const BVHNode& a, const BVHNode& b) {
    return a.boundsX[0] == b.boundsX[0] && a.boundsX[1] == b.boundsX[1] && a.boundsY[0] == b.boundsY[0] && a.boundsY[1] == b.boundsY[1] &&
           a.boundsZ[0] == b.boundsZ[0] && a.boundsZ[1] == b.boundsZ[1];
}

// ---- the rule is the builder's: refitting the unchanged points gives every node the builder's box (by value)
static void check_unchanged(const RtSceneArrays& a) {
    std::string error;
    const std::vector<RefitMesh> meshes = refit_meshes(a, error);
    CHECK(error.empty(), "%s", error.c_str());
    std::vector<BVHNode> nodes(a.bvhNodes, a.bvhNodes + a.bvhNodeCount);
    for (BVHNode& n : nodes) n.boundsX[0] = n.boundsX[1] = n.boundsY[0] = n.boundsY[1] = n.boundsZ[0] = n.boundsZ[1] = std::numeric_limits<float>::quiet_NaN();
    for (const RefitMesh& m : meshes) refit_nodes_host(nodes.data(), a.triangles, a.triPoints, m.root);
    std::set<uint32_t> roots;
    for (uint32_t i = 0; i < a.objectCount; i++) roots.insert(a.objects[i].bvhIndex);
    CHECK(meshes.size() == roots.size(), "%zu meshes, %zu roots", meshes.size(), roots.size());
    for (uint32_t n = 0; n < a.bvhNodeCount; n++) {
        CHECK(same_box_value(nodes[n], a.bvhNodes[n]), "node %u: refit (%g %g %g)-(%g %g %g), builder (%g %g %g)-(%g %g %g)", n, nodes[n].boundsX[0], nodes[n].boundsY[0],
              nodes[n].boundsZ[0], nodes[n].boundsX[1], nodes[n].boundsY[1], nodes[n].boundsZ[1], a.bvhNodes[n].boundsX[0], a.bvhNodes[n].boundsY[0], a.bvhNodes[n].boundsZ[0],
              a.bvhNodes[n].boundsX[1], a.bvhNodes[n].boundsY[1], a.bvhNodes[n].boundsZ[1]);
        CHECK(nodes[n].index == a.bvhNodes[n].index && nodes[n].triCount == a.bvhNodes[n].triCount, "node %u: topology changed", n);
    }
}

// ---- the plan against the scene and the device numbering
static void check_plan(const RtSceneArrays& a) {
    const MeshLayout l = layout_meshes(a);
    CHECK(l.error.empty(), "%s", l.error.c_str());
    const RefitPlan p = plan_refit(a, l);
    CHECK(p.error.empty(), "%s", p.error.c_str());
    if (!l.error.empty() || !p.error.empty()) return;
    CHECK(p.pointCount == a.triPointCount, "%u", p.pointCount);
    std::vector<int> seenInterior(l.nodeCount, 0), seenLeaf(l.nodeCount, 0);
    std::vector<uint32_t> refOf(l.nodeCount, 0xffffffffu);
    for (uint32_t n = 0; n < a.bvhNodeCount; n++) refOf[l.nodeRemap[n]] = n;
    uint32_t hotInLists = 0;
    for (const RefitMesh& m : p.meshes) {
        const RootInfo& r = l.rootOf[m.root];
        CHECK(r.idx != 0xffffffffu, "mesh %u is no root of the layout", m.root);
        CHECK(m.rootDev == l.nodeRemap[m.root], "root %u", m.root);
        CHECK(m.triFirst == r.triFirst && m.triCount == r.triTotal, "mesh %u: triangles [%u, +%u), layout [%u, +%u)", m.root, m.triFirst, m.triCount, r.triFirst, r.triTotal);
        uint32_t lo = 0xffffffffu, hi = 0;
        for (uint32_t t = m.triFirst; t < m.triFirst + m.triCount; t++)
            for (uint32_t v : {a.triangles[t].v0, a.triangles[t].v1, a.triangles[t].v2}) { lo = std::min(lo, v); hi = std::max(hi, v); }
        CHECK(m.pointFirst == lo && m.pointEnd == hi + 1, "mesh %u: points [%u, %u), its triangles use [%u, %u]", m.root, m.pointFirst, m.pointEnd, lo, hi);
        // offsets of the levels: increasing, from 0 to the count; the last level is the root alone (or there is none: a root leaf)
        const uint32_t* lv = p.levels.data() + m.levelOff;
        CHECK(lv[0] == 0 && lv[m.levelCount] == m.interiorCount, "mesh %u: level offsets", m.root);
        for (uint32_t k = 0; k < m.levelCount; k++) CHECK(lv[k] < lv[k + 1], "mesh %u: empty level %u", m.root, k);
        const bool rootIsLeaf = a.bvhNodes[m.root].triCount != 0;
        CHECK(rootIsLeaf == (m.interiorCount == 0), "mesh %u", m.root);
        if (rootIsLeaf) CHECK(m.inlineLeaves + m.bigLeaves == 1 && p.leaves[m.leafOff] == m.rootDev, "mesh %u: a root leaf is its own only leaf", m.root);
        else CHECK(lv[m.levelCount] - lv[m.levelCount - 1] == 1 && p.interior[m.interiorOff + m.interiorCount - 1] == m.rootDev, "mesh %u: the last level is the root", m.root);
        // every child sits at a deeper offset than its parent (an earlier level), or is a leaf of this mesh
        std::vector<uint32_t> levelOf(l.nodeCount, 0xffffffffu);
        for (uint32_t k = 0; k < m.levelCount; k++)
            for (uint32_t i = lv[k]; i < lv[k + 1]; i++) levelOf[p.interior[m.interiorOff + i]] = k;
        std::set<uint32_t> myLeaves(p.leaves.begin() + m.leafOff, p.leaves.begin() + m.leafOff + m.inlineLeaves + m.bigLeaves);
        CHECK(myLeaves.size() == m.inlineLeaves + m.bigLeaves, "mesh %u: a leaf twice", m.root);
        for (uint32_t i = 0; i < m.interiorCount; i++) {
            const uint32_t dev = p.interior[m.interiorOff + i];
            CHECK(dev < l.nodeCount && refOf[dev] != 0xffffffffu, "interior index %u", dev);
            seenInterior[dev]++;
            hotInLists += dev < l.hotNodes;
            const BVHNode& b = a.bvhNodes[refOf[dev]];
            CHECK(b.triCount == 0, "device node %u in the interior list is a leaf", dev);
            for (uint32_t c : {l.nodeRemap[b.index], l.nodeRemap[b.index + 1]}) {
                if (a.bvhNodes[refOf[c]].triCount) CHECK(myLeaves.count(c) == 1, "leaf child %u of %u is not in the mesh's leaves", c, dev);
                else CHECK(levelOf[c] != 0xffffffffu && levelOf[c] < levelOf[dev], "child %u (level %u) of %u (level %u) is not deeper", c, levelOf[c], dev, levelOf[dev]);
            }
        }
        for (uint32_t i = 0; i < m.inlineLeaves + m.bigLeaves; i++) {
            const uint32_t dev = p.leaves[m.leafOff + i];
            seenLeaf[dev]++;
            hotInLists += dev < l.hotNodes;
            const BVHNode& b = a.bvhNodes[refOf[dev]];
            CHECK(b.triCount != 0, "device node %u in the leaf list is interior", dev);
            uint32_t w0;
            memcpy(&w0, &l.nodes[2 * (size_t)dev].w, 4);
            const bool isInline = ((w0 >> RT_LEAF_CNT_SHIFT) & 7u) != 0;
            CHECK(isInline == (i < m.inlineLeaves), "leaf %u: the form of its W0 and its place in the list", dev);
            if (isInline) CHECK(((w0 >> RT_LEAF_CNT_SHIFT) & 7u) == b.triCount && (w0 & RT_LEAF_IDX_MASK) == b.index, "leaf %u: W0", dev);
            else CHECK(l.leafFirst[dev] == b.index, "leaf %u: leafFirst", dev);
            CHECK(b.index >= m.triFirst && b.index + b.triCount <= m.triFirst + m.triCount, "leaf %u outside its mesh's triangles", dev);
        }
    }
    // complete: every node of the scene that a mesh reaches is in exactly one list, once
    for (uint32_t n = 0; n < a.bvhNodeCount; n++) {
        const uint32_t dev = l.nodeRemap[n];
        if (a.bvhNodes[n].triCount) CHECK(seenLeaf[dev] == 1 && seenInterior[dev] == 0, "leaf %u (device %u): %d / %d", n, dev, seenLeaf[dev], seenInterior[dev]);
        else CHECK(seenInterior[dev] == 1 && seenLeaf[dev] == 0, "interior node %u (device %u): %d / %d", n, dev, seenInterior[dev], seenLeaf[dev]);
    }
    // the lists survive the hot-pair renumbering: every hot slot is a node of some mesh and was found through a list
    CHECK(hotInLists == l.hotNodes, "%u of %u hot nodes in the lists", hotInLists, l.hotNodes);
}

// ---- deformations through rt_scene_update_points
static uint32_t g_rng = 1;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return (float)((g_rng >> 8) & 0xffff) / 65535.f - 0.5f; }

static void dump(const std::string& name, const void* p, size_t bytes) {
    FILE* f = fopen((g_out + "/" + name).c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", name.c_str()); exit(2); }
    fclose(f);
}

static void check_deformed(int which, int kind) {   // kind 0: all points, 1: a sub-range of the last mesh, 2: a range that straddles two meshes
    rt_scene* s = make_scene(which);
    RtSceneArrays a = arrays_of(s);
    std::string error;
    const std::vector<RefitMesh> meshes = refit_meshes(a, error);
    CHECK(error.empty() && !meshes.empty(), "%s", error.c_str());
    uint32_t first = 0, count = a.triPointCount;
    if (kind == 1) { const RefitMesh& m = meshes.back(); const uint32_t n = m.pointEnd - m.pointFirst; first = m.pointFirst + n / 3; count = std::max(1u, n / 4); }
    if (kind == 2) {   // two meshes whose point ranges follow each other
        size_t k = 0;
        while (k + 1 < meshes.size() && meshes[k].pointEnd != meshes[k + 1].pointFirst) k++;
        CHECK(k + 1 < meshes.size(), "no two meshes with adjacent point ranges");
        if (k + 1 >= meshes.size()) { rt_scene_destroy(s); return; }
        first = meshes[k].pointEnd - 2; count = 5;
    }
    const std::vector<BVHNode> before(a.bvhNodes, a.bvhNodes + a.bvhNodeCount);
    const std::vector<TrianglePoint> oldPoints(a.triPoints, a.triPoints + a.triPointCount);
    std::vector<TrianglePoint> np(oldPoints.begin() + first, oldPoints.begin() + first + count);
    g_rng = 77u + 10u * which + kind;
    const float amp = kind == 0 ? 0.2f : 0.6f;
    for (TrianglePoint& p : np) {
        for (int k = 0; k < 3; k++) p.position[k] += amp * rnd();
        for (int k = 0; k < 4; k++) p.normal[k] += 0.1f * rnd();
        p.position[3] += 0.05f * rnd();
    }
    np[0].position[0] = -0.f; if (count > 1) np[1].position[0] = 0.f;   // zeros of both signs among the vertices
    const int rc = rt_scene_update_points(s, np.data(), first, count);
    CHECK(rc == 0, "%s", rt_scene_last_error(s));
    a = arrays_of(s);
    CHECK(memcmp(a.triPoints + first, np.data(), count * sizeof(TrianglePoint)) == 0, "the new points are not in the scene");
    for (uint32_t i = 0; i < a.triPointCount; i++)
        if (i < first || i >= first + count) CHECK(memcmp(&a.triPoints[i], &oldPoints[i], sizeof(TrianglePoint)) == 0, "point %u outside the range changed", i);
    const std::vector<uint32_t> touched = touched_meshes(meshes, first, count);
    CHECK(!touched.empty() && (kind != 0 || touched.size() == meshes.size()) && (kind != 2 || touched.size() >= 2), "%zu meshes touched", touched.size());
    std::vector<uint32_t> touchedRoots;
    std::vector<uint8_t> inTouched(a.bvhNodeCount, 0);
    for (uint32_t k : touched) {
        const RefitMesh& m = meshes[k];
        touchedRoots.push_back(m.root);
        std::vector<uint32_t> st(1, m.root);
        while (!st.empty()) {
            const uint32_t n = st.back(); st.pop_back();
            inTouched[n] = 1;
            if (a.bvhNodes[n].triCount == 0) { st.push_back(a.bvhNodes[n].index); st.push_back(a.bvhNodes[n].index + 1); }
        }
        // the root box is the min / max over the mesh's new vertices
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t t = m.triFirst; t < m.triFirst + m.triCount; t++)
            for (uint32_t v : {a.triangles[t].v0, a.triangles[t].v1, a.triangles[t].v2})
                for (int d = 0; d < 3; d++) { lo[d] = std::min(lo[d], a.triPoints[v].position[d]); hi[d] = std::max(hi[d], a.triPoints[v].position[d]); }
        const BVHNode& r = a.bvhNodes[m.root];
        CHECK(r.boundsX[0] == lo[0] && r.boundsY[0] == lo[1] && r.boundsZ[0] == lo[2] && r.boundsX[1] == hi[0] && r.boundsY[1] == hi[1] && r.boundsZ[1] == hi[2],
              "root %u: (%g %g %g)-(%g %g %g), vertices (%g %g %g)-(%g %g %g)", m.root, r.boundsX[0], r.boundsY[0], r.boundsZ[0], r.boundsX[1], r.boundsY[1], r.boundsZ[1], lo[0],
              lo[1], lo[2], hi[0], hi[1], hi[2]);
    }
    for (uint32_t n = 0; n < a.bvhNodeCount; n++) {
        CHECK(a.bvhNodes[n].index == before[n].index && a.bvhNodes[n].triCount == before[n].triCount, "node %u: topology changed", n);
        if (!inTouched[n]) CHECK(memcmp(&a.bvhNodes[n], &before[n], sizeof(BVHNode)) == 0, "node %u of an untouched mesh changed", n);
    }
    const std::string tag = std::string(kSceneNames[which]) + "_" + std::to_string(kind) + "_";
    dump(tag + "triangles.bin", a.triangles, (size_t)a.triangleCount * sizeof(Triangle));
    dump(tag + "points.bin", a.triPoints, (size_t)a.triPointCount * sizeof(TrianglePoint));
    dump(tag + "nodes_before.bin", before.data(), before.size() * sizeof(BVHNode));
    dump(tag + "nodes_after.bin", a.bvhNodes, (size_t)a.bvhNodeCount * sizeof(BVHNode));
    dump(tag + "roots.bin", touchedRoots.data(), touchedRoots.size() * sizeof(uint32_t));
    rt_scene_destroy(s);
}

// ---- refusals: each with its message, the arrays unmodified
static void check_refusals() {
    rt_scene* s = make_scene(1);
    RtSceneArrays a = arrays_of(s);
    const std::vector<TrianglePoint> points(a.triPoints, a.triPoints + a.triPointCount);
    const std::vector<BVHNode> nodes(a.bvhNodes, a.bvhNodes + a.bvhNodeCount);
    auto unmodified = [&]() {
        const RtSceneArrays b = arrays_of(s);
        return b.triPointCount == points.size() && b.bvhNodeCount == nodes.size() && memcmp(b.triPoints, points.data(), points.size() * sizeof(TrianglePoint)) == 0 &&
               memcmp(b.bvhNodes, nodes.data(), nodes.size() * sizeof(BVHNode)) == 0;
    };
    auto refused = [&](const TrianglePoint* p, uint32_t first, uint32_t count, const char* message) {
        const int rc = rt_scene_update_points(s, p, first, count);
        CHECK(rc < 0 && strstr(rt_scene_last_error(s), message), "rc %d, \"%s\", expected \"%s\"", rc, rt_scene_last_error(s), message);
        CHECK(unmodified(), "a refused update changed the scene (%s)", message);
    };
    std::vector<TrianglePoint> np(points.begin(), points.begin() + 4);
    refused(np.data(), a.triPointCount - 3, 4, "run past the scene's");
    refused(np.data(), 0xfffffffeu, 4, "run past the scene's");
    refused(nullptr, 0, 4, "points is null");
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), INFINITY, -INFINITY})
        for (int k = 0; k < 3; k++) {
            std::vector<TrianglePoint> q = np;
            q[2].position[k] = bad;
            refused(q.data(), 5, 4, "the position of point 7 is not finite");
        }
    {   // uv and normals may hold anything: only positions feed the boxes
        std::vector<TrianglePoint> q = np;
        q[1].position[3] = std::numeric_limits<float>::quiet_NaN();
        CHECK(check_update_points("f", a.triPointCount, q.data(), 0, 4).empty(), "a NaN u was refused");
    }
    CHECK(rt_scene_update_points(s, nullptr, 0, 0) == 0 && unmodified(), "count 0 with null points is a no-op that succeeds");
    CHECK(rt_scene_update_points(s, np.data(), a.triPointCount, 0) == 0 && unmodified(), "count 0 at the end is a no-op that succeeds");
    CHECK(rt_scene_update_points(nullptr, np.data(), 0, 1) < 0, "null scene");

    // a mesh that shares children with another mesh, and one whose triangles are not one contiguous range: refit_meshes and
    // plan_refit refuse the arrays, rt_scene_update_points refuses a scene that holds them and leaves it as it is
    uint32_t interiorRoot = 0xffffffffu;
    for (uint32_t i = 0; i < a.objectCount; i++)
        if (nodes[a.objects[i].bvhIndex].triCount == 0) interiorRoot = a.objects[i].bvhIndex;
    CHECK(interiorRoot != 0xffffffffu, "no mesh with an interior root");
    if (interiorRoot != 0xffffffffu) {
        std::string error;
        {
            std::vector<RenderObject> objs(a.objects, a.objects + a.objectCount);
            RtSceneArrays b = a;
            objs.push_back(objs[0]);
            objs.back().bvhIndex = nodes[interiorRoot].index;   // an object whose mesh is the first child of another mesh's root
            b.objects = objs.data(); b.objectCount = (uint32_t)objs.size();
            CHECK(refit_meshes(b, error).empty() && error.find("shares BVH nodes") != std::string::npos, "\"%s\"", error.c_str());
            const MeshLayout l = layout_meshes(b);
            CHECK(l.error.empty(), "%s", l.error.c_str());
            if (l.error.empty()) { const RefitPlan p = plan_refit(b, l); CHECK(p.error.find("shares BVH nodes") != std::string::npos, "\"%s\"", p.error.c_str()); }
        }
        // the leaf that holds the mesh's first triangle loses its last one: a hole in the mesh's range, as long as it has another leaf
        const std::vector<RefitMesh> meshes = refit_meshes(a, error);
        uint32_t firstLeaf = 0xffffffffu, leaves = 0;
        for (const RefitMesh& m : meshes) {
            if (m.root != interiorRoot) continue;
            std::vector<uint32_t> st(1, m.root);
            while (!st.empty()) {
                const uint32_t n = st.back(); st.pop_back();
                if (nodes[n].triCount == 0) { st.push_back(nodes[n].index); st.push_back(nodes[n].index + 1); continue; }
                leaves++;
                if (nodes[n].index == m.triFirst) firstLeaf = n;
            }
        }
        CHECK(firstLeaf != 0xffffffffu && leaves > 1 && nodes[firstLeaf].triCount > 1, "leaf %u of %u leaves: the tree cannot be broken this way", firstLeaf, leaves);
        if (firstLeaf != 0xffffffffu && leaves > 1 && nodes[firstLeaf].triCount > 1) {
            std::vector<BVHNode> holed(nodes);
            holed[firstLeaf].triCount -= 1;
            RtSceneArrays g = a;
            g.bvhNodes = holed.data();
            CHECK(refit_meshes(g, error).empty() && error.find("not one contiguous range") != std::string::npos, "\"%s\"", error.c_str());
            const MeshLayout l = layout_meshes(g);
            CHECK(l.error.empty(), "%s", l.error.c_str());
            if (l.error.empty()) { const RefitPlan p = plan_refit(g, l); CHECK(p.error.find("not one contiguous range") != std::string::npos, "\"%s\"", p.error.c_str()); }

            // the same two through rt_scene_update_points, on scenes of their own (the scene's vectors edited behind its back)
            rt_scene* broken = make_scene(1);
            RtSceneHost& h = *rt_scene_host(broken);
            h.bvhNodes[firstLeaf].triCount -= 1;
            const std::vector<TrianglePoint> bp(h.triPoints);
            const std::vector<BVHNode> bn(h.bvhNodes);
            int rc = rt_scene_update_points(broken, np.data(), 0, 4);
            CHECK(rc < 0 && strstr(rt_scene_last_error(broken), "rt_scene_update_points: the triangles of a mesh are not one contiguous range"), "rc %d \"%s\"", rc, rt_scene_last_error(broken));
            CHECK(memcmp(h.triPoints.data(), bp.data(), bp.size() * sizeof(TrianglePoint)) == 0 && memcmp(h.bvhNodes.data(), bn.data(), bn.size() * sizeof(BVHNode)) == 0, "a refused update changed the scene");
            h.bvhNodes[firstLeaf].triCount += 1;
            h.objects.push_back(h.objects[0]);
            h.objects.back().bvhIndex = h.bvhNodes[interiorRoot].index;
            rc = rt_scene_update_points(broken, np.data(), 0, 4);
            CHECK(rc < 0 && strstr(rt_scene_last_error(broken), "rt_scene_update_points: a mesh shares BVH nodes with another mesh"), "rc %d \"%s\"", rc, rt_scene_last_error(broken));
            CHECK(memcmp(h.triPoints.data(), bp.data(), bp.size() * sizeof(TrianglePoint)) == 0, "a refused update changed the scene");
            h.bvhNodes[interiorRoot].index = (uint32_t)h.bvhNodes.size();   // a child index past the end
            h.objects.pop_back();
            rc = rt_scene_update_points(broken, np.data(), 0, 4);
            CHECK(rc < 0 && strstr(rt_scene_last_error(broken), "BVH child index out of range"), "rc %d \"%s\"", rc, rt_scene_last_error(broken));
            rt_scene_destroy(broken);
        }
    }
    // the kept list of meshes: a second update of the same scene gives what a first update of a fresh scene gives, and adding
    // geometry makes the list again
    {
        rt_scene* one = make_scene(1);
        rt_scene* two = make_scene(1);
        std::vector<TrianglePoint> q(points);
        for (TrianglePoint& p : q) p.position[1] += 0.125f;
        CHECK(rt_scene_update_points(one, points.data(), 0, (uint32_t)points.size()) == 0, "%s", rt_scene_last_error(one));
        CHECK(rt_scene_update_points(one, q.data(), 0, (uint32_t)q.size()) == 0, "%s", rt_scene_last_error(one));
        CHECK(rt_scene_update_points(two, q.data(), 0, (uint32_t)q.size()) == 0, "%s", rt_scene_last_error(two));
        RtSceneArrays x = arrays_of(one), y = arrays_of(two);
        CHECK(x.bvhNodeCount == y.bvhNodeCount && memcmp(x.bvhNodes, y.bvhNodes, x.bvhNodeCount * sizeof(BVHNode)) == 0, "the second update through the kept list differs");
        RtPlacement pl;
        rt_placement_default(&pl);
        pl.position[0] = 0.3f;
        for (rt_scene* sc : {one, two}) CHECK(rt_scene_read_obj(sc, (g_assets + "/bunny.obj").c_str(), &pl, 1) == 0, "%s", rt_scene_last_error(sc));
        x = arrays_of(one);
        std::vector<TrianglePoint> all(x.triPoints, x.triPoints + x.triPointCount);
        for (TrianglePoint& p : all) p.position[2] -= 0.25f;
        CHECK(rt_scene_update_points(one, all.data(), 0, (uint32_t)all.size()) == 0, "%s", rt_scene_last_error(one));
        x = arrays_of(one);
        std::string error;
        const std::vector<RefitMesh> ms = refit_meshes(x, error);
        std::vector<BVHNode> expect(x.bvhNodes, x.bvhNodes + x.bvhNodeCount);
        for (const RefitMesh& m : ms) refit_nodes_host(expect.data(), x.triangles, x.triPoints, m.root);
        CHECK(memcmp(expect.data(), x.bvhNodes, expect.size() * sizeof(BVHNode)) == 0, "after adding a mesh the update did not refit every mesh (a stale list)");
        rt_scene_destroy(one);
        rt_scene_destroy(two);
    }
    rt_scene_destroy(s);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: mesh_refit_check <assets dir> <out dir>\n"); return 2; }
    g_assets = argv[1]; g_out = argv[2];
    for (int which = 0; which < 4; which++) {
        rt_scene* s = make_scene(which);
        const RtSceneArrays a = arrays_of(s);
        g_where = std::string(kSceneNames[which]) + " unchanged";
        check_unchanged(a);
        g_where = std::string(kSceneNames[which]) + " plan";
        check_plan(a);
        rt_scene_destroy(s);
        for (int kind = 0; kind < 3; kind++) {
            g_where = std::string(kSceneNames[which]) + " deformed " + std::to_string(kind);
            check_deformed(which, kind);
        }
    }
    g_where = "refusals";
    check_refusals();
    return check_finish("mesh refit ok");
}
