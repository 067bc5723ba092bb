// mesh_refit.cpp — the refit plan, its checks and the host refit (mesh_refit.h). Host only.

#include "mesh_refit.h"

#include "scene_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace {

std::vector<uint32_t> mesh_roots(const RtSceneArrays& s) {
    std::vector<uint32_t> roots;
    for (uint32_t i = 0; i < s.objectCount; i++) roots.push_back(s.objects[i].bvhIndex);
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
    return roots;
}

struct Box3 {
    float lo[3] = {RT_REFIT_LO, RT_REFIT_LO, RT_REFIT_LO}, hi[3] = {RT_REFIT_HI, RT_REFIT_HI, RT_REFIT_HI};
    void grow(const float* plo, const float* phi) {
        for (int i = 0; i < 3; i++) {
            lo[i] = plo[i] < lo[i] ? plo[i] : lo[i];
            hi[i] = hi[i] < phi[i] ? phi[i] : hi[i];
        }
    }
};

}  // namespace

std::vector<RefitMesh> refit_meshes(const RtSceneArrays& s, std::string& error) {
    std::vector<RefitMesh> meshes;
    error.clear();
    const uint32_t nNodes = s.bvhNodeCount;
    std::vector<uint8_t> seen(nNodes, 0);
    std::vector<uint32_t> st;
    for (uint32_t root : mesh_roots(s)) {
        if (root >= nNodes) { error = "object.bvhIndex out of range"; return {}; }
        RefitMesh m;
        m.root = root;
        uint64_t triLo = ~0ull, triHi = 0, triSum = 0;
        uint32_t ptLo = 0xffffffffu, ptHi = 0;
        st.assign(1, root);
        while (!st.empty()) {
            const uint32_t nidx = st.back();
            st.pop_back();
            if (seen[nidx]) { error = "a mesh shares BVH nodes with another mesh: it cannot be refit on its own"; return {}; }
            seen[nidx] = 1;
            const BVHNode& b = s.bvhNodes[nidx];
            if (b.triCount == 0) {
                if ((uint64_t)b.index + 1 >= nNodes) { error = "BVH child index out of range"; return {}; }
                st.push_back(b.index);
                st.push_back(b.index + 1);
                continue;
            }
            if ((uint64_t)b.index + b.triCount > s.triangleCount) { error = "BVH leaf triangle range out of bounds"; return {}; }
            triLo = std::min<uint64_t>(triLo, b.index); triHi = std::max<uint64_t>(triHi, (uint64_t)b.index + b.triCount); triSum += b.triCount;
            for (uint32_t t = b.index; t < b.index + b.triCount; t++)
                for (uint32_t v : {s.triangles[t].v0, s.triangles[t].v1, s.triangles[t].v2}) {
                    if (v >= s.triPointCount) { error = "triangle point index out of range"; return {}; }
                    ptLo = std::min(ptLo, v); ptHi = std::max(ptHi, v);
                }
        }
        if (triSum != triHi - triLo) { error = "the triangles of a mesh are not one contiguous range: it cannot be refit"; return {}; }
        m.triFirst = (uint32_t)triLo; m.triCount = (uint32_t)triSum;
        m.pointFirst = ptLo; m.pointEnd = ptHi + 1;
        meshes.push_back(m);
    }
    return meshes;
}

RefitPlan plan_refit(const RtSceneArrays& s, const MeshLayout& l) {
    RefitPlan p;
    p.pointCount = s.triPointCount;
    p.meshes = refit_meshes(s, p.error);
    if (!p.error.empty()) return p;
    std::vector<uint32_t> level, next, big;
    std::vector<std::vector<uint32_t>> byDepth;
    for (RefitMesh& m : p.meshes) {
        m.rootDev = l.nodeRemap[m.root];
        m.leafOff = (uint32_t)p.leaves.size();
        byDepth.clear();
        big.clear();
        level.assign(1, m.root);
        while (!level.empty()) {   // breadth first: the interior nodes of every depth, the leaves by the form of their W0
            next.clear();
            byDepth.emplace_back();
            for (uint32_t nidx : level) {
                const BVHNode& b = s.bvhNodes[nidx];
                const uint32_t dev = l.nodeRemap[nidx];
                if (b.triCount == 0) {
                    byDepth.back().push_back(dev);
                    next.push_back(b.index);
                    next.push_back(b.index + 1);
                } else {
                    uint32_t w0;
                    const float4& lo = l.nodes[2 * (size_t)dev];
                    memcpy(&w0, &lo.w, 4);
                    if ((w0 >> RT_LEAF_CNT_SHIFT) & 7u) { p.leaves.push_back(dev); m.inlineLeaves++; }
                    else big.push_back(dev);
                }
            }
            level.swap(next);
        }
        p.leaves.insert(p.leaves.end(), big.begin(), big.end());
        m.bigLeaves = (uint32_t)big.size();
        while (!byDepth.empty() && byDepth.back().empty()) byDepth.pop_back();
        m.interiorOff = (uint32_t)p.interior.size();
        m.levelOff = (uint32_t)p.levels.size();
        for (size_t d = byDepth.size(); d-- > 0;) {
            if (byDepth[d].empty()) continue;   // (cannot happen above the deepest interior level; kept out of the launch list anyway)
            p.levels.push_back((uint32_t)p.interior.size() - m.interiorOff);
            p.interior.insert(p.interior.end(), byDepth[d].begin(), byDepth[d].end());
            m.levelCount++;
        }
        m.interiorCount = (uint32_t)p.interior.size() - m.interiorOff;
        p.levels.push_back(m.interiorCount);
    }
    return p;
}

std::string check_update_points(const char* fn, uint32_t pointCount, const TrianglePoint* points, uint32_t first, uint32_t count) {
    const std::string f = fn;
    if ((uint64_t)first + count > pointCount)
        return f + ": points [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) + ") run past the scene's " + std::to_string(pointCount) + " points";
    if (count && !points) return f + ": points is null";
    for (uint32_t i = 0; i < count; i++)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(points[i].position[k])) return f + ": the position of point " + std::to_string(first + i) + " is not finite";
    return "";
}

std::vector<uint32_t> touched_meshes(const std::vector<RefitMesh>& meshes, uint32_t first, uint32_t count) {
    std::vector<uint32_t> out;
    const uint64_t end = (uint64_t)first + count;
    for (size_t i = 0; i < meshes.size(); i++)
        if (count && meshes[i].pointFirst < end && first < meshes[i].pointEnd) out.push_back((uint32_t)i);
    return out;
}

void refit_nodes_host(BVHNode* nodes, const Triangle* triangles, const TrianglePoint* points, uint32_t root) {
    std::vector<uint32_t> order(1, root);   // parents before their children; walked backwards below
    for (size_t i = 0; i < order.size(); i++) {
        const BVHNode& b = nodes[order[i]];
        if (b.triCount == 0) { order.push_back(b.index); order.push_back(b.index + 1); }
    }
    for (size_t i = order.size(); i-- > 0;) {
        BVHNode& n = nodes[order[i]];
        Box3 b;
        if (n.triCount) {
            for (uint32_t t = n.index; t < n.index + n.triCount; t++)
                for (uint32_t v : {triangles[t].v0, triangles[t].v1, triangles[t].v2}) b.grow(points[v].position, points[v].position);
        } else {
            const BVHNode &l = nodes[n.index], &r = nodes[n.index + 1];
            const float llo[3] = {l.boundsX[0], l.boundsY[0], l.boundsZ[0]}, lhi[3] = {l.boundsX[1], l.boundsY[1], l.boundsZ[1]};
            const float rlo[3] = {r.boundsX[0], r.boundsY[0], r.boundsZ[0]}, rhi[3] = {r.boundsX[1], r.boundsY[1], r.boundsZ[1]};
            for (int k = 0; k < 3; k++) { b.lo[k] = llo[k]; b.hi[k] = lhi[k]; }
            b.grow(rlo, rhi);
        }
        n.boundsX[0] = b.lo[0]; n.boundsX[1] = b.hi[0];
        n.boundsY[0] = b.lo[1]; n.boundsY[1] = b.hi[1];
        n.boundsZ[0] = b.lo[2]; n.boundsZ[1] = b.hi[2];
    }
}

// rt_update_points on the host scene's own arrays: the same replacement, the same rule. The list of meshes is made on the first
// call and kept in the scene until geometry is added (a walk over every node and triangle otherwise paid per call).
extern "C" int rt_scene_update_points(rt_scene* s, const TrianglePoint* points, uint32_t first, uint32_t count) {
    if (!s) return -1;
    RtSceneHost& h = *rt_scene_host(s);
    const std::string refused = check_update_points("rt_scene_update_points", (uint32_t)h.triPoints.size(), points, first, count);
    if (!refused.empty()) return rt_scene_fail(s, refused.c_str());
    if (count == 0) return 0;
    const size_t key[4] = {h.bvhNodes.size(), h.triangles.size(), h.objects.size(), h.triPoints.size()};
    std::vector<RefitMesh> meshes;
    if (!h.refitMeshes.empty() && std::equal(key, key + 4, h.refitMeshesFor)) {
        for (size_t i = 0; i + 5 <= h.refitMeshes.size(); i += 5) {
            RefitMesh m;
            m.root = h.refitMeshes[i]; m.pointFirst = h.refitMeshes[i + 1]; m.pointEnd = h.refitMeshes[i + 2]; m.triFirst = h.refitMeshes[i + 3]; m.triCount = h.refitMeshes[i + 4];
            meshes.push_back(m);
        }
    } else {
        RtSceneArrays a;
        rt_scene_get_arrays(s, &a);
        std::string error;
        meshes = refit_meshes(a, error);
        if (!error.empty()) return rt_scene_fail(s, ("rt_scene_update_points: " + error).c_str());
        h.refitMeshes.clear();
        for (const RefitMesh& m : meshes) h.refitMeshes.insert(h.refitMeshes.end(), {m.root, m.pointFirst, m.pointEnd, m.triFirst, m.triCount});
        std::copy(key, key + 4, h.refitMeshesFor);
    }
    std::copy(points, points + count, h.triPoints.begin() + first);
    for (uint32_t m : touched_meshes(meshes, first, count)) refit_nodes_host(h.bvhNodes.data(), h.triangles.data(), h.triPoints.data(), meshes[m].root);
    return 0;
}
