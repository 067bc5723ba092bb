// mesh_topology.cpp — see mesh_topology.h. Host only: compiled into the library by hipcc and into tests/mesh_topology_check.cpp by g++.
#include "mesh_topology.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <utility>

#include "point_queries.h"
#include "rt_point_side.h"

namespace {

struct V3d { double x, y, z; };
V3d sub(V3d a, V3d b) { return V3d{a.x - b.x, a.y - b.y, a.z - b.z}; }
V3d cross(V3d a, V3d b) { return V3d{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(V3d a, V3d b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// the triangles of the mesh under `root`: its leaf ranges, in index order. false: the tree indexes out of range
bool mesh_triangles(const RtSceneArrays& s, uint32_t root, std::vector<uint32_t>* tris) {
    if (root >= s.bvhNodeCount) return false;
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    std::vector<uint32_t> st(1, root);
    size_t visited = 0;
    while (!st.empty()) {
        const uint32_t nidx = st.back();
        st.pop_back();
        if (nidx >= s.bvhNodeCount || ++visited > (size_t)s.bvhNodeCount + 1) return false;
        const BVHNode& b = s.bvhNodes[nidx];
        if (b.triCount) {
            if ((uint64_t)b.index + b.triCount > s.triangleCount) return false;
            ranges.emplace_back(b.index, b.triCount);
        } else {
            st.push_back(b.index);
            st.push_back(b.index + 1);
        }
    }
    std::sort(ranges.begin(), ranges.end());
    for (const auto& r : ranges)
        for (uint32_t t = r.first; t < r.first + r.second; t++) tris->push_back(t);
    return true;
}

uint32_t find_root(std::vector<uint32_t>& parent, uint32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}

struct EdgeUse { uint32_t lo, hi, ref; };   // welded ends, triangle (local) << 2 | edge

// One mesh: the rows of its triangles (written into rows[] at their scene indices) and its statistics (orientation left 0)
RtMeshTopology mesh_topology(const RtSceneArrays& s, const std::vector<uint32_t>& tris, std::vector<uint4>& rows) {
    RtMeshTopology st;
    memset(&st, 0, sizeof st);
    const uint32_t T = (uint32_t)tris.size();
    st.triangles = T;
    // 1. weld: the mesh's points sorted by position bits (-0 as +0); NaN positions stay single
    std::vector<uint32_t> used;
    used.reserve((size_t)T * 3);
    for (uint32_t t : tris) { const Triangle& tr = s.triangles[t]; used.push_back(tr.v0); used.push_back(tr.v1); used.push_back(tr.v2); }
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    struct Key { uint32_t b[3]; bool nan; };
    auto key_of = [&](uint32_t p) {
        Key k;
        k.nan = false;
        for (int d = 0; d < 3; d++) {
            const float f = s.triPoints[p].position[d];
            k.nan = k.nan || f != f;
            k.b[d] = f == 0.f ? 0u : rt_f2u(f);
        }
        return k;
    };
    std::vector<uint32_t> order(used.size());
    std::iota(order.begin(), order.end(), 0u);
    std::vector<Key> keys(used.size());
    for (size_t i = 0; i < used.size(); i++) keys[i] = key_of(used[i]);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const Key &ka = keys[a], &kb = keys[b];
        if (ka.b[0] != kb.b[0]) return ka.b[0] < kb.b[0];
        if (ka.b[1] != kb.b[1]) return ka.b[1] < kb.b[1];
        if (ka.b[2] != kb.b[2]) return ka.b[2] < kb.b[2];
        return a < b;
    });
    std::vector<uint32_t> weldOfUsed(used.size(), 0);
    uint32_t welded = 0;
    for (size_t i = 0; i < order.size(); i++) {
        const Key& k = keys[order[i]];
        const bool same = i > 0 && !k.nan && !keys[order[i - 1]].nan && memcmp(k.b, keys[order[i - 1]].b, sizeof k.b) == 0;
        if (!same) welded++;
        weldOfUsed[order[i]] = welded - 1;
    }
    st.weldedVertices = welded;
    auto weld = [&](uint32_t p) { return weldOfUsed[(size_t)(std::lower_bound(used.begin(), used.end(), p) - used.begin())]; };
    auto pos = [&](uint32_t p) { const float* f = s.triPoints[p].position; return V3d{(double)f[0], (double)f[1], (double)f[2]}; };

    // 2. corners and degenerate triangles
    std::vector<uint32_t> w((size_t)T * 3);
    std::vector<uint8_t> degenerate(T, 0);
    for (uint32_t i = 0; i < T; i++) {
        const Triangle& tr = s.triangles[tris[i]];
        const uint32_t v[3] = {tr.v0, tr.v1, tr.v2};
        for (int k = 0; k < 3; k++) w[(size_t)i * 3 + k] = weld(v[k]);
        const V3d n = cross(sub(pos(tr.v1), pos(tr.v0)), sub(pos(tr.v2), pos(tr.v0)));
        const bool flat = !(dot(n, n) > 0.0);
        degenerate[i] = w[(size_t)i * 3] == w[(size_t)i * 3 + 1] || w[(size_t)i * 3 + 1] == w[(size_t)i * 3 + 2] || w[(size_t)i * 3 + 2] == w[(size_t)i * 3] || flat;
        st.degenerateTriangles += degenerate[i];
    }

    // 3. edges
    std::vector<EdgeUse> edges;
    edges.reserve((size_t)T * 3);
    for (uint32_t i = 0; i < T; i++) {
        if (degenerate[i]) continue;
        for (uint32_t k = 0; k < 3; k++) {
            const uint32_t p = w[(size_t)i * 3 + k], q = w[(size_t)i * 3 + (k + 1) % 3];
            edges.push_back(EdgeUse{std::min(p, q), std::max(p, q), i << 2 | k});
        }
    }
    std::sort(edges.begin(), edges.end(), [](const EdgeUse& a, const EdgeUse& b) {
        if (a.lo != b.lo) return a.lo < b.lo;
        if (a.hi != b.hi) return a.hi < b.hi;
        return a.ref < b.ref;
    });
    std::vector<uint32_t> nb((size_t)T * 3, RT_TOPO_NONE);   // local triangle << 2 | edge
    std::vector<uint32_t> parent(T);
    std::iota(parent.begin(), parent.end(), 0u);
    std::vector<uint8_t> open(T, 0);   // the triangle has an edge that is not shared by exactly two
    for (size_t i = 0; i < edges.size();) {
        size_t j = i + 1;
        while (j < edges.size() && edges[j].lo == edges[i].lo && edges[j].hi == edges[i].hi) j++;
        const size_t uses = j - i;
        if (uses == 2) {
            nb[(size_t)(edges[i].ref >> 2) * 3 + (edges[i].ref & 3u)] = edges[i + 1].ref;
            nb[(size_t)(edges[i + 1].ref >> 2) * 3 + (edges[i + 1].ref & 3u)] = edges[i].ref;
        } else {
            if (uses == 1) st.boundaryEdges++;
            else st.nonManifoldEdges++;
            for (size_t k = i; k < j; k++) open[edges[k].ref >> 2] = 1;
        }
        for (size_t k = i + 1; k < j; k++) {
            const uint32_t a = find_root(parent, edges[i].ref >> 2), b = find_root(parent, edges[k].ref >> 2);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);   // a component's root is its lowest triangle
        }
        i = j;
    }

    // 4, 5. components: closed, orientable, with a volume
    std::vector<uint8_t> flip(T, 0), signable(T, 0), compOpen(T, 0);
    for (uint32_t i = 0; i < T; i++)
        if (!degenerate[i] && open[i]) compOpen[find_root(parent, i)] = 1;
    std::vector<std::vector<uint32_t>> members(T);
    for (uint32_t i = 0; i < T; i++)
        if (!degenerate[i]) members[find_root(parent, i)].push_back(i);
    std::vector<uint8_t> seen(T, 0);
    std::vector<uint32_t> queue;
    for (uint32_t root = 0; root < T; root++) {
        if (members[root].empty()) continue;
        st.components++;
        if (compOpen[root]) continue;
        bool orientable = true;
        queue.assign(1, root);
        seen[root] = 1;
        for (size_t head = 0; head < queue.size() && orientable; head++) {
            const uint32_t t = queue[head];
            for (uint32_t k = 0; k < 3; k++) {
                const uint32_t r = nb[(size_t)t * 3 + k], t2 = r >> 2, k2 = r & 3u;
                // stored windings that run along the shared edge the same way disagree
                const bool sameWay = w[(size_t)t * 3 + k] == w[(size_t)t2 * 3 + k2];
                const uint8_t want = flip[t] ^ (sameWay ? 1 : 0);
                if (!seen[t2]) { seen[t2] = 1; flip[t2] = want; queue.push_back(t2); }
                else if (flip[t2] != want) { orientable = false; break; }
            }
        }
        if (!orientable) continue;
        double volume = 0;
        for (uint32_t t : members[root]) {
            const Triangle& tr = s.triangles[tris[t]];
            const double v = dot(pos(tr.v0), cross(pos(tr.v1), pos(tr.v2)));
            volume += flip[t] ? -v : v;
        }
        if (!(volume != 0.0) || !std::isfinite(volume)) continue;
        st.signableComponents++;
        for (uint32_t t : members[root]) {
            if (volume < 0) flip[t] ^= 1;
            signable[t] = 1;
            st.signableTriangles++;
            st.flippedTriangles += flip[t];
        }
    }

    // 6. fans, by welded vertex
    std::vector<uint32_t> touching(welded, 0);
    for (uint32_t i = 0; i < T; i++)
        if (!degenerate[i])
            for (int k = 0; k < 3; k++) touching[w[(size_t)i * 3 + k]]++;
    for (uint32_t i = 0; i < T; i++) {
        uint4 row;
        row.x = row.y = row.z = RT_TOPO_NONE;
        row.w = 0;
        if (!degenerate[i]) {
            uint32_t n[3] = {RT_TOPO_NONE, RT_TOPO_NONE, RT_TOPO_NONE};
            for (uint32_t k = 0; k < 3; k++) {
                const uint32_t r = nb[(size_t)i * 3 + k];
                if (r != RT_TOPO_NONE) n[k] = tris[r >> 2] << 2 | (r & 3u);
            }
            row.x = n[0]; row.y = n[1]; row.z = n[2];
            row.w = (flip[i] && signable[i] ? RT_TOPO_FLIP : 0u) | (signable[i] ? RT_TOPO_SIGNABLE : 0u);
            for (uint32_t k = 0; k < 3; k++) {
                const uint32_t vertex = w[(size_t)i * 3 + k];
                uint32_t t = i, e = k, count = 0;   // cross edge e of t next
                bool closed = false;
                while (count < (uint32_t)RT_SIDE_MAX_FAN) {
                    count++;
                    const uint32_t r = nb[(size_t)t * 3 + e];
                    if (r == RT_TOPO_NONE) break;
                    const uint32_t t2 = r >> 2, e2 = r & 3u;
                    if (t2 == i) { closed = true; break; }
                    // the shared vertex is one end of the neighbour's edge e2; the other edge at that corner comes next
                    e = w[(size_t)t2 * 3 + e2] == vertex ? (e2 + 2) % 3 : (e2 + 1) % 3;
                    t = t2;
                }
                if (closed && count == touching[vertex]) row.w |= RT_TOPO_FAN << k;
            }
        }
        rows[tris[i]] = row;
    }
    return st;
}

struct HostAcc {
    const RtSceneArrays* s;
    const uint4* rows;
    const float* m;
    bool ident;
    rt_topo_row row(uint32_t tri) const {
        rt_topo_row r;
        r.n[0] = rows[tri].x; r.n[1] = rows[tri].y; r.n[2] = rows[tri].z; r.flags = rows[tri].w;
        return r;
    }
    void corners(uint32_t tri, rt_vec3* a, rt_vec3* b, rt_vec3* c) const {
        const Triangle& tr = s->triangles[tri];
        const float *pa = s->triPoints[tr.v0].position, *pb = s->triPoints[tr.v1].position, *pc = s->triPoints[tr.v2].position;
        *a = rt_v3(pa[0], pa[1], pa[2]); *b = rt_v3(pb[0], pb[1], pb[2]); *c = rt_v3(pc[0], pc[1], pc[2]);
        if (!ident) { *a = rt_xform_point(m, *a); *b = rt_xform_point(m, *b); *c = rt_xform_point(m, *c); }
    }
};

}  // namespace

int32_t object_orientation(const float* m) {
    const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (!std::isfinite(det) || det == 0.0) return 0;
    return det > 0 ? 1 : -1;
}

std::vector<int32_t> layout_orientation(const RenderObject* o, uint32_t n) {
    std::vector<int32_t> t(std::max(n, 1u), 0);
    for (uint32_t i = 0; i < n; i++) t[i] = object_orientation(o[i].transformMatrix);
    return t;
}

TopologyTables build_topology(const char* fn, const RtSceneArrays& s) {
    TopologyTables out;
    const std::string f(fn);
    if (s.triangleCount >= (uint32_t)RT_TOPOLOGY_MAX_TRIANGLES) {
        out.error = f + ": " + std::to_string(s.triangleCount) + " triangles do not fit the 30 bits of a neighbour word";
        return out;
    }
    for (uint32_t t = 0; t < s.triangleCount; t++)
        if (s.triangles[t].v0 >= s.triPointCount || s.triangles[t].v1 >= s.triPointCount || s.triangles[t].v2 >= s.triPointCount) {
            out.error = f + ": triangle " + std::to_string(t) + " indexes a point out of range";
            return out;
        }
    uint4 none;
    none.x = none.y = none.z = RT_TOPO_NONE;
    none.w = 0;
    out.rows.assign(std::max(s.triangleCount, 1u), none);
    out.stats.resize(s.objectCount);
    for (uint32_t i = 0; i < s.objectCount; i++) {
        const uint32_t root = s.objects[i].bvhIndex;
        bool shared = false;
        for (uint32_t k = 0; k < i && !shared; k++)
            if (s.objects[k].bvhIndex == root) { out.stats[i] = out.stats[k]; shared = true; }
        if (shared) continue;
        std::vector<uint32_t> tris;
        if (!mesh_triangles(s, root, &tris)) {
            out.error = f + ": the BVH of object " + std::to_string(i) + " indexes out of range";
            return out;
        }
        out.stats[i] = mesh_topology(s, tris, out.rows);
    }
    out.orientation = layout_orientation(s.objects, s.objectCount);
    for (uint32_t i = 0; i < s.objectCount; i++) out.stats[i].orientation = out.orientation[i];
    return out;
}

std::string check_signed_query(const char* fn, bool sceneUploaded, bool topologyUploaded, const TopologyCounts& topology, const TopologyCounts& scene,
                               const RtPointBatch* points, const void* out, const void* side) {
    const std::string f(fn);
    if (!sceneUploaded) return f + " before rt_upload_scene";
    if (!topologyUploaded) return f + ": no topology uploaded";
    if (!(topology == scene)) return f + ": topology does not match the uploaded scene";
    if (!points) return f + ": the batch is NULL";
    if (points->n == 0) return "";
    if (!points->points || !out || !side) return f + ": points, the output and side are required";
    if (points->n >= (uint32_t)RT_NEAREST_MAX_POINTS) return f + ": a batch of " + std::to_string(points->n) + " points does not fit the 30 bits of a slot id";
    return "";
}

extern "C" {

int rt_scene_topology(const RtSceneArrays* s, RtMeshTopology* out, uint32_t nObjects) {
    if (!s || (!out && nObjects)) return -1;
    const TopologyTables t = build_topology("rt_scene_topology", *s);
    if (!t.error.empty()) return -1;
    for (uint32_t i = 0; i < nObjects && i < s->objectCount; i++) out[i] = t.stats[i];
    return 0;
}

// the rule over a batch; feature / fan: per point the region code (255: the rule ended before it, or no triangle) and the fan walked
static int side_loop(const char* fn, const RtSceneArrays* s, const RtPointBatch* points, const RtNearest* recs, int8_t* side, uint8_t* feature, uint16_t* fan) {
    if (!s || !points) return -1;
    const uint32_t n = points->n;
    if (n == 0) return 0;
    if (!points->points || !recs || !side || n >= (uint32_t)RT_NEAREST_MAX_POINTS) return -1;
    const TopologyTables t = build_topology(fn, *s);
    if (!t.error.empty()) return -1;
    for (uint32_t i = 0; i < n; i++) {
        const RtNearest& r = recs[i];
        if (!r.found) continue;
        if (r.isSphere ? r.objectIndex >= s->sphereCount : (r.objectIndex >= s->objectCount || r.triIndex >= s->triangleCount)) return -1;
    }
    auto is_identity = [](const float* m) {   // rows 0..2 of the matrix are the identity's (RT_OBJ_FWD_IDENTITY on the device)
        bool is = true;
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 3; r++) is = is && m[c * 4 + r] == (r == c ? 1.f : 0.f);
        return is;
    };
    for (uint32_t i = 0; i < n; i++) {
        const RtNearest& r = recs[i];
        const rt_vec3 q = rt_v3(points->points[(size_t)i * 3], points->points[(size_t)i * 3 + 1], points->points[(size_t)i * 3 + 2]);
        int sd = 0, feat = -1;
        uint32_t steps = 0;
        if (r.found && r.isSphere) {
            const Sphere& sp = s->spheres[r.objectIndex];
            sd = rt_point_side_sphere(q, rt_v3(sp.position[0], sp.position[1], sp.position[2]), sp.radius);
        } else if (r.found) {
            const float* m = s->objects[r.objectIndex].transformMatrix;
            const HostAcc acc{s, t.rows.data(), m, is_identity(m)};
            sd = rt_point_side_triangle(acc, q, r.triIndex, r.uv[0], r.uv[1], (int)t.orientation[r.objectIndex], &feat, &steps);
        }
        side[i] = (int8_t)sd;
        if (feature) feature[i] = feat < 0 ? 255 : (uint8_t)feat;
        if (fan) fan[i] = (uint16_t)steps;
    }
    return 0;
}

int rt_nearest_side_host(const RtSceneArrays* s, const RtPointBatch* points, const RtNearest* recs, int8_t* side) {
    return side_loop("rt_nearest_side_host", s, points, recs, side, nullptr, nullptr);
}

int rt_nearest_side_features_host(const RtSceneArrays* s, const RtPointBatch* points, const RtNearest* recs, int8_t* side, uint8_t* feature, uint16_t* fan) {
    return side_loop("rt_nearest_side_features_host", s, points, recs, side, feature, fan);
}

}  // extern "C"
