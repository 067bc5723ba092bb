// mesh_topology_check.cpp — the host-only unit of the signed point queries (ray_tracer_amd/csrc/mesh_topology.h) and the units of their
// rule (include/rt_point_side.h) on the CPU, built with plain g++ by tests/test_mesh_topology_host.py. Hand-made meshes with their
// exact expected rows and statistics: a tetrahedron (adjacency and edge numbers spelled out), one face reversed, stored inside out,
// two tetrahedra sharing one vertex, an open box, a Moebius strip, a closed non-orientable grid (a Klein bottle's), a mesh with
// degenerate triangles and -0 / +0 / NaN points, a flat double-sided quad, fans of 256 and 300 triangles; every refusal message;
// the orientation of identity, mirrored, singular and NaN matrices; rt_point_triangle_feature against the (u, v) rt_point_triangle
// returns; rt_angle against double atan2; rt_nearest_side_host on the tetrahedron. Prints "mesh topology ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mesh_topology.h"
#include "rt_point_side.h"
#include "check.h"

namespace {

const uint32_t NONE = RT_TOPO_NONE;
const uint32_t ALL_FANS = RT_TOPO_FAN | RT_TOPO_FAN << 1 | RT_TOPO_FAN << 2;

struct P3 { float x, y, z; };

// One mesh under one leaf root, every triangle with three points of its own (as an OBJ reader leaves them): welding has to find them
struct Mesh {
    std::vector<TrianglePoint> points;
    std::vector<Triangle> tris;
    std::vector<RenderObject> objects;
    BVHNode node;
    void add(P3 a, P3 b, P3 c) {
        Triangle t;
        memset(&t, 0, sizeof t);
        t.v0 = (uint32_t)points.size(); t.v1 = t.v0 + 1; t.v2 = t.v0 + 2;
        for (const P3& p : {a, b, c}) {
            TrianglePoint tp;
            memset(&tp, 0, sizeof tp);
            tp.position[0] = p.x; tp.position[1] = p.y; tp.position[2] = p.z;
            points.push_back(tp);
        }
        tris.push_back(t);
    }
    void add(const std::vector<P3>& v, int i, int j, int k) { add(v[i], v[j], v[k]); }
    RtSceneArrays arrays() {
        if (objects.empty()) place(nullptr);
        memset(&node, 0, sizeof node);
        node.index = 0; node.triCount = (uint32_t)tris.size();
        RtSceneArrays a;
        memset(&a, 0, sizeof a);
        a.triPoints = points.data(); a.triPointCount = (uint32_t)points.size();
        a.triangles = tris.data(); a.triangleCount = (uint32_t)tris.size();
        a.objects = objects.data(); a.objectCount = (uint32_t)objects.size();
        a.bvhNodes = &node; a.bvhNodeCount = 1;
        return a;
    }
    void place(const float* m) {
        RenderObject o;
        memset(&o, 0, sizeof o);
        for (int k = 0; k < 4; k++) o.transformMatrix[k * 5] = 1.f;
        if (m) memcpy(o.transformMatrix, m, sizeof o.transformMatrix);
        objects.push_back(o);
    }
};

void expect_row(const TopologyTables& t, uint32_t tri, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t flags) {
    const uint4 r = t.rows[tri];
    CHECK(r.x == n0 && r.y == n1 && r.z == n2 && r.w == flags, "triangle %u: {%u, %u, %u, %u}, expected {%u, %u, %u, %u}", tri, r.x, r.y, r.z, r.w, n0, n1, n2, flags);
}
void expect_stats(const RtMeshTopology& s, uint32_t tris, uint32_t welded, uint32_t comps, uint32_t sigComps, uint32_t sigTris, uint32_t boundary, uint32_t nonManifold,
                  uint32_t flipped, uint32_t degenerate) {
    CHECK(s.triangles == tris && s.weldedVertices == welded && s.components == comps && s.signableComponents == sigComps && s.signableTriangles == sigTris &&
              s.boundaryEdges == boundary && s.nonManifoldEdges == nonManifold && s.flippedTriangles == flipped && s.degenerateTriangles == degenerate,
          "statistics {%u %u %u %u %u %u %u %u %u}", s.triangles, s.weldedVertices, s.components, s.signableComponents, s.signableTriangles, s.boundaryEdges,
          s.nonManifoldEdges, s.flippedTriangles, s.degenerateTriangles);
}

const std::vector<P3> TETRA = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
// outward: T0 = (0, 2, 1) on z = 0, T1 = (0, 1, 3) on y = 0, T2 = (0, 3, 2) on x = 0, T3 = (1, 2, 3)
Mesh tetrahedron(int reversedFrom = 4, int reversedTo = 4) {
    const int f[4][3] = {{0, 2, 1}, {0, 1, 3}, {0, 3, 2}, {1, 2, 3}};
    Mesh m;
    for (int k = 0; k < 4; k++) {
        if (k >= reversedFrom && k < reversedTo) m.add(TETRA, f[k][0], f[k][2], f[k][1]);
        else m.add(TETRA, f[k][0], f[k][1], f[k][2]);
    }
    return m;
}

void tetrahedra() {
    const uint32_t OK = RT_TOPO_SIGNABLE | ALL_FANS;
    {
        g_where = "tetrahedron";
        Mesh m = tetrahedron();
        const TopologyTables t = build_topology("f", m.arrays());
        CHECK(t.error.empty() && t.rows.size() == 4 && t.stats.size() == 1);
        // T0's edges (0,2) (2,1) (1,0) meet T2's edge 2, T3's edge 0, T1's edge 0; and so on: triangle << 2 | edge
        expect_row(t, 0, 2u << 2 | 2, 3u << 2 | 0, 1u << 2 | 0, OK);
        expect_row(t, 1, 0u << 2 | 2, 3u << 2 | 2, 2u << 2 | 0, OK);
        expect_row(t, 2, 1u << 2 | 2, 3u << 2 | 1, 0u << 2 | 0, OK);
        expect_row(t, 3, 0u << 2 | 1, 2u << 2 | 1, 1u << 2 | 1, OK);
        expect_stats(t.stats[0], 4, 4, 1, 1, 4, 0, 0, 0, 0);
        CHECK(t.stats[0].orientation == 1 && t.orientation[0] == 1);
    }
    {
        g_where = "one face reversed";
        Mesh m = tetrahedron(3, 4);   // T3 stored as (1, 3, 2): its edges are (1,3) (3,2) (2,1)
        const TopologyTables t = build_topology("f", m.arrays());
        expect_row(t, 0, 2u << 2 | 2, 3u << 2 | 2, 1u << 2 | 0, OK);
        expect_row(t, 1, 0u << 2 | 2, 3u << 2 | 0, 2u << 2 | 0, OK);
        expect_row(t, 2, 1u << 2 | 2, 3u << 2 | 1, 0u << 2 | 0, OK);
        expect_row(t, 3, 1u << 2 | 1, 2u << 2 | 1, 0u << 2 | 1, OK | RT_TOPO_FLIP);
        expect_stats(t.stats[0], 4, 4, 1, 1, 4, 0, 0, 1, 0);
    }
    {
        g_where = "the first face reversed";   // the walk starts at the reversed one: the volume decides
        Mesh m = tetrahedron(0, 1);
        const TopologyTables t = build_topology("f", m.arrays());
        CHECK(t.rows[0].w == (OK | RT_TOPO_FLIP) && t.rows[1].w == OK && t.rows[2].w == OK && t.rows[3].w == OK);
        expect_stats(t.stats[0], 4, 4, 1, 1, 4, 0, 0, 1, 0);
    }
    {
        g_where = "inside out";
        Mesh m = tetrahedron(0, 4);
        const TopologyTables t = build_topology("f", m.arrays());
        for (uint32_t k = 0; k < 4; k++) CHECK(t.rows[k].w == (OK | RT_TOPO_FLIP));
        expect_stats(t.stats[0], 4, 4, 1, 1, 4, 0, 0, 4, 0);
    }
    {
        g_where = "two tetrahedra sharing a vertex";
        Mesh m = tetrahedron();
        std::vector<P3> mirrored;
        for (const P3& p : TETRA) mirrored.push_back(P3{-p.x, -p.y, -p.z});
        const int f[4][3] = {{0, 1, 2}, {0, 3, 1}, {0, 2, 3}, {1, 3, 2}};   // the point reflection turns every face over
        for (int k = 0; k < 4; k++) m.add(mirrored, f[k][0], f[k][1], f[k][2]);
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 8, 7, 2, 2, 8, 0, 0, 0, 0);
        // corner 0 of the three faces at the origin, in both: six triangles touch the vertex, a fan sees three
        for (uint32_t k = 0; k < 8; k++) CHECK(t.rows[k].w == (RT_TOPO_SIGNABLE | ((k & 3u) == 3u ? ALL_FANS : (ALL_FANS & ~RT_TOPO_FAN))), "triangle %u: flags %u", k, t.rows[k].w);
        CHECK((t.rows[4].x >> 2) >= 4 && (t.rows[0].x >> 2) < 4);   // no neighbour across the two
    }
}

void add_quad(Mesh& m, const std::vector<P3>& v, int a, int b, int c, int d) { m.add(v, a, b, c); m.add(v, a, c, d); }

void open_and_odd() {
    {
        g_where = "open box";
        const std::vector<P3> v = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
        Mesh m;
        add_quad(m, v, 0, 3, 2, 1);   // bottom
        add_quad(m, v, 0, 1, 5, 4); add_quad(m, v, 1, 2, 6, 5); add_quad(m, v, 2, 3, 7, 6); add_quad(m, v, 3, 0, 4, 7);   // no lid
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 10, 8, 1, 0, 0, 4, 0, 0, 0);
        for (uint32_t k = 0; k < 10; k++) CHECK(!(t.rows[k].w & (RT_TOPO_SIGNABLE | RT_TOPO_FLIP)));
        uint32_t none = 0;
        for (uint32_t k = 0; k < 10; k++) none += (t.rows[k].x == NONE) + (t.rows[k].y == NONE) + (t.rows[k].z == NONE);
        CHECK(none == 4);
        // with the lid it is a solid
        add_quad(m, v, 4, 5, 6, 7);
        const TopologyTables c = build_topology("f", m.arrays());
        expect_stats(c.stats[0], 12, 8, 1, 1, 12, 0, 0, 0, 0);
    }
    {
        g_where = "Moebius strip";
        const int n = 7;
        std::vector<P3> a(n + 1), b(n + 1);
        for (int i = 0; i <= n; i++) {
            const double u = 2 * M_PI * i / n, h = 0.3;
            a[i] = P3{(float)((1 + h * std::cos(u / 2)) * std::cos(u)), (float)((1 + h * std::cos(u / 2)) * std::sin(u)), (float)(h * std::sin(u / 2))};
            b[i] = P3{(float)((1 - h * std::cos(u / 2)) * std::cos(u)), (float)((1 - h * std::cos(u / 2)) * std::sin(u)), (float)(-h * std::sin(u / 2))};
        }
        a[n] = b[0]; b[n] = a[0];   // the half twist
        Mesh m;
        for (int i = 0; i < n; i++) { m.add(a[i], b[i], b[i + 1]); m.add(a[i], b[i + 1], a[i + 1]); }
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 2 * n, 2 * n, 1, 0, 0, 2 * n, 0, 0, 0);
    }
    {
        g_where = "closed, not orientable";   // an N x M grid closed as a Klein bottle: column N is column 0 upside down
        const int N = 5, M = 5;
        std::vector<P3> v(N * M);
        uint32_t lcg = 12345u;
        for (P3& p : v) {
            float c[3];
            for (float& x : c) { lcg = lcg * 1664525u + 1013904223u; x = (float)(lcg >> 8) / 16777216.f; }
            p = P3{c[0], c[1], c[2]};
        }
        auto at = [&](int i, int j) { j = ((j % M) + M) % M; return i < N ? i * M + j : (M - j) % M; };
        Mesh m;
        for (int i = 0; i < N; i++)
            for (int j = 0; j < M; j++) add_quad(m, v, at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1));
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 2 * N * M, N * M, 1, 0, 0, 0, 0, 0, 0);
        for (uint32_t k = 0; k < (uint32_t)(2 * N * M); k++) CHECK(t.rows[k].x != NONE && t.rows[k].y != NONE && t.rows[k].z != NONE && !(t.rows[k].w & RT_TOPO_SIGNABLE));
        // the same grid closed as a torus is a solid's surface
        auto torus = [&](int i, int j) { return ((i % N) * M) + ((j % M) + M) % M; };
        Mesh o;
        for (int i = 0; i < N; i++)
            for (int j = 0; j < M; j++) add_quad(o, v, torus(i, j), torus(i + 1, j), torus(i + 1, j + 1), torus(i, j + 1));
        const TopologyTables to = build_topology("f", o.arrays());
        CHECK(to.stats[0].signableComponents == 1 && to.stats[0].signableTriangles == (uint32_t)(2 * N * M));
    }
    {
        g_where = "degenerate triangles, -0 and NaN";
        Mesh m = tetrahedron();
        for (TrianglePoint& p : m.points)   // every other zero is a negative one
            for (int d = 0; d < 3; d++)
                if (p.position[d] == 0.f && ((&p - m.points.data()) + d) % 2) p.position[d] = -0.f;
        m.add(TETRA[0], P3{-0.f, 0.f, -0.f}, TETRA[1]);                                       // two corners weld
        m.add(TETRA[0], TETRA[1], P3{2, 0, 0});                                               // collinear
        m.add(TETRA[0], TETRA[1], P3{std::numeric_limits<float>::quiet_NaN(), 0, 0});          // a NaN welds with nothing
        m.add(TETRA[0], TETRA[1], P3{std::numeric_limits<float>::quiet_NaN(), 0, 0});
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 8, 4 + 1 + 2, 1, 1, 4, 0, 0, 0, 4);
        for (uint32_t k = 0; k < 4; k++) CHECK(t.rows[k].w == (RT_TOPO_SIGNABLE | ALL_FANS) && (t.rows[k].x >> 2) < 4 && (t.rows[k].y >> 2) < 4 && (t.rows[k].z >> 2) < 4);
        for (uint32_t k = 4; k < 8; k++) expect_row(t, k, NONE, NONE, NONE, 0);
    }
    {
        g_where = "flat double-sided quad";
        const std::vector<P3> v = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
        Mesh m;
        m.add(v, 0, 1, 2); m.add(v, 0, 2, 3); m.add(v, 0, 3, 1); m.add(v, 1, 3, 2);
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 4, 4, 1, 0, 0, 0, 0, 0, 0);   // closed and orientable, but it holds no volume
        for (uint32_t k = 0; k < 4; k++) CHECK(t.rows[k].w == ALL_FANS);
    }
    for (int n : {256, 300}) {
        g_where = "a fan of " + std::to_string(n);
        std::vector<P3> ring(n);
        for (int i = 0; i < n; i++) ring[i] = P3{(float)std::cos(2 * M_PI * i / n), (float)std::sin(2 * M_PI * i / n), 0.f};
        const P3 top{0, 0, 1}, bottom{0, 0, -1};
        Mesh m;
        for (int i = 0; i < n; i++) { m.add(top, ring[i], ring[(i + 1) % n]); m.add(bottom, ring[(i + 1) % n], ring[i]); }
        const TopologyTables t = build_topology("f", m.arrays());
        expect_stats(t.stats[0], 2 * n, n + 2, 1, 1, 2 * n, 0, 0, 0, 0);
        const uint32_t apex = n <= RT_SIDE_MAX_FAN ? RT_TOPO_FAN : 0u;
        for (uint32_t k = 0; k < (uint32_t)(2 * n); k++) CHECK(t.rows[k].w == (RT_TOPO_SIGNABLE | apex | RT_TOPO_FAN << 1 | RT_TOPO_FAN << 2), "triangle %u: flags %u", k, t.rows[k].w);
        // the rule: above the apex is outside, just below it inside (256), or unknown (300: the fan is not walked)
        RtSceneArrays a = m.arrays();
        const float q[6] = {0.f, 0.f, 1.5f, 0.f, 0.f, 0.5f};
        const RtPointBatch pts{q, nullptr, 2};
        RtNearest rec[2];
        int8_t side[2] = {9, 9};
        CHECK(rt_nearest_exhaustive_host(&a, &pts, rec) == 0 && rt_nearest_side_host(&a, &pts, rec, side) == 0);
        CHECK(rec[0].uv[0] == 0.f && rec[0].uv[1] == 0.f);
        CHECK(side[0] == (n <= RT_SIDE_MAX_FAN ? 1 : 0) && side[1] == -1, "sides %d %d", side[0], side[1]);
    }
}

void refusals_and_orientation() {
    g_where = "refusals";
    float* const P = (float*)(uintptr_t)0x10000000u;
    void* const OUT = (void*)(uintptr_t)0x40000000u;
    void* const SIDE = (void*)(uintptr_t)0x50000000u;
    const TopologyCounts a{3, 100, 199}, otherObjects{4, 100, 199}, otherTris{3, 101, 199}, otherNodes{3, 100, 201};
    for (const char* fn : {"rt_query_nearest_signed", "rt_query_nearest_signed_host"}) {
        const std::string f(fn);
        const RtPointBatch ok{P, nullptr, 1000}, none{nullptr, nullptr, 0}, noP{nullptr, nullptr, 5}, big{P, nullptr, 1u << 30}, most{P, nullptr, (1u << 30) - 1u};
        CHECK(check_signed_query(fn, true, true, a, a, &ok, OUT, SIDE).empty());
        CHECK(check_signed_query(fn, true, true, a, a, &most, OUT, SIDE).empty());
        CHECK(check_signed_query(fn, true, true, a, a, &none, nullptr, nullptr).empty());
        CHECK(check_signed_query(fn, false, true, a, a, &ok, OUT, SIDE) == f + " before rt_upload_scene");
        CHECK(check_signed_query(fn, true, false, a, a, &ok, OUT, SIDE) == f + ": no topology uploaded");
        for (const TopologyCounts& other : {otherObjects, otherTris, otherNodes})
            CHECK(check_signed_query(fn, true, true, other, a, &ok, OUT, SIDE) == f + ": topology does not match the uploaded scene");
        CHECK(check_signed_query(fn, true, true, a, a, nullptr, OUT, SIDE) == f + ": the batch is NULL");
        CHECK(check_signed_query(fn, true, true, a, a, &noP, OUT, SIDE) == f + ": points, the output and side are required");
        CHECK(check_signed_query(fn, true, true, a, a, &ok, nullptr, SIDE) == f + ": points, the output and side are required");
        CHECK(check_signed_query(fn, true, true, a, a, &ok, OUT, nullptr) == f + ": points, the output and side are required");
        CHECK(check_signed_query(fn, true, true, a, a, &big, OUT, SIDE) == f + ": a batch of 1073741824 points does not fit the 30 bits of a slot id");
        // the order: the scene, the topology, its match, the batch, the pointers, the size; n == 0 does not excuse the first three
        CHECK(check_signed_query(fn, false, false, otherTris, a, nullptr, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_signed_query(fn, true, false, otherTris, a, nullptr, nullptr, nullptr) == f + ": no topology uploaded");
        CHECK(check_signed_query(fn, true, true, otherTris, a, nullptr, nullptr, nullptr) == f + ": topology does not match the uploaded scene");
        CHECK(check_signed_query(fn, true, false, a, a, &none, nullptr, nullptr) == f + ": no topology uploaded");
        CHECK(check_signed_query(fn, true, true, a, a, &big, nullptr, SIDE) == f + ": points, the output and side are required");
    }
    {
        Mesh m = tetrahedron();
        RtSceneArrays s = m.arrays();
        s.triangleCount = 1u << 30;   // (refused before any triangle is read)
        CHECK(build_topology("rt_upload_topology", s).error == "rt_upload_topology: 1073741824 triangles do not fit the 30 bits of a neighbour word");
        RtMeshTopology st;
        CHECK(rt_scene_topology(&s, &st, 1) == -1 && rt_scene_topology(nullptr, &st, 1) == -1);
        s = m.arrays();
        m.tris[2].v1 = 1000;
        CHECK(build_topology("f", s).error == "f: triangle 2 indexes a point out of range");
        m = tetrahedron();
        s = m.arrays();
        m.node.index = 2;
        CHECK(build_topology("f", s).error == "f: the BVH of object 0 indexes out of range");
        // rt_nearest_side_host: records that index out of range
        m = tetrahedron();
        s = m.arrays();
        const float q[3] = {5, 5, 5};
        const RtPointBatch pts{q, nullptr, 1};
        RtNearest r;
        int8_t side = 9;
        CHECK(rt_nearest_exhaustive_host(&s, &pts, &r) == 0 && rt_nearest_side_host(&s, &pts, &r, &side) == 0 && side == 1);
        RtNearest bad = r;
        bad.triIndex = 4;
        CHECK(rt_nearest_side_host(&s, &pts, &bad, &side) == -1);
        bad = r; bad.objectIndex = 1;
        CHECK(rt_nearest_side_host(&s, &pts, &bad, &side) == -1);
        bad = r; bad.isSphere = 1;
        CHECK(rt_nearest_side_host(&s, &pts, &bad, &side) == -1);
        CHECK(rt_nearest_side_host(&s, &pts, nullptr, &side) == -1 && rt_nearest_side_host(&s, &pts, &r, nullptr) == -1 && rt_nearest_side_host(nullptr, &pts, &r, &side) == -1);
        memset(&bad, 0, sizeof bad);
        bad.dst = RT_MISS_DST;
        side = 9;
        CHECK(rt_nearest_side_host(&s, &pts, &bad, &side) == 0 && side == 0);   // nothing found
    }
    g_where = "orientation";
    float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(object_orientation(m) == 1);
    m[0] = -1;
    CHECK(object_orientation(m) == -1);
    m[5] = -2;
    CHECK(object_orientation(m) == 1);
    m[10] = 0;
    CHECK(object_orientation(m) == 0);
    m[10] = std::numeric_limits<float>::quiet_NaN();
    CHECK(object_orientation(m) == 0);
    m[10] = std::numeric_limits<float>::infinity();
    CHECK(object_orientation(m) == 0);
    const float shear[16] = {1, 0, -0.4f, 0, 0.7f, 1, 0, 0, 0, 0, 1, 0, 3, 4, 5, 1};
    CHECK(object_orientation(shear) == 1);
    const float dependent[16] = {1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(object_orientation(dependent) == 0);
    {
        Mesh t = tetrahedron();
        float mirror[16] = {-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, flat[16] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        t.place(nullptr); t.place(mirror); t.place(flat);
        const RtSceneArrays s = t.arrays();
        const TopologyTables tt = build_topology("f", s);
        CHECK(tt.orientation.size() == 3 && tt.orientation[0] == 1 && tt.orientation[1] == -1 && tt.orientation[2] == 0);
        CHECK(tt.stats[1].signableTriangles == 4 && tt.stats[1].orientation == -1 && tt.stats[2].orientation == 0);   // one mesh, shared rows
        CHECK(layout_orientation(s.objects, 0).size() == 1);
        // inside stays inside under the mirror; the flat placement is unknown
        const float q[6] = {0.3f, 0.1f, 0.2f, -0.3f, 0.1f, 0.2f};
        const RtPointBatch pts{q, nullptr, 2};
        RtNearest rec[2];
        int8_t side[2];
        CHECK(rt_nearest_exhaustive_host(&s, &pts, rec) == 0 && rt_nearest_side_host(&s, &pts, rec, side) == 0);
        CHECK(rec[0].objectIndex != 1 && rec[1].objectIndex == 1);
        CHECK(side[0] == (rec[0].objectIndex == 2 ? 0 : -1) && side[1] == -1, "sides %d %d", side[0], side[1]);
    }
}

float rnd(uint32_t* s) { return rt_random(s) * 2.f - 1.f; }

void features() {
    g_where = "rt_point_triangle_feature";
    uint32_t state = 2024u;
    int seen[7] = {};
    for (int it = 0; it < 200000; it++) {
        rt_vec3 a = rt_v3(rnd(&state), rnd(&state), rnd(&state)), b = rt_v3(rnd(&state), rnd(&state), rnd(&state)), c = rt_v3(rnd(&state), rnd(&state), rnd(&state));
        const int kind = it % 8;
        if (kind == 5) c = rt_add(a, rt_scale(rt_sub(b, a), rnd(&state)));          // collinear up to rounding
        if (kind == 6) c = b;                                                        // an edge twice
        if (kind == 7) { b = a; if (it % 16 == 7) c = a; }                           // a point
        if (kind == 4) c = rt_add(rt_add(a, rt_scale(rt_sub(b, a), 0.5f)), rt_scale(rt_v3(rnd(&state), rnd(&state), rnd(&state)), 1e-6f));   // a sliver
        rt_vec3 q = rt_v3(2.f * rnd(&state), 2.f * rnd(&state), 2.f * rnd(&state));
        if (it % 5 == 0) q = rt_bary_point(a, b, c, 0.3f, 0.3f);                     // on the plane
        if (it % 50 == 0) q = a;
        float u, v, u2, v2;
        const float d2 = rt_point_triangle(q, a, b, c, &u, &v);
        const int f = rt_point_triangle_feature(q, a, b, c);
        CHECK(f >= 0 && f <= 6);
        seen[f < 0 || f > 6 ? 0 : f]++;
        switch (f) {
            case RT_FEAT_A: CHECK(u == 0.f && v == 0.f); break;
            case RT_FEAT_B: CHECK(u == 1.f && v == 0.f); break;
            case RT_FEAT_C: CHECK(u == 0.f && v == 1.f); break;
            case RT_FEAT_AB: CHECK(v == 0.f); break;
            case RT_FEAT_AC: CHECK(u == 0.f); break;
            case RT_FEAT_BC: CHECK(u == 1.f - v); break;
            default: CHECK(u >= 0.f && v >= 0.f); break;
        }
        // rt_point_triangle keeps its bits with the feature beside it
        CHECK(rt_f2u(rt_point_triangle(q, a, b, c, &u2, &v2)) == rt_f2u(d2) && rt_f2u(u2) == rt_f2u(u) && rt_f2u(v2) == rt_f2u(v));
    }
    for (int k = 0; k < 7; k++) CHECK(seen[k] > 1000, "feature %d seen %d times", k, seen[k]);
}

void angles() {
    g_where = "rt_angle";
    uint32_t state = 99u;
    double worst = 0;
    auto one = [&](rt_vec3 e1, rt_vec3 e2) {
        const double x[3] = {(double)e1.y * e2.z - (double)e1.z * e2.y, (double)e1.z * e2.x - (double)e1.x * e2.z, (double)e1.x * e2.y - (double)e1.y * e2.x};
        const double ref = std::atan2(std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), (double)e1.x * e2.x + (double)e1.y * e2.y + (double)e1.z * e2.z);
        const double err = std::fabs((double)rt_angle(e1, e2) - ref);
        if (err > worst) worst = err;
        CHECK(err <= 1e-6, "rt_angle off by %.3g at angle %.9g", err, ref);
    };
    for (int it = 0; it < 400000; it++) {
        const rt_vec3 e1 = rt_v3(rnd(&state), rnd(&state), rnd(&state));
        rt_vec3 e2 = rt_v3(rnd(&state), rnd(&state), rnd(&state));
        const float s = rt_exp2(8.f * rnd(&state));
        if (it % 4 == 1) e2 = rt_add(rt_scale(e1, rnd(&state)), rt_scale(e2, 1e-3f * rnd(&state)));   // nearly parallel or opposite
        if (it % 4 == 2) e2 = rt_cross(e1, e2);                                                          // a right angle
        one(rt_scale(e1, s), e2);
    }
    // every angle of a plane sweep, and the ends
    for (int k = 0; k <= 36000; k++) {
        const double t = M_PI * k / 36000.0;
        one(rt_v3(1.f, 0.f, 0.f), rt_v3((float)std::cos(t), (float)std::sin(t), 0.f));
    }
    CHECK(rt_angle(rt_v3(1, 0, 0), rt_v3(2, 0, 0)) == 0.f && rt_angle(rt_v3(0, 0, 0), rt_v3(1, 0, 0)) == 0.f);
    CHECK(std::fabs(rt_angle(rt_v3(1, 0, 0), rt_v3(-3, 0, 0)) - (float)M_PI) <= 1e-6f);
    printf("rt_angle worst %.3g\n", worst);
}

// the tetrahedron, stored with one face reversed and under a mirror: faces, edges and vertices from both sides
void sides() {
    g_where = "sides";
    for (int variant = 0; variant < 3; variant++) {
        Mesh m = variant == 1 ? tetrahedron(1, 3) : tetrahedron();
        const float mirror[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (variant == 2) m.place(mirror);
        const RtSceneArrays s = m.arrays();
        const float sy = variant == 2 ? -1.f : 1.f;
        struct Q { float x, y, z; int side; } const qs[] = {
            {0.2f, 0.2f, -0.5f, 1}, {0.2f, 0.2f, 0.1f, -1}, {1.f, 1.f, 1.f, 1},                 // faces
            {-0.3f, -0.3f, -0.3f, 1}, {2.f, -0.1f, -0.1f, 1}, {-0.1f, -0.1f, 2.f, 1},          // vertices
            {0.5f, -0.4f, -0.4f, 1}, {-0.4f, 0.5f, -0.4f, 1}, {0.7f, 0.7f, -0.3f, 1},          // edges
            {0.02f, 0.02f, 0.02f, -1}, {0.9f, 0.03f, 0.03f, -1},
            {-1.f, 0.3f, 0.3f, 1}, {0.25f, 0.25f, 0.25f, -1}};
        const uint32_t n = sizeof qs / sizeof qs[0];
        std::vector<float> q;
        for (const Q& p : qs) { q.push_back(p.x); q.push_back(p.y * sy); q.push_back(p.z); }
        const RtPointBatch pts{q.data(), nullptr, n};
        std::vector<RtNearest> rec(n);
        std::vector<int8_t> side(n, 9);
        CHECK(rt_nearest_exhaustive_host(&s, &pts, rec.data()) == 0 && rt_nearest_side_host(&s, &pts, rec.data(), side.data()) == 0);
        for (uint32_t i = 0; i < n; i++) CHECK(side[i] == qs[i].side, "variant %d point %u: side %d", variant, i, side[i]);
    }
    // spheres
    CHECK(rt_point_side_sphere(rt_v3(2, 0, 0), rt_v3(0, 0, 0), 1.f) == 1 && rt_point_side_sphere(rt_v3(0.5f, 0, 0), rt_v3(0, 0, 0), 1.f) == -1);
    CHECK(rt_point_side_sphere(rt_v3(0, 1, 0), rt_v3(0, 0, 0), 1.f) == 0 && rt_point_side_sphere(rt_v3(0, 0, 0), rt_v3(0, 0, 0), 1.f) == -1);
}

}  // namespace

int main() {
    tetrahedra();
    open_and_odd();
    refusals_and_orientation();
    features();
    angles();
    sides();
    return check_finish("mesh topology ok");
}
