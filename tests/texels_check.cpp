// texels_check.cpp — the host-only unit of the lightmap texel passes (ray_tracer_amd/csrc/texel_queries.h) and their rule
// (include/rt_texels.h) on the CPU, built with plain g++ by tests/test_texels_host.py: what the passes refuse, in their order and
// with their messages (made-up addresses: no array is dereferenced by the checks); watertightness and the fill rule on a quad
// and on two 5 x 5 grids of quads with mirrored windings, one with every uv vertex on texel corners and centres of a 64 x 64 map
// (covered == W x H and overlapped == 0 at every map size); owner = lowest index on hand-made overlaps; dilation against a version
// written out by hand on a 5 x 5 map; the block arithmetic at the map's border, the scan's levels and the scratch layouts.
// Prints "texel queries ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt_texels.h"
#include "texel_queries.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

// One object over one leaf: triangles in the order given
struct Mesh {
    std::vector<TrianglePoint> points;
    std::vector<Triangle> tris;
    std::vector<RenderObject> objects;
    std::vector<BVHNode> nodes;
    RtSceneArrays arrays;
    void add(const float (*uv)[2]) {
        Triangle t;
        memset(&t, 0, sizeof t);
        t.v0 = (uint32_t)points.size(); t.v1 = t.v0 + 1; t.v2 = t.v0 + 2;
        for (int k = 0; k < 3; k++) {
            TrianglePoint p;
            memset(&p, 0, sizeof p);
            p.position[0] = 2.f * uv[k][0] - 1.f; p.position[1] = 0.25f * uv[k][0] * uv[k][1]; p.position[2] = 2.f * uv[k][1] - 1.f;
            p.position[3] = uv[k][0];
            p.normal[0] = 0.1f; p.normal[1] = -1.f; p.normal[2] = 0.2f;
            p.normal[3] = uv[k][1];
            points.push_back(p);
        }
        tris.push_back(t);
    }
    const RtSceneArrays* finish(bool identity) {
        RenderObject o;
        memset(&o, 0, sizeof o);
        const float placed[16] = {1.2f, 0.3f, 0.f, 0.f, -0.2f, 0.7f, 0.4f, 0.f, 0.1f, -0.5f, 2.f, 0.f, 0.3f, -0.2f, 1.5f, 1.f};
        for (int i = 0; i < 16; i++) o.transformMatrix[i] = identity ? (i % 5 == 0 ? 1.f : 0.f) : placed[i];
        objects.assign(1, o);
        BVHNode n;
        memset(&n, 0, sizeof n);
        n.index = 0; n.triCount = (uint32_t)tris.size();
        nodes.assign(1, n);
        memset(&arrays, 0, sizeof arrays);
        arrays.triPoints = points.data(); arrays.triPointCount = (uint32_t)points.size();
        arrays.triangles = tris.data(); arrays.triangleCount = (uint32_t)tris.size();
        arrays.objects = objects.data(); arrays.objectCount = 1;
        arrays.bvhNodes = nodes.data(); arrays.bvhNodeCount = 1;
        return &arrays;
    }
};

uint32_t g_rng = 12345u;
float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return (float)(g_rng >> 8) / 16777216.f; }

void quad(Mesh& m) {
    const float a[3][2] = {{0, 0}, {1, 0}, {1, 1}}, b[3][2] = {{0, 0}, {1, 1}, {0, 1}};
    m.add(a); m.add(b);
}

// 5 x 5 quads over [0, 1]^2, interior vertices jittered by a fifth of a cell, half the quads mirrored, both diagonals in use;
// snapped: every vertex on a multiple of 1 / 128
void grid(Mesh& m, bool snapped) {
    float vu[6][6], vv[6][6];
    for (int i = 0; i <= 5; i++)
        for (int j = 0; j <= 5; j++) {
            vu[i][j] = ((float)i + (rnd() - 0.5f) * 0.4f) / 5.f;
            vv[i][j] = ((float)j + (rnd() - 0.5f) * 0.4f) / 5.f;
            if (snapped) { vu[i][j] = std::nearbyint(vu[i][j] * 128.f) / 128.f; vv[i][j] = std::nearbyint(vv[i][j] * 128.f) / 128.f; }
            if (i == 0) vu[i][j] = 0.f;
            if (i == 5) vu[i][j] = 1.f;
            if (j == 0) vv[i][j] = 0.f;
            if (j == 5) vv[i][j] = 1.f;
        }
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) {
            const float a[2] = {vu[i][j], vv[i][j]}, b[2] = {vu[i + 1][j], vv[i + 1][j]}, c[2] = {vu[i + 1][j + 1], vv[i + 1][j + 1]}, d[2] = {vu[i][j + 1], vv[i][j + 1]};
            const float* t[2][3] = {{a, b, c}, {a, c, d}};
            if ((i * 5 + j) % 3 == 0) { t[0][2] = d; t[1][0] = b; t[1][1] = c; t[1][2] = d; }
            for (int k = 0; k < 2; k++) {
                const bool mirrored = (i + j) % 2 != 0;
                const float uv[3][2] = {{t[k][0][0], t[k][0][1]}, {t[k][mirrored ? 2 : 1][0], t[k][mirrored ? 2 : 1][1]}, {t[k][mirrored ? 1 : 2][0], t[k][mirrored ? 1 : 2][1]}};
                m.add(uv);
            }
        }
}

void refusals() {
    void* const OUT = at<void>(0x40000000u);
    for (const char* fn : {"rt_bake_texels", "rt_bake_texels_host", "rt_bake_lightmap"}) {
        const std::string f(fn);
        const auto check = [&](bool scene, const void* out, uint32_t object, uint32_t w, uint32_t h, uint32_t triTotal = 12u) {
            return check_texel_bake(fn, scene, out, object, 3u, w, h, triTotal);
        };
        CHECK(check(true, OUT, 0, 64, 64).empty());
        CHECK(check(true, OUT, 2, 1, 8192).empty());
        CHECK(check(true, OUT, 2, 8192, 1).empty());
        CHECK(check(false, OUT, 0, 64, 64) == f + " before rt_upload_scene");
        CHECK(check(true, nullptr, 0, 64, 64) == f + ": the output is required");
        CHECK(check(true, OUT, 3, 64, 64) == f + ": object 3 of 3");
        CHECK(check(true, OUT, 0xffffffffu, 64, 64) == f + ": object 4294967295 of 3");
        CHECK(check(true, OUT, 0, 0, 64) == f + ": a map of 0 x 64 texels; width and height must be in 1 .. 8192");
        CHECK(check(true, OUT, 0, 64, 8193) == f + ": a map of 64 x 8193 texels; width and height must be in 1 .. 8192");
        CHECK(check(true, OUT, 0, 0xffffffffu, 1) == f + ": a map of 4294967295 x 1 texels; width and height must be in 1 .. 8192");
        CHECK(check(true, OUT, 1, 64, 64, 0xffffffffu) == f + ": the triangles of object 1's mesh are not one contiguous range");
        // the order: each refusal with everything after it wrong as well
        CHECK(check(false, nullptr, 9, 0, 0, 0xffffffffu) == f + " before rt_upload_scene");
        CHECK(check(true, nullptr, 9, 0, 0, 0xffffffffu) == f + ": the output is required");
        CHECK(check(true, OUT, 9, 0, 0, 0xffffffffu) == f + ": object 9 of 3");
        CHECK(check(true, OUT, 1, 0, 0, 0xffffffffu) == f + ": a map of 0 x 0 texels; width and height must be in 1 .. 8192");
    }
    const std::string f("rt_bake_lightmap");
    const RtIrradianceParams ok{64, 8, 0, 0, 0.00001f}, progressive{64, 8, 1, 0, 0.00001f};
    CHECK(check_lightmap("rt_bake_lightmap", &ok, 254, OUT).empty());
    CHECK(check_lightmap("rt_bake_lightmap", nullptr, 255, nullptr) == f + ": the params are required");
    CHECK(check_lightmap("rt_bake_lightmap", &progressive, 255, nullptr) == f + ": one shot; progressive refinement goes through rt_texels_compact and rt_query_irradiance");
    CHECK(check_lightmap("rt_bake_lightmap", &ok, 255, nullptr) == f + ": at most 254 dilation passes");
    CHECK(check_lightmap("rt_bake_lightmap", &ok, 2, nullptr) == f + ": the fill plane is required");
    const std::string p("rt_texels_scatter");
    CHECK(check_texel_pass("rt_texels_scatter", true, 64, 64, 0).empty());
    CHECK(check_texel_pass("rt_texels_scatter", true, 8192ull * 8192ull, 0, 254).empty());
    CHECK(check_texel_pass("rt_texels_scatter", false, 0, 65, 255) == p + ": every array is required");
    CHECK(check_texel_pass("rt_texels_scatter", true, 0, 65, 255) == p + ": 0 texels; a map has 1 .. 8192 x 8192");
    CHECK(check_texel_pass("rt_texels_scatter", true, 8192ull * 8192ull + 1, 65, 255) == p + ": 67108865 texels; a map has 1 .. 8192 x 8192");
    CHECK(check_texel_pass("rt_texels_scatter", true, 64, 65, 255) == p + ": 65 covered texels of 64");
    CHECK(check_texel_pass("rt_texels_scatter", true, 64, 64, 255) == p + ": at most 254 dilation passes");
    // the host forms
    Mesh m;
    quad(m);
    const RtSceneArrays* s = m.finish(false);
    std::vector<RtTexel> t(64);
    RtTexelStats st;
    CHECK(rt_texels_exhaustive_host(nullptr, 0, 8, 8, t.data(), &st) == -1);
    CHECK(rt_texels_exhaustive_host(s, 0, 8, 8, nullptr, &st) == -1);
    CHECK(rt_texels_exhaustive_host(s, 1, 8, 8, t.data(), &st) == -1);
    CHECK(rt_texels_exhaustive_host(s, 0, 0, 8, t.data(), &st) == -1);
    CHECK(rt_texels_exhaustive_host(s, 0, 8, 8193, t.data(), &st) == -1);
    CHECK(rt_texels_exhaustive_host(s, 0, 8, 8, t.data(), nullptr) == 0);
    float rgba[4] = {0, 0, 0, 0};
    uint8_t fill[1] = {0};
    CHECK(rt_dilate_texels_host(1, 1, 255, rgba, fill) == -1 && rt_dilate_texels_host(0, 1, 1, rgba, fill) == -1 && rt_dilate_texels_host(1, 1, 1, nullptr, fill) == -1);
    CHECK(rt_dilate_texels_host(1, 1, 254, rgba, fill) == 0 && fill[0] == 0);
}

const uint32_t MAPS[][2] = {{64, 64}, {37, 23}, {1, 1}, {8192, 1}, {1, 8192}, {8, 8}, {200, 300}};

void watertight() {
    for (int which = 0; which < 4; which++) {
        Mesh m;
        if (which == 0) quad(m);
        else grid(m, which == 2);
        const RtSceneArrays* s = m.finish(which == 3);
        for (const auto& map : MAPS) {
            const uint32_t w = map[0], h = map[1];
            g_where = std::string(which == 0 ? "quad" : which == 2 ? "snapped grid" : "grid") + " " + std::to_string(w) + " x " + std::to_string(h);
            std::vector<RtTexel> t((size_t)w * h);
            RtTexelStats st;
            CHECK(rt_texels_exhaustive_host(s, 0, w, h, t.data(), &st) == 0);
            CHECK(st.covered == w * h && st.overlapped == 0 && st.skippedTriangles == 0 && st.degenerateTexels == 0, "covered %u of %u, overlapped %u, skipped %u",
                  st.covered, w * h, st.overlapped, st.skippedTriangles);
            bool ok = true;
            for (size_t i = 0; i < t.size() && ok; i++) {
                const RtTexel& r = t[i];
                const float len = std::sqrt(r.normal[0] * r.normal[0] + r.normal[1] * r.normal[1] + r.normal[2] * r.normal[2]);
                ok = r.state == 1 && r.triIndex < m.tris.size() && r.uv[0] >= 0.f && r.uv[1] >= 0.f && r.uv[0] + r.uv[1] <= 1.00001f && std::fabs(len - 1.f) < 1e-5f &&
                     r._pad[0] == 0 && r._pad[1] == 0;
            }
            CHECK(ok);
        }
    }
    g_where.clear();
    // edges through centres: a 4 x 4 map split along its diagonal and along the line x = 2 (a centre line of no texel) and x = 1.5
    // (through the centres of column 1): every centre belongs to exactly one of the two triangles or rectangles
    {
        Mesh m;
        const float a[3][2] = {{0, 0}, {0.375f, 0}, {0.375f, 1}}, b[3][2] = {{0, 0}, {0.375f, 1}, {0, 1}}, c[3][2] = {{0.375f, 0}, {1, 0}, {1, 1}}, d[3][2] = {{0.375f, 0}, {1, 1}, {0.375f, 1}};
        m.add(a); m.add(b); m.add(c); m.add(d);
        std::vector<RtTexel> t(16);
        RtTexelStats st;
        CHECK(rt_texels_exhaustive_host(m.finish(false), 0, 4, 4, t.data(), &st) == 0);
        CHECK(st.covered == 16 && st.overlapped == 0);
        // the centres of column 1 lie on the shared vertical edge u = 0.375: it is the left edge of the right-hand pair
        for (int y = 0; y < 4; y++) CHECK(t[4 * y + 1].triIndex >= 2 && t[4 * y].triIndex < 2, "row %d: %u %u", y, t[4 * y].triIndex, t[4 * y + 1].triIndex);
    }
}

void owners() {
    // three triangles over the whole map and one over its lower left half, in this order: the owner is always triangle 0, every
    // texel overlapped; without the first, triangle 1
    const float whole[3][2] = {{-1, -1}, {3, -1}, {-1, 3}}, mirrored[3][2] = {{-1, -1}, {-1, 3}, {3, -1}}, half[3][2] = {{0, 0}, {1, 0}, {0, 1}};
    for (int drop = 0; drop < 2; drop++) {
        Mesh m;
        if (!drop) m.add(whole);
        m.add(mirrored); m.add(whole); m.add(half);
        std::vector<RtTexel> t(37 * 23);
        RtTexelStats st;
        CHECK(rt_texels_exhaustive_host(m.finish(false), 0, 37, 23, t.data(), &st) == 0);
        CHECK(st.covered == 37 * 23 && st.overlapped == 37 * 23);
        bool ok = true;
        for (const RtTexel& r : t) ok = ok && r.triIndex == 0 && r.state == 3;
        CHECK(ok);
    }
    // a small triangle listed first owns its texels, the rest belongs to the big one behind it, overlapped only where both cover
    Mesh m;
    const float small[3][2] = {{0.25f, 0.25f}, {0.75f, 0.25f}, {0.25f, 0.75f}};
    m.add(small); m.add(whole);
    std::vector<RtTexel> t(64);
    RtTexelStats st;
    CHECK(rt_texels_exhaustive_host(m.finish(false), 0, 8, 8, t.data(), &st) == 0);
    uint32_t first = 0;
    for (const RtTexel& r : t) {
        CHECK((r.triIndex == 0 && r.state == 3) || (r.triIndex == 1 && r.state == 1));
        first += r.triIndex == 0;
    }
    CHECK(st.covered == 64 && st.overlapped == first && first > 0 && first < 20, "%u", first);
    // skipped: a NaN, an infinity, two equal corners, collinear corners, a uv beyond 2^27 sub-texels
    Mesh sk;
    const float nanUv[3][2] = {{0, 0}, {NAN, 0}, {0, 1}}, infUv[3][2] = {{0, 0}, {1, INFINITY}, {0, 1}}, equal[3][2] = {{0.2f, 0.2f}, {0.2f, 0.2f}, {0.9f, 0.1f}},
                line[3][2] = {{0, 0}, {0.5f, 0.5f}, {1, 1}}, far[3][2] = {{0, 0}, {70000.f, 0}, {0, 1}};
    sk.add(nanUv); sk.add(infUv); sk.add(equal); sk.add(line); sk.add(far);
    CHECK(rt_texels_exhaustive_host(sk.finish(false), 0, 8, 8, t.data(), &st) == 0);
    CHECK(st.covered == 0 && st.skippedTriangles == 5, "%u %u", st.covered, st.skippedTriangles);
    bool zero = true;
    for (size_t i = 0; i < sizeof(RtTexel) * 64; i++) zero = zero && ((const unsigned char*)t.data())[i] == 0;
    CHECK(zero);
}

void dilation() {
    // 5 x 5, one filled texel in a corner and one in the middle of the far edge
    float rgba[25][4];
    uint8_t fill[25];
    memset(rgba, 0, sizeof rgba);
    memset(fill, 0, sizeof fill);
    const float A[4] = {1.f, 2.f, 4.f, 1.f}, B[4] = {0.5f, 0.25f, 3.f, 1.f};
    memcpy(rgba[0], A, sizeof A); fill[0] = 1;            // (0, 0)
    memcpy(rgba[4 * 5 + 2], B, sizeof B); fill[4 * 5 + 2] = 1;   // (2, 4)
    float one[25][4];
    uint8_t oneFill[25];
    memcpy(one, rgba, sizeof one); memcpy(oneFill, fill, sizeof fill);
    CHECK(rt_dilate_texels_host(5, 5, 1, &one[0][0], oneFill) == 0);
    // pass 1 by hand: the three neighbours of (0, 0) copy A / 1, the five of (2, 4) copy B / 1; nothing else
    const int nearA[3] = {1, 5, 6}, nearB[5] = {3 * 5 + 1, 3 * 5 + 2, 3 * 5 + 3, 4 * 5 + 1, 4 * 5 + 3};
    for (int i = 0; i < 25; i++) {
        bool a = false, b = false;
        for (int k : nearA) a = a || k == i;
        for (int k : nearB) b = b || k == i;
        if (i == 0 || i == 22) CHECK(oneFill[i] == 1 && memcmp(one[i], rgba[i], 16) == 0);
        else if (a) CHECK(oneFill[i] == 2 && one[i][0] == A[0] && one[i][1] == A[1] && one[i][2] == A[2] && one[i][3] == 0.f);
        else if (b) CHECK(oneFill[i] == 2 && one[i][0] == B[0] && one[i][1] == B[1] && one[i][2] == B[2] && one[i][3] == 0.f);
        else CHECK(oneFill[i] == 0 && one[i][0] == 0.f && one[i][3] == 0.f, "texel %d", i);
    }
    // pass 2 by hand at (1, 2): its filled neighbours after pass 1 are, in the rule's order, (0, 1), (1, 1) [row above] and
    // (1, 3), (2, 3) [row below, from B]: ((A + A) + B) + B over 4
    float two[25][4];
    uint8_t twoFill[25];
    memcpy(two, rgba, sizeof two); memcpy(twoFill, fill, sizeof fill);
    CHECK(rt_dilate_texels_host(5, 5, 2, &two[0][0], twoFill) == 0);
    const int i12 = 2 * 5 + 1;
    CHECK(twoFill[i12] == 3 && two[i12][3] == 0.f);
    for (int ch = 0; ch < 3; ch++) CHECK(two[i12][ch] == (((0.f + A[ch]) + A[ch]) + B[ch] + B[ch]) / 4.f, "channel %d: %g", ch, two[i12][ch]);
    // pass 1's texels keep their fill of 2 and their values; two passes equal one pass twice
    float again[25][4];
    uint8_t againFill[25];
    memcpy(again, one, sizeof one); memcpy(againFill, oneFill, sizeof oneFill);
    // (a second single pass numbers its texels 2, not 3: only the values are compared)
    CHECK(rt_dilate_texels_host(5, 5, 1, &again[0][0], againFill) == 0);
    CHECK(memcmp(again, two, sizeof two) == 0);
    for (int i = 0; i < 25; i++) CHECK((twoFill[i] == 3) == (oneFill[i] == 0 && againFill[i] == 2) && (twoFill[i] == 3 || twoFill[i] == oneFill[i]));
    // no wrap: a filled texel at the right border does not reach column 0
    float edge[25][4];
    uint8_t edgeFill[25];
    memset(edge, 0, sizeof edge); memset(edgeFill, 0, sizeof edgeFill);
    memcpy(edge[1 * 5 + 4], A, sizeof A); edgeFill[1 * 5 + 4] = 1;
    CHECK(rt_dilate_texels_host(5, 5, 1, &edge[0][0], edgeFill) == 0);
    for (int y = 0; y < 5; y++) CHECK(edgeFill[y * 5] == 0 && edgeFill[y * 5 + 1] == 0);
    // zero passes do nothing
    CHECK(rt_dilate_texels_host(5, 5, 0, &edge[0][0], edgeFill) == 0 && edgeFill[1 * 5 + 3] == 2);
}

void arithmetic() {
    CHECK(texel_groups(0, 256) == 0 && texel_groups(1, 256) == 1 && texel_groups(256, 256) == 1 && texel_groups(257, 256) == 2);
    CHECK(texel_groups(8192ull * 8192ull, 64) == 1u << 20);
    // the blocks of a box at the map's border: a triangle over the whole 37 x 23 map touches 5 x 3 blocks, the last ones ragged
    const float whole[6] = {-1, -1, 3, -1, -1, 3};
    rt_texel_tri t;
    rt_texel_box b;
    CHECK(rt_texel_setup(whole, 37, 23, &t) && rt_texel_bounds(&t, 37, 23, &b));
    CHECK(b.x0 == 0 && b.y0 == 0 && b.x1 == 36 && b.y1 == 22 && rt_texel_box_blocks(&b) == 15);
    uint32_t x, y;
    rt_texel_box_block(&b, 14, &x, &y);
    CHECK(x == 32 && y == 16);
    rt_texel_box_block(&b, 5, &x, &y);
    CHECK(x == 0 && y == 8);
    bool skipped;
    CHECK(rt_texel_tri_blocks(whole, 1024, 1024, &skipped) == 1u << 14 && !skipped);
    CHECK(rt_texel_tri_blocks(whole, 8192, 8192, &skipped) == 1u << 20 && !skipped);
    CHECK(rt_texel_tri_blocks(whole, 8192, 1, &skipped) == 1024 && rt_texel_tri_blocks(whole, 1, 1, &skipped) == 1);
    // a triangle wholly outside the map, and one between centres, have no items and are not skipped
    const float outside[6] = {1.5f, 0.2f, 1.9f, 0.2f, 1.5f, 0.8f}, between[6] = {0.501f, 0.501f, 0.504f, 0.501f, 0.502f, 0.504f};
    CHECK(rt_texel_tri_blocks(outside, 64, 64, &skipped) == 0 && !skipped);
    CHECK(rt_texel_tri_blocks(between, 64, 64, &skipped) == 0 && !skipped);
    // a box that ends exactly on a centre includes it; one that ends just before does not
    const float onCentre[6] = {0.f, 0.f, 8.5f / 64.f, 0.f, 0.f, 8.5f / 64.f};
    CHECK(rt_texel_setup(onCentre, 64, 64, &t) && rt_texel_bounds(&t, 64, 64, &b) && b.x1 == 8 && b.y0 == 55 && b.y1 == 63 && rt_texel_box_blocks(&b) == 4);
    // the block test: a block far outside an edge is outside, one the triangle crosses is not
    const float lower[6] = {0, 0, 1, 0, 0, 1};
    CHECK(rt_texel_setup(lower, 64, 64, &t));
    CHECK(rt_texel_block_outside(&t, 56, 0) && !rt_texel_block_outside(&t, 0, 56) && !rt_texel_block_outside(&t, 24, 32));
    // snapping: ties to even, both signs
    CHECK(rt_texel_rint(0.5) == 0 && rt_texel_rint(1.5) == 2 && rt_texel_rint(2.5) == 2 && rt_texel_rint(-0.5) == 0 && rt_texel_rint(-1.5) == -2 && rt_texel_rint(3.49) == 3);
    int64_t v;
    CHECK(rt_texel_snap(1.f, false, 8192, &v) && v == 2097152 && rt_texel_snap(0.25f, true, 64, &v) && v == 12288);
    CHECK(rt_texel_snap(63.99f, false, 8192, &v) && !rt_texel_snap(64.f, false, 8192, &v) && !rt_texel_snap(-64.f, false, 8192, &v));
    // the scan's levels
    ScanLevels l = scan_levels(1);
    CHECK(l.levels == 2 && l.count[0] == 1 && l.count[1] == 1 && l.offset[0] == 0 && l.offset[1] == 1 && l.elems == 2);
    l = scan_levels(256);
    CHECK(l.levels == 2 && l.count[1] == 1 && l.elems == 2);
    l = scan_levels(257);
    CHECK(l.levels == 3 && l.count[1] == 2 && l.count[2] == 1 && l.offset[1] == 2 && l.offset[2] == 3 && l.elems == 4);
    l = scan_levels((1ull << 28) + 1);
    CHECK(l.levels == 5 && l.count[1] == (1u << 20) + 1 && l.count[2] == 4097 && l.count[3] == 17 && l.count[4] == 1);
    CHECK(l.elems == (1ull << 20) + 1 + 4097 + 17 + 1 + 1);
    l = scan_levels(8192ull * 8192ull);
    CHECK(l.levels == 5 && l.count[1] == 1u << 18 && l.count[2] == 1024 && l.count[3] == 4 && l.count[4] == 1);
    // the scratch layouts: aligned parts in order, nothing overlaps
    const TexelScratch s = texel_scratch(50, 37, 23);
    CHECK(s.stats == 0 && s.owner == 256 && s.overlapped == 256 + 3584 && s.counts == s.overlapped + 1024 && s.offsets == s.counts + 256 && s.sums == s.offsets + 512 &&
          s.bytes == s.sums + 256);
    const LightmapScratch g = lightmap_scratch(37, 23);
    CHECK(g.texels == 0 && g.points == 40960 && g.normals == g.points + 10240 && g.index == g.normals + 10240 && g.count == g.index + 3584 && g.values == g.count + 256 &&
          g.bytes == g.values + 13824);
    CHECK(sizeof(RtTexel) == 48 && sizeof(RtTexelStats) == 16);
}

}  // namespace

int main() {
    refusals();
    watertight();
    owners();
    dilation();
    arithmetic();
    return check_finish("texel queries ok");
}
