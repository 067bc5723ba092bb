// ray_hits_check.cpp — what the all-hit ray queries refuse (ray_tracer_amd/csrc/ray_hits.h: check_hits_query), in their order and
// with their messages, the block and byte arithmetic of a batch (hits_shape) at n = 0, 1, 2^30 - 1 and k = 0, 1, 8, the stack
// choice (hits_stack), and the units of the rule (include/rt_ray_hits.h: the sphere roots, the limit, the key with a tie in every
// position, the list insertion with overflow past k and k = 0; rt_hits_walk_host on a hand-made scene), on the CPU, built with
// plain g++ by tests/test_ray_hits_host.py. No array of a batch is ever dereferenced by the checks: the addresses are made up.
// Prints "ray hits ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ray_hits.h"
#include "rt_ray_hits.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

void refusals() {
    float* const O = at<float>(0x10000000u);
    float* const D = at<float>(0x20000000u);
    float* const T = at<float>(0x30000000u);
    void* const H = at<void>(0x40000000u);
    void* const C = at<void>(0x50000000u);
    for (const char* fn : {"rt_query_hits", "rt_query_hits_host"}) {
        const std::string f(fn);
        const RtRayBatch ok{O, D, T, 1000}, noLimit{O, D, nullptr, 1000};
        for (uint32_t k : {0u, 1u, 8u}) {
            CHECK(check_hits_query(fn, true, &ok, k, H, C).empty());
            CHECK(check_hits_query(fn, true, &noLimit, k, H, C).empty());
        }
        CHECK(check_hits_query(fn, true, &ok, 0, nullptr, C).empty());   // counts only
        CHECK(check_hits_query(fn, false, &ok, 8, H, C) == f + " before rt_upload_scene");
        CHECK(check_hits_query(fn, true, nullptr, 8, H, C) == f + ": the batch is NULL");
        const RtRayBatch noO{nullptr, D, T, 5}, noD{O, nullptr, T, 5};
        CHECK(check_hits_query(fn, true, &noO, 8, H, C) == f + ": origins, dirs and the output are required");
        CHECK(check_hits_query(fn, true, &noD, 8, H, C) == f + ": origins, dirs and the output are required");
        CHECK(check_hits_query(fn, true, &ok, 9, H, C) == f + ": k = 9 is above RT_HITS_MAX_K = 8");
        CHECK(check_hits_query(fn, true, &ok, 0xffffffffu, H, C) == f + ": k = 4294967295 is above RT_HITS_MAX_K = 8");
        CHECK(check_hits_query(fn, true, &ok, 8, H, nullptr) == f + ": counts and, with k > 0, hits are required");
        CHECK(check_hits_query(fn, true, &ok, 0, H, nullptr) == f + ": counts and, with k > 0, hits are required");
        CHECK(check_hits_query(fn, true, &ok, 1, nullptr, C) == f + ": counts and, with k > 0, hits are required");
        const RtRayBatch big{O, D, T, 1u << 30}, most{O, D, T, (1u << 30) - 1u}, huge{O, D, T, 0xffffffffu};
        CHECK(check_hits_query(fn, true, &big, 8, H, C) == f + ": a batch of 1073741824 rays does not fit the 30 bits of a slot id");
        CHECK(check_hits_query(fn, true, &huge, 0, nullptr, C) == f + ": a batch of 4294967295 rays does not fit the 30 bits of a slot id");
        CHECK(check_hits_query(fn, true, &most, 8, H, C).empty());
        // n == 0 succeeds whatever the pointers and k are, but not without a scene or a batch
        const RtRayBatch none{nullptr, nullptr, nullptr, 0};
        CHECK(check_hits_query(fn, true, &none, 99, nullptr, nullptr).empty());
        CHECK(check_hits_query(fn, false, &none, 99, nullptr, nullptr) == f + " before rt_upload_scene");
        // the order: the scene, the batch, origins and dirs, k, the outputs, the size
        const RtRayBatch bigNoO{nullptr, D, T, 1u << 30};
        CHECK(check_hits_query(fn, false, nullptr, 9, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_hits_query(fn, true, nullptr, 9, nullptr, nullptr) == f + ": the batch is NULL");
        CHECK(check_hits_query(fn, true, &bigNoO, 9, nullptr, nullptr) == f + ": origins, dirs and the output are required");
        CHECK(check_hits_query(fn, true, &big, 9, nullptr, nullptr) == f + ": k = 9 is above RT_HITS_MAX_K = 8");
        CHECK(check_hits_query(fn, true, &big, 8, nullptr, C) == f + ": counts and, with k > 0, hits are required");
    }
}

void arithmetic() {
    CHECK(sizeof(RtHit) == 60 && RT_HITS_MAX_K == 8 && RT_HITS_WORDS == 3);
    for (uint32_t k : {0u, 1u, 8u}) {
        const HitsShape zero = hits_shape(0, k, 256);
        CHECK(zero.searchBlocks == 0 && zero.resolveBlocks == 0 && zero.vecBytes == 0 && zero.tmaxBytes == 0 && zero.hitBytes == 0 && zero.countBytes == 0 && zero.listBytes == 0);
        struct Row { uint32_t n, blocks; } const rows[] = {{1, 1}, {63, 1}, {64, 1}, {65, 1}, {256, 1}, {257, 2}, {1024, 4}, {(1u << 30) - 1u, 1u << 22}};
        for (const Row& r : rows) {
            const HitsShape s = hits_shape(r.n, k, 256);
            CHECK(s.searchBlocks == r.blocks);
            const uint64_t slots = (uint64_t)r.n * k;
            CHECK((uint64_t)s.resolveBlocks * 256 >= slots && (k == 0 ? s.resolveBlocks == 0 : (uint64_t)(s.resolveBlocks - 1) * 256 < slots));
            CHECK(s.vecBytes == (size_t)12 * r.n && s.tmaxBytes == (size_t)4 * r.n && s.countBytes == (size_t)4 * r.n);
            CHECK(s.hitBytes == (size_t)60 * r.n * k);
            CHECK(s.listBytes == (size_t)r.blocks * 256 * 96);   // 8 entries of 3 words for every lane of the grid
        }
    }
    CHECK(hits_shape((1u << 30) - 1u, 8, 256).hitBytes == 515396075040ull);   // past 32 bits: size_t arithmetic
    CHECK(hits_shape((1u << 30) - 1u, 8, 256).resolveBlocks == (1u << 25));
    CHECK(hits_shape((1u << 30) - 1u, 1, 256).hitBytes == 64424509380ull);

    std::string e;
    CHECK(hits_stack("f", 0, &e) == 24 && hits_stack("f", 24, &e) == 24 && hits_stack("f", 25, &e) == 64 && hits_stack("f", 64, &e) == 64);
    CHECK(e.empty());
    CHECK(hits_stack("rt_query_hits", 65, &e) == 0);
    CHECK(e == "rt_query_hits: the scene's BVH has a leaf at depth 65, beyond the 64 entries of the deepest k_ray_hits");
}

struct Entry { float dst; uint32_t prim, tri; };
bool operator==(const Entry& a, const Entry& b) { return a.dst == b.dst && a.prim == b.prim && a.tri == b.tri; }

// the candidates through the insertion, at stride `stride`: the list and the number held
std::vector<Entry> through(const std::vector<Entry>& cands, uint32_t k, uint32_t stride) {
    std::vector<uint32_t> list((size_t)RT_HITS_MAX_K * RT_HITS_WORDS * stride + 1, 0xdeadbeefu);
    uint32_t have = 0;
    for (const Entry& c : cands) have = rt_hits_insert(list.data(), stride, k, have, c.dst, c.prim, c.tri);
    CHECK(have == (cands.size() < k ? (uint32_t)cands.size() : k));
    std::vector<Entry> out;
    for (uint32_t e = 0; e < have; e++)
        out.push_back(Entry{rt_u2f(list[(size_t)e * RT_HITS_WORDS * stride]), list[((size_t)e * RT_HITS_WORDS + 1) * stride], list[((size_t)e * RT_HITS_WORDS + 2) * stride]});
    // nothing past the k entries is written
    for (size_t w = (size_t)k * RT_HITS_WORDS * stride; w < list.size(); w++) CHECK(list[w] == 0xdeadbeefu);
    return out;
}

void rule_units() {
    // the limit
    bool search = false;
    CHECK(rt_hits_start(false, 0.f, &search) == RT_MISS_DST && search);
    CHECK(rt_hits_start(true, 2.5f, &search) == 2.5f && search);
    for (float bad : {0.f, -0.f, -1.f, std::numeric_limits<float>::quiet_NaN()}) { (void)rt_hits_start(true, bad, &search); CHECK(!search); }
    CHECK(rt_hits_accepts(0.f, 1.f) && rt_hits_accepts(0.5f, 1.f) && !rt_hits_accepts(1.f, 1.f) && !rt_hits_accepts(-0.5f, 1.f));
    CHECK(!rt_hits_accepts(std::numeric_limits<float>::quiet_NaN(), 1.f));

    // the sphere: from outside entry then exit, from inside a negative entry, a tangent ray one root twice, a miss
    float t0 = 0, t1 = 0;
    const rt_vec3 c = rt_v3(0, 0, 5), z = rt_v3(0, 0, 1);
    CHECK(rt_hits_sphere_roots(c, 1.f, rt_v3(0, 0, 0), z, &t0, &t1) && t0 == 4.f && t1 == 6.f);
    CHECK(rt_hits_sphere_roots(c, 1.f, rt_v3(0, 0, 5), z, &t0, &t1) && t0 == -1.f && t1 == 1.f);
    CHECK(rt_hits_sphere_roots(c, 1.f, rt_v3(1, 0, 0), z, &t0, &t1) && t0 == 5.f && t1 == 5.f);
    CHECK(!rt_hits_sphere_roots(c, 1.f, rt_v3(2, 0, 0), z, &t0, &t1));
    CHECK(rt_hits_sphere_roots(c, 0.f, rt_v3(0, 0, 0), z, &t0, &t1) && t0 == 5.f && t1 == 5.f);   // radius 0, through the centre
    CHECK(rt_hits_sphere_roots(c, 1.f, rt_v3(0, 0, 0), rt_v3(0, 0, 2), &t0, &t1) && t0 == 2.f && t1 == 3.f);   // in units of |dir|

    // the triangle and the slab test on exact figures
    const RtHitsTri h = rt_hits_triangle(rt_v3(0.25f, 0.25f, -2), z, rt_v3(0, 0, 0), rt_v3(1, 0, 0), rt_v3(0, 1, 0), false);
    CHECK(h.didHit && h.dst == 2.f && h.u == 0.25f && h.v == 0.25f && h.w == 0.5f && !h.frontFace);
    CHECK(!rt_hits_triangle(rt_v3(0.25f, 0.25f, -2), z, rt_v3(0, 0, 0), rt_v3(1, 0, 0), rt_v3(0, 1, 0), true).didHit);   // a back face, frontOnly
    CHECK(rt_hits_triangle(rt_v3(0.25f, 0.25f, -2), z, rt_v3(0, 0, 0), rt_v3(0, 1, 0), rt_v3(1, 0, 0), true).frontFace);
    CHECK(!rt_hits_triangle(rt_v3(2, 2, -2), z, rt_v3(0, 0, 0), rt_v3(1, 0, 0), rt_v3(0, 1, 0), false).didHit);
    const float inf = std::numeric_limits<float>::infinity();
    const rt_vec3 inv = rt_v3(inf, inf, 1.f);   // 1 / dir of the ray along +z
    CHECK(rt_hits_box(rt_v3(-1, -1, 3), rt_v3(1, 1, 4), rt_v3(0, 0, 0), inv) == 3.f);
    CHECK(rt_hits_box(rt_v3(-1, -1, -1), rt_v3(1, 1, 4), rt_v3(0, 0, 0), inv) == 0.f);           // from inside
    CHECK(rt_hits_box(rt_v3(-1, -1, -4), rt_v3(1, 1, -3), rt_v3(0, 0, 0), inv) == RT_MISS_DST);  // behind
    CHECK(rt_hits_box(rt_v3(2, -1, 3), rt_v3(3, 1, 4), rt_v3(0, 0, 0), inv) == RT_MISS_DST);

    // the key, a tie in every position but the one compared
    const uint32_t s0in = rt_hits_sphere_word(0, false), s0out = rt_hits_sphere_word(0, true), s1in = rt_hits_sphere_word(1, false);
    CHECK(rt_hits_is_sphere(s0out) && rt_hits_sphere_index(s1in) == 1 && rt_hits_sphere_exit(s0out) && !rt_hits_sphere_exit(s1in) && !rt_hits_is_sphere(7));
    CHECK(rt_hits_before(1.f, 5, 9, 2.f, 0, 0) && !rt_hits_before(2.f, 0, 0, 1.f, 5, 9));            // dst
    CHECK(rt_hits_before(1.f, s1in, 0, 1.f, 0, 0) && !rt_hits_before(1.f, 0, 0, 1.f, s1in, 0));      // spheres before triangles
    CHECK(rt_hits_before(1.f, s0out, 0, 1.f, s1in, 0) && !rt_hits_before(1.f, s1in, 0, 1.f, s0out, 0));   // the lower sphere
    CHECK(rt_hits_before(1.f, 3, 9, 1.f, 4, 2) && !rt_hits_before(1.f, 4, 2, 1.f, 3, 9));            // the lower object
    CHECK(rt_hits_before(1.f, 3, 2, 1.f, 3, 9) && !rt_hits_before(1.f, 3, 9, 1.f, 3, 2));            // the lower triangle
    CHECK(rt_hits_before(1.f, s0in, 0, 1.f, s0out, 0) && !rt_hits_before(1.f, s0out, 0, 1.f, s0in, 0));   // entry before exit
    CHECK(!rt_hits_before(1.f, 3, 2, 1.f, 3, 2));
    CHECK(rt_hits_before(-0.f, 3, 2, 0.f, 3, 3) && !rt_hits_before(0.f, 3, 3, -0.f, 3, 2));          // an fp32 compare: -0 == 0

    // the insertion: every order of arrival gives the sorted list; ties in every key position; overflow past k; k = 0
    const std::vector<Entry> sorted = {{0.5f, s1in, 0}, {1.f, s0in, 0}, {1.f, s0out, 0}, {1.f, s1in, 0}, {1.f, 2, 7}, {1.f, 3, 1}, {1.f, 3, 2}, {1.5f, 0, 0},
                                       {2.f, s0out, 0}, {2.f, 1, 1}, {3.f, 0, 5}, {RT_MISS_DST - 8.f, 9, 9}};
    uint32_t seed = 12345u;
    for (int round = 0; round < 200; round++) {
        std::vector<Entry> shuffled = sorted;
        for (size_t i = shuffled.size() - 1; i > 0; i--) {
            seed = seed * 747796405u + 2891336453u;
            std::swap(shuffled[i], shuffled[(seed >> 8) % (i + 1)]);
        }
        if (round == 0) shuffled = sorted;
        if (round == 1) shuffled.assign(sorted.rbegin(), sorted.rend());
        for (uint32_t k = 0; k <= (uint32_t)RT_HITS_MAX_K; k++)
            for (uint32_t stride : {1u, 64u}) {
                const std::vector<Entry> got = through(shuffled, k, stride);
                CHECK(got.size() == k);
                for (uint32_t e = 0; e < got.size(); e++) CHECK(got[e] == sorted[e], "round %d k %u stride %u entry %u", round, k, stride, e);
            }
    }
    CHECK(through({{1.f, 0, 0}, {0.5f, 0, 1}}, 8, 1) == (std::vector<Entry>{{0.5f, 0, 1}, {1.f, 0, 0}}));   // fewer than k
    CHECK(through(sorted, 0, 1).empty());
}

// A hand-made scene: one sphere, and one mesh of two parallel unit quads (4 triangles under an interior root with two leaves)
// placed twice: as it is, and moved by +10 in z. A ray along +z from (0.25, 0.25, -10) crosses everything.
void hand_made_scene() {
    Sphere spheres[2];
    memset(spheres, 0, sizeof spheres);
    spheres[0].position[2] = -5.f; spheres[0].radius = 1.f; spheres[0].materialIndex = 1;
    RayMaterial mats[2];
    memset(mats, 0, sizeof mats);
    for (RayMaterial& m : mats) m.albedoIndex = m.metalnessIndex = m.alphaIndex = m.bumpIndex = -1;
    TrianglePoint pts[8];
    memset(pts, 0, sizeof pts);
    const float xy[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
    for (int q = 0; q < 2; q++)
        for (int v = 0; v < 4; v++) {
            TrianglePoint& p = pts[4 * q + v];
            p.position[0] = xy[v][0]; p.position[1] = xy[v][1]; p.position[2] = q ? 2.f : 1.f;
            p.normal[2] = -1.f;
        }
    Triangle tris[4];
    memset(tris, 0, sizeof tris);
    for (int q = 0; q < 2; q++) {
        tris[2 * q] = Triangle{(uint32_t)(4 * q), (uint32_t)(4 * q + 2), (uint32_t)(4 * q + 1), 0, {0, 0, 0}, 0, {0, 0, 0}, 0};   // faces -z: a front face for the ray
        tris[2 * q + 1] = Triangle{(uint32_t)(4 * q), (uint32_t)(4 * q + 3), (uint32_t)(4 * q + 2), 0, {0, 0, 0}, 0, {0, 0, 0}, 0};
    }
    BVHNode nodes[3] = {{{0, 1}, {0, 1}, {1, 2}, 1, 0}, {{0, 1}, {0, 1}, {1, 1}, 0, 2}, {{0, 1}, {0, 1}, {2, 2}, 2, 2}};
    RenderObject objs[2];
    memset(objs, 0, sizeof objs);
    for (RenderObject& o : objs) { o.transformMatrix[0] = o.transformMatrix[5] = o.transformMatrix[10] = o.transformMatrix[15] = 1.f; o.bvhIndex = 0; }
    objs[1].transformMatrix[14] = 10.f;
    objs[1].materialIndex = 1;
    const RtSceneArrays s{spheres, 2, mats, 2, pts, 8, tris, 4, objs, 2, nodes, 3};

    const float o[6] = {0.25f, 0.25f, -10.f, 0.25f, 0.25f, -5.f}, d[6] = {0, 0, 1, 0, 0, 1};
    RtHit hits[16];
    uint32_t counts[2];
    const RtRayBatch rays{o, d, nullptr, 2};
    CHECK(rt_hits_walk_host(&s, 1, 2, nullptr, 0, &rays, 8, hits, counts) == 0);
    // ray 0: sphere in 4.03.., sphere out 5.96.., quads at 11, 12, 21, 22 (which of a quad's two triangles: x = y is the shared edge; 0.25, 0.25 lies on it)
    CHECK(counts[0] >= 6);
    CHECK(hits[0].isSphere == 1 && hits[0].frontFace == 1 && hits[0].materialIndex == 1 && hits[0].dst > 4.f && hits[0].dst < 4.1f);
    CHECK(hits[1].isSphere == 1 && hits[1].frontFace == 0 && hits[1].dst > 5.9f && hits[1].dst < 6.f);
    CHECK(hits[0].normal[2] < -0.9f && hits[1].normal[2] < -0.9f);   // the exit's normal is turned against the ray as well
    for (uint32_t e = 0; e + 1 < 8 && e + 1 < counts[0]; e++) CHECK(hits[e].dst <= hits[e + 1].dst);
    CHECK(hits[2].dst == 11.f && hits[2].isSphere == 0 && hits[2].objectHitIndex == 0 && hits[2].frontFace == 1 && hits[2].hitPoint[2] == 1.f);
    CHECK(hits[counts[0] < 8 ? counts[0] - 1 : 7].objectHitIndex == 1);
    if (counts[0] < 8) CHECK(hits[counts[0]].dst == RT_MISS_DST && hits[counts[0]].didHit == 0);
    // ray 1 starts inside the sphere: the exit only
    CHECK(hits[8].isSphere == 1 && hits[8].frontFace == 0 && hits[8].dst > 0.9f && hits[8].dst < 1.f && counts[1] == counts[0] - 1);
    CHECK(hits[9].isSphere == 0 && hits[9].dst == 6.f);

    // a ray off the shared edge: exactly one triangle per quad, six candidates; k = 2 truncates, the count stays
    const float o2[3] = {0.75f, 0.25f, -10.f};
    const RtRayBatch one{o2, d, nullptr, 1};
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &one, 8, hits, counts) == 0 && counts[0] == 4);
    const float want[4] = {11.f, 12.f, 21.f, 22.f};
    for (int e = 0; e < 4; e++) CHECK(hits[e].dst == want[e] && hits[e].triHitIndex == (uint32_t)(2 * (e & 1)) && hits[e].objectHitIndex == (uint32_t)(e / 2) && hits[e].materialIndex == (uint32_t)(e / 2));
    CHECK(hits[3].hitPoint[2] == 12.f && hits[3].normal[2] == -1.f);
    for (int e = 4; e < 8; e++) CHECK(hits[e].dst == RT_MISS_DST && hits[e].didHit == 0 && hits[e].objectHitIndex == 0);
    RtHit two[2];
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &one, 2, two, counts) == 0 && counts[0] == 4 && memcmp(two, hits, sizeof two) == 0);
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &one, 0, nullptr, counts) == 0 && counts[0] == 4);
    // limits: a constant bound, strict
    struct Limit { float T; uint32_t count; } const limits[] = {{11.f, 0}, {11.5f, 1}, {12.f, 1}, {21.5f, 3}, {100.f, 4}, {0.f, 0}, {-1.f, 0}, {std::numeric_limits<float>::quiet_NaN(), 0}};
    for (const Limit& lim : limits) {
        const RtRayBatch lr{o2, d, &lim.T, 1};
        CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &lr, 8, hits, counts) == 0 && counts[0] == lim.count, "limit %g: %u", (double)lim.T, counts[0]);
        CHECK(hits[lim.count].dst == RT_MISS_DST);
    }
    // refusals of the walk itself
    CHECK(rt_hits_walk_host(nullptr, 0, 0, nullptr, 0, &one, 1, hits, counts) == -1);
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &one, 9, hits, counts) == -1);
    CHECK(rt_hits_walk_host(&s, 3, 2, nullptr, 0, &one, 1, hits, counts) == -1);
    CHECK(rt_hits_walk_host(&s, 0, 3, nullptr, 0, &one, 1, hits, counts) == -1);
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &one, 1, nullptr, counts) == -1);
    const RtRayBatch none{nullptr, nullptr, nullptr, 0};
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &none, 8, nullptr, nullptr) == 0);
    nodes[0].index = 0;   // the root is its own child
    CHECK(rt_hits_walk_host(&s, 0, 2, nullptr, 0, &one, 1, hits, counts) == -1);
}

}  // namespace

int main() {
    refusals();
    arithmetic();
    rule_units();
    hand_made_scene();
    return check_finish("ray hits ok");
}
