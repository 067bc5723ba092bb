// irradiance_check.cpp — the host-only unit of the baked-light queries (ray_tracer_amd/csrc/irradiance_queries.h) on the CPU, built
// with plain g++ by tests/test_irradiance_host.py: what the queries refuse, in their order and with their messages (made-up
// addresses: no array is dereferenced by the checks), the chunks of whole points for n x S straddling the piece cap, the byte
// counts and the scratch layout, the rays' ids and origins (rt_irradiance_rays_host), and the order of the gather's sum
// (rt_irradiance_gather_host) against a fold written out here as a tree, with values whose sum depends on the order.
// Prints "irradiance queries ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "irradiance_queries.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

const uint64_t K = 1024;   // "radiance_max_kslots" 1

void refusals() {
    float* const P = at<float>(0x10000000u);
    float* const N = at<float>(0x20000000u);
    void* const OUT = at<void>(0x40000000u);
    const RtIrradianceParams ok{64, 8, 0, 0, 0.00001f};
    const char* const fns[4] = {"rt_query_irradiance", "rt_query_irradiance_host", "rt_query_sh_probes", "rt_query_sh_probes_host"};
    for (int k = 0; k < 4; k++) {
        const char* fn = fns[k];
        const bool sphere = k >= 2;
        const std::string f(fn);
        const std::string arrays = f + (sphere ? ": points and the output are required" : ": points, normals and the output are required");
        const auto check = [&](bool scene, const RtPointNormalBatch* b, const RtIrradianceParams* p, const void* out, uint64_t maxSlots = 24ull << 20) {
            return check_irradiance_query(fn, sphere, scene, b, p, out, maxSlots);
        };
        const RtPointNormalBatch batch{P, N, 1000};
        CHECK(check(true, &batch, &ok, OUT).empty());
        const RtIrradianceParams edge{(1u << 24) - 1u, (1u << 28) - 2u, 1, 0xffffffffu, 0.f};
        CHECK(check(true, &batch, &edge, OUT).empty());
        const RtPointNormalBatch most{P, N, (1u << 30) - 1u};
        CHECK(check(true, &most, &ok, OUT).empty());
        // every refusal
        CHECK(check(false, &batch, &ok, OUT) == f + " before rt_upload_scene");
        CHECK(check(true, nullptr, &ok, OUT) == f + ": the batch and the params are required");
        CHECK(check(true, &batch, nullptr, OUT) == f + ": the batch and the params are required");
        const RtPointNormalBatch noP{nullptr, N, 5}, noN{P, nullptr, 5};
        CHECK(check(true, &noP, &ok, OUT) == arrays);
        CHECK(check(true, &batch, &ok, nullptr) == arrays);
        if (sphere) CHECK(check(true, &noN, &ok, OUT).empty());   // the probe form ignores the normals
        else CHECK(check(true, &noN, &ok, OUT) == arrays);
        const RtIrradianceParams noSamples{0, 8, 0, 0, 0.f}, manySamples{1u << 24, 8, 0, 0, 0.f}, mostSamples{0xffffffffu, 8, 0, 0, 0.f};
        for (const RtIrradianceParams* p : {&noSamples, &manySamples, &mostSamples})
            CHECK(check(true, &batch, p, OUT) == f + ": samples must be in 1 .. 2^24 - 1");
        const RtIrradianceParams deep{4, (1u << 28) - 1u, 0, 0, 0.f}, deepest{4, 0xffffffffu, 0, 0, 0.f};
        CHECK(check(true, &batch, &deep, OUT) == f + ": bounceLimit needs more than 28 bits");
        CHECK(check(true, &batch, &deepest, OUT) == f + ": bounceLimit needs more than 28 bits");
        for (float b : {-1e-6f, -INFINITY, INFINITY, NAN}) {
            const RtIrradianceParams bad{4, 8, 0, 0, b};
            CHECK(check(true, &batch, &bad, OUT) == f + ": bias must be finite and >= 0");
        }
        const RtIrradianceParams negZero{4, 8, 0, 0, -0.f};
        CHECK(check(true, &batch, &negZero, OUT).empty());
        // samples against the piece cap: S == cap passes, cap + 1 is refused
        const RtIrradianceParams atCap{1024, 8, 0, 0, 0.f}, pastCap{1025, 8, 0, 0, 0.f};
        CHECK(check(true, &batch, &atCap, OUT, K).empty());
        CHECK(check(true, &batch, &pastCap, OUT, K) == f + ": the 1025 rays of a point do not fit a piece of 1024 rays (radiance_max_kslots)");
        const RtPointNormalBatch big{P, N, 1u << 30}, huge{P, N, 0xffffffffu};
        CHECK(check(true, &big, &ok, OUT) == f + ": a batch of 1073741824 points does not fit the 30 bits of a slot id");
        CHECK(check(true, &huge, &ok, OUT) == f + ": a batch of 4294967295 points does not fit the 30 bits of a slot id");
        // n == 0 succeeds whatever the arrays and the params hold, but not without a scene, a batch or params
        const RtPointNormalBatch none{nullptr, nullptr, 0};
        CHECK(check(true, &none, &noSamples, nullptr).empty());
        CHECK(check(false, &none, &ok, nullptr) == f + " before rt_upload_scene");
        CHECK(check(true, &none, nullptr, nullptr) == f + ": the batch and the params are required");
        // the order: each refusal with everything after it wrong as well
        const RtIrradianceParams bad5{0, 0xffffffffu, 0, 0, NAN}, bad6{1025, 0xffffffffu, 0, 0, NAN}, bad7{1025, 8, 0, 0, NAN}, bad8{1025, 8, 0, 0, 0.f};
        const RtPointNormalBatch w4{nullptr, nullptr, 1u << 30}, w5{P, N, 1u << 30};
        CHECK(check(false, nullptr, nullptr, nullptr, K) == f + " before rt_upload_scene");
        CHECK(check(false, &w4, &bad5, nullptr, K) == f + " before rt_upload_scene");
        CHECK(check(true, nullptr, &bad5, nullptr, K) == f + ": the batch and the params are required");
        CHECK(check(true, &w4, nullptr, nullptr, K) == f + ": the batch and the params are required");
        CHECK(check(true, &w4, &bad5, nullptr, K) == arrays);
        CHECK(check(true, &w5, &bad5, nullptr, K) == arrays);
        CHECK(check(true, &w5, &bad5, OUT, K) == f + ": samples must be in 1 .. 2^24 - 1");
        CHECK(check(true, &w5, &bad6, OUT, K) == f + ": bounceLimit needs more than 28 bits");
        CHECK(check(true, &w5, &bad7, OUT, K) == f + ": bias must be finite and >= 0");
        CHECK(check(true, &w5, &bad8, OUT, K) == f + ": the 1025 rays of a point do not fit a piece of 1024 rays (radiance_max_kslots)");
        CHECK(check(true, &w5, &atCap, OUT, K) == f + ": a batch of 1073741824 points does not fit the 30 bits of a slot id");
    }
    RtIrradianceParams d{9, 9, 9, 9, 9.f};
    rt_irradiance_params_default(&d);
    CHECK(d.samples == 64 && d.bounceLimit == 8 && d.progressive == 0 && d.frameCount == 0 && d.bias == 0.00001f);
    rt_irradiance_params_default(nullptr);
}

// the chunks cover [0, n) in order, whole points, none empty, every chunk's rays within the cap, only the last one short
void cover(uint32_t n, uint32_t S, uint64_t maxSlots, uint32_t expectPer, uint32_t expectChunks) {
    g_where = "n " + std::to_string(n) + " S " + std::to_string(S);
    const uint64_t cap = (uint64_t)std::min<uint64_t>(std::max<uint64_t>(maxSlots, 1), (1u << 30) - 1u);
    const uint32_t per = irradiance_chunk_points(S, maxSlots), chunks = irradiance_chunk_count(n, S, maxSlots);
    CHECK(per == expectPer && chunks == expectChunks, "per %u chunks %u", per, chunks);
    uint64_t at = 0;
    for (uint32_t k = 0; k < chunks; k++) {
        const IrradianceChunk c = irradiance_chunk(n, S, maxSlots, k);
        CHECK(c.first == at && c.n >= 1 && (uint64_t)c.n * S <= cap);
        CHECK(k + 1 == chunks || c.n == per);
        at += c.n;
    }
    CHECK(at == n);
    const IrradianceChunk past = irradiance_chunk(n, S, maxSlots, chunks);
    CHECK(past.first == n && past.n == 0);
    g_where.clear();
}

void chunks() {
    cover(0, 64, K, 16, 0); cover(1, 64, K, 16, 1); cover(16, 64, K, 16, 1); cover(17, 64, K, 16, 2); cover(37, 64, K, 16, 3);
    cover(37, 65, K, 15, 3); cover(37, 200, K, 5, 8); cover(37, 1, K, 1024, 1); cover(1025, 1, K, 1024, 2); cover(37, 5, K, 204, 1);
    cover(205, 5, K, 204, 2);   // 1020 rays fit, 1025 do not
    cover(3, 1024, K, 1, 3);    // S equal to the cap: one point per chunk
    CHECK(irradiance_chunk_points(1025, K) == 0 && irradiance_chunk_count(3, 1025, K) == 0);   // cap + 1: refused before (above)
    CHECK(irradiance_chunk_points(0, K) == 0 && irradiance_chunk_count(3, 0, K) == 0);
    const IrradianceChunk last = irradiance_chunk(37, 64, K, 2);
    CHECK(last.first == 32 && last.n == 5);
    cover(65536, 64, 24ull << 20, 393216, 1);                          // the default cap: 24 M paths
    cover((1u << 30) - 1u, 64, 24ull << 20, 393216, 2731);
    cover((1u << 30) - 1u, (1u << 24) - 1u, 1ull << 40, 64, 16777216);   // the largest of everything
}

void shape() {
    for (uint32_t n : {1u, 37u, 64u, (1u << 30) - 1u})
        for (int ids = 0; ids < 2; ids++) {
            const IrradianceShape e = irradiance_shape(n, ids != 0, false), p = irradiance_shape(n, ids != 0, true);
            CHECK(e.vecBytes == (size_t)12 * n && e.idBytes == (ids ? (size_t)4 * n : 0) && e.outBytes == (size_t)16 * n);
            CHECK(p.vecBytes == (size_t)12 * n && p.idBytes == e.idBytes && p.outBytes == (size_t)108 * n);
        }
    CHECK(irradiance_shape((1u << 30) - 1u, true, true).outBytes == 115964116884ull);   // past 32 bits: size_t arithmetic
    for (uint32_t rays : {1u, 1020u, 1024u, (1u << 30) - 1u}) {
        const IrradianceScratch s = irradiance_scratch(rays);
        const size_t r = rays;
        CHECK(s.radiance == 0 && s.origins == 16 * r && s.dirs == 28 * r && s.ids == 40 * r && s.bytes == 44 * r);
    }
}

void rays() {
    const float P[3][3] = {{0.5f, -0.25f, 2.f}, {-1.f, 3.f, 0.125f}, {7.f, 8.f, 9.f}};
    const float N[3][3] = {{0.f, -1.f, 0.f}, {1.f, 0.f, 0.f}, {0.6f, 0.f, -0.8f}};
    const uint32_t ids[3] = {7u, 0xffffffffu, 0x33333334u};   // x 5 wraps for the last two
    const RtPointNormalBatch b{&P[0][0], &N[0][0], 3};
    const RtIrradianceParams p{5, 8, 0, 3, 0.25f};
    for (int sphere = 0; sphere < 2; sphere++) {
        g_where = sphere ? "probe rays" : "irradiance rays";
        float o[15][3], d[15][3];
        uint32_t id[15];
        CHECK(rt_irradiance_rays_host(&b, ids, &p, sphere, 0, 3, &o[0][0], &d[0][0], id) == 0);
        for (uint32_t i = 0; i < 3; i++)
            for (uint32_t s = 0; s < 5; s++) {
                const uint32_t r = i * 5 + s;
                CHECK(id[r] == (uint32_t)(ids[i] * 5u + s));
                for (int c = 0; c < 3; c++) CHECK(bits(o[r][c]) == bits(sphere ? P[i][c] : P[i][c] + (N[i][c] * 1.f) * 0.25f));
                const double len = std::sqrt((double)d[r][0] * d[r][0] + (double)d[r][1] * d[r][1] + (double)d[r][2] * d[r][2]);
                CHECK(std::fabs(len - 1.0) < 1e-5, "length %.9g", len);
                if (!sphere) CHECK((double)d[r][0] * N[i][0] + (double)d[r][1] * N[i][1] + (double)d[r][2] * N[i][2] > -1e-6);
            }
        CHECK(id[5] == 0xfffffffbu && id[9] == 0xffffffffu && id[10] == 4u);   // 0xffffffff x 5 = -5; 0x33333334 x 5 = 2^32 + 4
        // without ids the point's index; a sub-range is the slice of the whole; the directions do not depend on the position
        uint32_t plain[15];
        float o2[15][3], d2[15][3];
        CHECK(rt_irradiance_rays_host(&b, nullptr, &p, sphere, 0, 3, &o2[0][0], &d2[0][0], plain) == 0);
        for (uint32_t r = 0; r < 15; r++) CHECK(plain[r] == r);
        float o1[5][3], d1[5][3];
        uint32_t id1[5];
        CHECK(rt_irradiance_rays_host(&b, ids, &p, sphere, 1, 1, &o1[0][0], &d1[0][0], id1) == 0);
        CHECK(!memcmp(o1, o[5], sizeof o1) && !memcmp(d1, d[5], sizeof d1) && !memcmp(id1, id + 5, sizeof id1));
        // another frame, other directions
        RtIrradianceParams q = p;
        q.frameCount = 4;
        CHECK(rt_irradiance_rays_host(&b, ids, &q, sphere, 0, 3, &o2[0][0], &d2[0][0], plain) == 0);
        CHECK(memcmp(d2, d, sizeof d) != 0 && !memcmp(plain, id, sizeof id));
        // refused
        CHECK(rt_irradiance_rays_host(&b, ids, &p, sphere, 2, 2, &o[0][0], &d[0][0], id) == -1);
        CHECK(rt_irradiance_rays_host(nullptr, ids, &p, sphere, 0, 3, &o[0][0], &d[0][0], id) == -1);
        CHECK(rt_irradiance_rays_host(&b, ids, &p, sphere, 0, 3, nullptr, &d[0][0], id) == -1);
        RtIrradianceParams bad = p;
        bad.samples = 0;
        CHECK(rt_irradiance_rays_host(&b, ids, &bad, sphere, 0, 3, &o[0][0], &d[0][0], id) == -1);
        bad = p;
        bad.bias = -1.f;
        CHECK(rt_irradiance_rays_host(&b, ids, &bad, sphere, 0, 3, &o[0][0], &d[0][0], id) == -1);
    }
    g_where.clear();
}

// The rule's fold as a tree, written from its result: the last addition joins the even partials with the odd ones, the one before
// it those = 0 and = 2 (mod 4), ..., the first one partial[l] and partial[l + 32]
float tree(const float* partial, uint32_t offset, uint32_t stride) {
    if (stride == 64) return partial[offset];
    return tree(partial, offset, stride * 2) + tree(partial, offset + stride, stride * 2);
}

float folded(const std::vector<float>& terms) {
    float partial[64];
    for (float& p : partial) p = 0.f;
    for (size_t s = 0; s < terms.size(); s++) partial[s % 64] = partial[s % 64] + terms[s];
    return tree(partial, 0, 1);
}

// radiance records whose sum depends on the order: magnitudes from 1e-3 to 1e7, both signs
float term(uint32_t point, uint32_t s, int c) {
    const float mags[5] = {1e7f, 0.3f, -1e7f, 1234.567f, -1e-3f};
    return mags[(s + (uint32_t)c + point) % 5] * (1.f + (float)((s * 7u + point * 3u) % 11u) * 0.37f);
}

void gather() {
    const float PI_F = 3.14159265358979f;
    bool orderMatters = false;
    for (uint32_t S : {1u, 5u, 64u, 65u, 200u}) {
        const uint32_t n = 3;
        const uint32_t ids[3] = {11u, 0xfffffff0u, 5u};
        const RtPointNormalBatch b{nullptr, nullptr, n};
        const RtIrradianceParams p{S, 8, 0, 2, 0.f};
        std::vector<float> rad((size_t)4 * n * S);
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t s = 0; s < S; s++) {
                for (int c = 0; c < 3; c++) rad[4 * ((size_t)i * S + s) + c] = term(i, s, c);
                rad[4 * ((size_t)i * S + s) + 3] = 1.f;
            }
        // irradiance form: E = pi * fold / S
        g_where = "irradiance gather, S " + std::to_string(S);
        std::vector<float> E(4 * n, -7.f);
        CHECK(rt_irradiance_gather_host(&b, ids, &p, 0, rad.data(), E.data()) == 0);
        for (uint32_t i = 0; i < n; i++) {
            for (int c = 0; c < 3; c++) {
                std::vector<float> terms;
                float plain = 0.f;
                for (uint32_t s = 0; s < S; s++) { terms.push_back(term(i, s, c)); plain += terms.back(); }
                const float f = folded(terms);
                if (bits(f) != bits(plain)) orderMatters = true;
                CHECK(bits(E[4 * i + c]) == bits((PI_F * f) / (float)S), "%g against %g", E[4 * i + c], (PI_F * f) / (float)S);
            }
            CHECK(E[4 * i + 3] == 1.f);
        }
        // probe form: the weights are the SH of the directions rt_irradiance_rays_host gives, evaluated here from the closed forms
        g_where = "probe gather, S " + std::to_string(S);
        std::vector<float> o((size_t)3 * n * S), d((size_t)3 * n * S), c9(27 * n, -7.f);
        std::vector<uint32_t> rid((size_t)n * S);
        const float Pz[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const RtPointNormalBatch pts{Pz, nullptr, n};
        CHECK(rt_irradiance_rays_host(&pts, ids, &p, 1, 0, n, o.data(), d.data(), rid.data()) == 0);
        CHECK(rt_irradiance_gather_host(&b, ids, &p, 1, rad.data(), c9.data()) == 0);
        for (uint32_t i = 0; i < n; i++)
            for (int j = 0; j < 9; j++)
                for (int c = 0; c < 3; c++) {
                    std::vector<float> terms;
                    for (uint32_t s = 0; s < S; s++) {
                        const float* v = &d[3 * ((size_t)i * S + s)];
                        const float x = v[0], y = v[1], z = v[2];
                        const float Y[9] = {0.282095f, 0.488603f * y, 0.488603f * z, 0.488603f * x, 1.092548f * (x * y), 1.092548f * (y * z),
                                            0.315392f * (3.f * (z * z) - 1.f), 1.092548f * (x * z), 0.546274f * (x * x - y * y)};
                        terms.push_back(term(i, s, c) * Y[j]);
                    }
                    const float want = ((4.f * PI_F) * folded(terms)) / (float)S;
                    CHECK(bits(c9[27 * i + 3 * j + c]) == bits(want), "point %u c_%d[%d]: %g against %g", i, j, c, c9[27 * i + 3 * j + c], want);
                }
        // progressive: blended with what the output holds, the alpha stays 1
        g_where = "progressive gather, S " + std::to_string(S);
        RtIrradianceParams q = p;
        q.progressive = 1;
        std::vector<float> prev(4 * n);
        for (size_t k = 0; k < prev.size(); k++) prev[k] = 0.5f + (float)k;
        std::vector<float> blended = prev;
        CHECK(rt_irradiance_gather_host(&b, ids, &q, 0, rad.data(), blended.data()) == 0);
        const float w = 1.f / ((float)q.frameCount + 1.f);
        for (uint32_t i = 0; i < n; i++) {
            for (int c = 0; c < 3; c++) CHECK(bits(blended[4 * i + c]) == bits(prev[4 * i + c] * (1.f - w) + E[4 * i + c] * w));
            CHECK(blended[4 * i + 3] == 1.f);
        }
    }
    g_where.clear();
    CHECK(orderMatters, "the records' sums do not depend on the order: the check above shows nothing");
    const RtPointNormalBatch b{nullptr, nullptr, 1};
    const RtIrradianceParams bad{0, 8, 0, 0, 0.f}, ok{4, 8, 0, 0, 0.f};
    float rad[16] = {}, out[27];
    CHECK(rt_irradiance_gather_host(&b, nullptr, &bad, 0, rad, out) == -1);
    CHECK(rt_irradiance_gather_host(&b, nullptr, &ok, 0, nullptr, out) == -1);
    CHECK(rt_irradiance_gather_host(nullptr, nullptr, &ok, 0, rad, out) == -1);
}

}  // namespace

int main() {
    refusals();
    chunks();
    shape();
    rays();
    gather();
    return check_finish("irradiance queries ok");
}
