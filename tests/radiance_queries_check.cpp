// radiance_queries_check.cpp — what the radiance queries refuse (ray_tracer_amd/csrc/radiance_queries.h: check_radiance_query), in
// their order and with their messages, the pieces of a batch (radiance_piece_count, radiance_piece), the bytes of its arrays
// (radiance_shape; where they lie in the staging buffer of the _host form: tests/host_staging_check.cpp) and the frame's seed (radiance_starting_seed), on the CPU, built with plain g++ by
// tests/test_radiance_queries_host.py. No array is ever dereferenced by the checks: the addresses are made up. Prints
// "seed <frameCount> <startingSeed>" for the frames the Python side compares with the oracle's random(), then "radiance queries ok".
#include <cstdio>
#include <string>

#include "radiance_queries.h"
#include "check.h"

namespace {

template <typename T> T* at(uintptr_t a) { return (T*)a; }

const char* const FNS[2] = {"rt_query_radiance", "rt_query_radiance_host"};

void refusals() {
    float* const O = at<float>(0x10000000u);
    float* const D = at<float>(0x20000000u);
    float* const T = at<float>(0x30000000u);
    void* const OUT = at<void>(0x40000000u);
    const RtRadianceParams ok{4, 8, 0, 0};
    for (const char* fn : FNS) {
        const std::string f(fn);
        const RtRayBatch rays{O, D, nullptr, 1000};
        CHECK(check_radiance_query(fn, true, &rays, &ok, OUT).empty());
        const RtRadianceParams edge{0xffffffffu, (1u << 28) - 2u, 1, 0xffffffffu};
        CHECK(check_radiance_query(fn, true, &rays, &edge, OUT).empty());
        const RtRayBatch most{O, D, nullptr, (1u << 30) - 1u};
        CHECK(check_radiance_query(fn, true, &most, &ok, OUT).empty());
        // every refusal
        CHECK(check_radiance_query(fn, false, &rays, &ok, OUT) == f + " before rt_upload_scene");
        CHECK(check_radiance_query(fn, true, nullptr, &ok, OUT) == f + ": the batch and the params are required");
        CHECK(check_radiance_query(fn, true, &rays, nullptr, OUT) == f + ": the batch and the params are required");
        const RtRayBatch noO{nullptr, D, nullptr, 5}, noD{O, nullptr, nullptr, 5};
        CHECK(check_radiance_query(fn, true, &noO, &ok, OUT) == f + ": origins, dirs and the output are required");
        CHECK(check_radiance_query(fn, true, &noD, &ok, OUT) == f + ": origins, dirs and the output are required");
        CHECK(check_radiance_query(fn, true, &rays, &ok, nullptr) == f + ": origins, dirs and the output are required");
        const RtRayBatch limited{O, D, T, 1000};
        CHECK(check_radiance_query(fn, true, &limited, &ok, OUT) == f + ": tmax must be NULL (a path has no reach limit)");
        const RtRadianceParams noSamples{0, 8, 0, 0};
        CHECK(check_radiance_query(fn, true, &rays, &noSamples, OUT) == f + ": samples must be >= 1");
        const RtRadianceParams deep{4, (1u << 28) - 1u, 0, 0}, deepest{4, 0xffffffffu, 0, 0};
        CHECK(check_radiance_query(fn, true, &rays, &deep, OUT) == f + ": bounceLimit needs more than 28 bits");
        CHECK(check_radiance_query(fn, true, &rays, &deepest, OUT) == f + ": bounceLimit needs more than 28 bits");
        const RtRayBatch big{O, D, nullptr, 1u << 30}, huge{O, D, nullptr, 0xffffffffu};
        CHECK(check_radiance_query(fn, true, &big, &ok, OUT) == f + ": a batch of 1073741824 rays does not fit the 30 bits of a slot id");
        CHECK(check_radiance_query(fn, true, &huge, &ok, OUT) == f + ": a batch of 4294967295 rays does not fit the 30 bits of a slot id");
        // n == 0 succeeds whatever the arrays and the params hold, but not without a scene, a batch or params
        const RtRayBatch none{nullptr, nullptr, T, 0};
        CHECK(check_radiance_query(fn, true, &none, &noSamples, nullptr).empty());
        CHECK(check_radiance_query(fn, false, &none, &ok, nullptr) == f + " before rt_upload_scene");
        CHECK(check_radiance_query(fn, true, &none, nullptr, nullptr) == f + ": the batch and the params are required");
        // the order: each refusal with everything after it wrong as well
        const RtRadianceParams bad{0, 0xffffffffu, 0, 0}, badDeep{4, 0xffffffffu, 0, 0};
        const RtRayBatch w3{nullptr, D, T, 1u << 30}, w4{O, D, T, 1u << 30}, w5{O, D, nullptr, 1u << 30};
        CHECK(check_radiance_query(fn, false, nullptr, nullptr, nullptr) == f + " before rt_upload_scene");
        CHECK(check_radiance_query(fn, false, &w3, &bad, nullptr) == f + " before rt_upload_scene");
        CHECK(check_radiance_query(fn, true, nullptr, &bad, nullptr) == f + ": the batch and the params are required");
        CHECK(check_radiance_query(fn, true, &w3, nullptr, nullptr) == f + ": the batch and the params are required");
        CHECK(check_radiance_query(fn, true, &w3, &bad, OUT) == f + ": origins, dirs and the output are required");
        CHECK(check_radiance_query(fn, true, &w4, &bad, nullptr) == f + ": origins, dirs and the output are required");
        CHECK(check_radiance_query(fn, true, &w4, &bad, OUT) == f + ": tmax must be NULL (a path has no reach limit)");
        CHECK(check_radiance_query(fn, true, &w5, &bad, OUT) == f + ": samples must be >= 1");
        CHECK(check_radiance_query(fn, true, &w5, &badDeep, OUT) == f + ": bounceLimit needs more than 28 bits");
        CHECK(check_radiance_query(fn, true, &w5, &ok, OUT) == f + ": a batch of 1073741824 rays does not fit the 30 bits of a slot id");
    }
    RtRadianceParams d{9, 9, 9, 9};
    rt_radiance_params_default(&d);
    CHECK(d.samples == 1 && d.bounceLimit == 8 && d.progressive == 0 && d.frameCount == 0);
    rt_radiance_params_default(nullptr);
}

// the pieces cover [0, n) in order, without gap or overlap, none empty, none above the cap
void cover(uint32_t n, uint64_t maxSlots, uint32_t expectPieces) {
    const uint32_t cap = radiance_piece_cap(maxSlots), pieces = radiance_piece_count(n, maxSlots);
    CHECK(pieces == expectPieces);
    uint64_t at = 0;
    for (uint32_t k = 0; k < pieces; k++) {
        const RadiancePiece p = radiance_piece(n, maxSlots, k);
        CHECK(p.first == at && p.n >= 1 && p.n <= cap);
        CHECK(k + 1 == pieces || p.n == cap);   // only the last one is short
        at += p.n;
    }
    CHECK(at == n);
    const RadiancePiece past = radiance_piece(n, maxSlots, pieces);
    CHECK(past.first == n && past.n == 0);
}

void pieces() {
    const uint64_t K = 1024;   // "radiance_max_kslots" 1
    CHECK(radiance_piece_cap(K) == 1024);
    cover(0, K, 0); cover(1, K, 1); cover(1023, K, 1); cover(1024, K, 1); cover(1025, K, 2); cover(3 * 1024 + 5, K, 4);
    const RadiancePiece last = radiance_piece(3 * 1024 + 5, K, 3);
    CHECK(last.first == 3072 && last.n == 5);
    // the default (24 M paths), a cap of more than the slot ids, a cap of nothing, the largest batch
    cover(2073600, 24ull << 20, 1); cover((1u << 30) - 1u, 24ull << 20, 43);
    CHECK(radiance_piece_cap(1ull << 40) == (1u << 30) - 1u && radiance_piece_cap(0) == 1);
    cover((1u << 30) - 1u, 1ull << 40, 1); cover(3, 0, 3);
    cover((1u << 30) - 1u, (1ull << 20) << 10, 1);   // the knob's largest value
}

void shape() {
    for (uint32_t n : {1u, 63u, 64u, 65u, 2299u, (1u << 30) - 1u})
        for (int ids = 0; ids < 2; ids++) {
            const RadianceShape g = radiance_shape(n, ids != 0);
            CHECK(g.vecBytes == (size_t)12 * n && g.idBytes == (ids ? (size_t)4 * n : 0) && g.outBytes == (size_t)16 * n);
        }
    const RadianceShape top = radiance_shape((1u << 30) - 1u, true);
    CHECK(top.outBytes == 17179869168ull);   // past 32 bits: size_t arithmetic
}

}  // namespace

int main() {
    refusals();
    pieces();
    shape();
    for (uint32_t frame : {0u, 3u, 0xffffffffu}) printf("seed %u %u\n", frame, radiance_starting_seed(frame));
    return check_finish("radiance queries ok");
}
