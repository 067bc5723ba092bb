// temporal_motion_check.cpp — the motion table of the temporal pass on the CPU (ray_tracer_amd/csrc/temporal_motion.h), built with
// plain g++ by tests/test_temporal_motion_host.py.
//   temporal_motion_check                 : worked cases with their expected flags and counts; prints "temporal motion ok"
//   temporal_motion_check <cases> <out>   : reads snapshots pairs from <cases>, writes the table motion_table makes of each to <out>
// Case file: per case a line "nPrev nNow sPrev sNow", then per previous object 25 hex words (fwd rows, inv rows, bvhIndex), the
// same per object now, then per previous sphere 4 hex words and the same per sphere now. Output: per case a line of the six
// counts, a line of 28 hex words per object now and a line of 8 hex words per sphere now.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "temporal_motion.h"
#include "check.h"

namespace {

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// an object under scale s (per axis) and translation t: its rows and the exact inverse rows (powers of two keep them exact)
void add_object(PlacementSnapshot& p, const float s[3], const float t[3], uint32_t bvh) {
    for (int r = 0; r < 3; r++) {
        float f[4] = {0, 0, 0, t[r]}, i[4] = {0, 0, 0, -t[r] / s[r]};
        f[r] = s[r];
        i[r] = 1.f / s[r];
        p.fwd.push_back(make_float4(f[0], f[1], f[2], f[3]));
        p.inv.push_back(make_float4(i[0], i[1], i[2], i[3]));
    }
    p.bvhIndex.push_back(bvh);
}

uint32_t object_flag(const MotionTable& t, uint32_t o) { return bits(t.objects[(size_t)o * RT_MOTION_OBJECT_RECORDS].x); }
uint32_t sphere_flag(const MotionTable& t, uint32_t s) { return bits(t.spheres[(size_t)s * RT_MOTION_SPHERE_RECORDS + 1].w); }

void worked_cases() {
    const float one[3] = {1, 1, 1}, origin[3] = {0, 0, 0}, shift[3] = {0.5f, -2.f, 4.f}, squash[3] = {2.f, 0.5f, 4.f};
    PlacementSnapshot a, b;
    for (int k = 0; k < 4; k++) add_object(a, one, origin, 7u + k);
    add_object(b, one, origin, 7);      // unmoved
    add_object(b, one, shift, 8);       // translated
    add_object(b, squash, shift, 9);    // rescaled, not uniformly
    add_object(b, one, origin, 3);      // re-pointed
    a.spheres = {make_float4(0, 0, 0, 1), make_float4(1, 2, 3, 0.5f), make_float4(1, 1, 1, 2)};
    b.spheres = {make_float4(0, 0, 0, 1), make_float4(1, 2.5f, 3, 0.5f), make_float4(1, 1, 1, 0.5f)};
    MotionTable t = motion_table(a, b);
    CHECK(t.objectCount == 4 && t.sphereCount == 3);
    CHECK(t.objects.size() == 4 * RT_MOTION_OBJECT_RECORDS && t.spheres.size() == 3 * RT_MOTION_SPHERE_RECORDS);
    CHECK(object_flag(t, 0) == RT_MOTION_UNMOVED && object_flag(t, 1) == RT_MOTION_MOVED && object_flag(t, 2) == RT_MOTION_MOVED &&
          object_flag(t, 3) == RT_MOTION_REPLACED);
    CHECK(t.movedObjects == 2 && t.replacedObjects == 1 && t.movedSpheres == 2 && t.replacedSpheres == 0 && t.any());
    for (int k = 1; k < (int)RT_MOTION_OBJECT_RECORDS; k++) {   // unmoved and replaced records carry nothing but the flag
        const float4 u = t.objects[k], r = t.objects[3 * RT_MOTION_OBJECT_RECORDS + k];
        CHECK(!bits(u.x) && !bits(u.y) && !bits(u.z) && !bits(u.w) && !bits(r.x) && !bits(r.y) && !bits(r.z) && !bits(r.w));
    }
    // translated: D = Fwd' Inv = the translation back, G the identity
    const float4* r1 = &t.objects[1 * RT_MOTION_OBJECT_RECORDS];
    CHECK(r1[1].x == 1.f && r1[1].y == 0.f && r1[1].z == 0.f && r1[1].w == -0.5f && r1[2].w == 2.f && r1[3].w == -4.f);
    CHECK(r1[4].x == 1.f && r1[5].y == 1.f && r1[6].z == 1.f && r1[4].y == 0.f && r1[4].w == 0.f);
    // squashed: D's linear part is diag(1/2, 2, 1/4), G its inverse transpose diag(2, 1/2, 4)
    const float4* r2 = &t.objects[2 * RT_MOTION_OBJECT_RECORDS];
    CHECK(r2[1].x == 0.5f && r2[2].y == 2.f && r2[3].z == 0.25f && r2[1].w == -0.25f && r2[2].w == 4.f && r2[3].w == -1.f);
    CHECK(r2[4].x == 2.f && r2[5].y == 0.5f && r2[6].z == 4.f);
    CHECK(sphere_flag(t, 0) == RT_MOTION_UNMOVED && sphere_flag(t, 1) == RT_MOTION_MOVED && sphere_flag(t, 2) == RT_MOTION_MOVED);
    const float4* s1 = &t.spheres[1 * RT_MOTION_SPHERE_RECORDS];
    CHECK(s1[0].y == 2.5f && s1[0].w == 1.f && s1[1].y == 2.f);
    const float4* s2 = &t.spheres[2 * RT_MOTION_SPHERE_RECORDS];
    CHECK(s2[0].w == 4.f && s2[1].x == 1.f);
    // nothing changed: says so
    t = motion_table(a, a);
    CHECK(!t.any() && t.objectCount == 4 && object_flag(t, 3) == RT_MOTION_UNMOVED && sphere_flag(t, 2) == RT_MOTION_UNMOVED);
    // a sign of zero is a change of bits: moved, with D the identity
    PlacementSnapshot z = a;
    z.fwd[0].y = -0.f;
    t = motion_table(a, z);
    CHECK(t.movedObjects == 1 && object_flag(t, 0) == RT_MOTION_MOVED && t.objects[1].x == 1.f && t.objects[1].w == 0.f);
    // growth: the new indices are replaced; shrinkage: the table ends with the objects there are now
    PlacementSnapshot g = a;
    add_object(g, one, shift, 7);
    g.spheres.push_back(make_float4(0, 0, 0, 1));
    t = motion_table(a, g);
    CHECK(t.objectCount == 5 && object_flag(t, 4) == RT_MOTION_REPLACED && object_flag(t, 3) == RT_MOTION_UNMOVED && t.replacedObjects == 1 &&
          t.movedObjects == 0);
    CHECK(t.sphereCount == 4 && sphere_flag(t, 3) == RT_MOTION_REPLACED && t.replacedSpheres == 1 && t.movedSpheres == 0);
    t = motion_table(g, a);
    CHECK(t.objectCount == 4 && t.objects.size() == 4 * RT_MOTION_OBJECT_RECORDS && t.replacedObjects == 1 && t.replacedSpheres == 1 && t.any());
    // nothing at all: tables of one zero record each, so that there is always something to upload
    t = motion_table(PlacementSnapshot{}, PlacementSnapshot{});
    CHECK(!t.any() && t.objects.size() == RT_MOTION_OBJECT_RECORDS && t.spheres.size() == RT_MOTION_SPHERE_RECORDS);
    t = motion_table(PlacementSnapshot{}, a);
    CHECK(t.replacedObjects == 4 && t.replacedSpheres == 3 && object_flag(t, 0) == RT_MOTION_REPLACED && sphere_flag(t, 2) == RT_MOTION_REPLACED);
    // a sphere that had or gets radius 0 has no ratio
    PlacementSnapshot r0 = a;
    r0.spheres[0].w = 0.f;
    t = motion_table(a, r0);
    CHECK(sphere_flag(t, 0) == RT_MOTION_REPLACED && t.replacedSpheres == 1 && t.movedSpheres == 0);
    t = motion_table(r0, a);
    CHECK(sphere_flag(t, 0) == RT_MOTION_MOVED && t.spheres[0].w == 0.f);
}

bool read_words(FILE* f, uint32_t* w, int n) {
    for (int k = 0; k < n; k++)
        if (fscanf(f, "%x", &w[k]) != 1) return false;
    return true;
}

bool read_snapshot(FILE* f, PlacementSnapshot& p, uint32_t nObjects) {
    for (uint32_t o = 0; o < nObjects; o++) {
        uint32_t w[25];
        if (!read_words(f, w, 25)) return false;
        for (int r = 0; r < 3; r++) p.fwd.push_back(make_float4(from_bits(w[4 * r]), from_bits(w[4 * r + 1]), from_bits(w[4 * r + 2]), from_bits(w[4 * r + 3])));
        for (int r = 3; r < 6; r++) p.inv.push_back(make_float4(from_bits(w[4 * r]), from_bits(w[4 * r + 1]), from_bits(w[4 * r + 2]), from_bits(w[4 * r + 3])));
        p.bvhIndex.push_back(w[24]);
    }
    return true;
}

bool read_spheres(FILE* f, PlacementSnapshot& p, uint32_t n) {
    for (uint32_t s = 0; s < n; s++) {
        uint32_t w[4];
        if (!read_words(f, w, 4)) return false;
        p.spheres.push_back(make_float4(from_bits(w[0]), from_bits(w[1]), from_bits(w[2]), from_bits(w[3])));
    }
    return true;
}

int from_file(const char* in, const char* out) {
    FILE *f = fopen(in, "r"), *g = fopen(out, "w");
    if (!f || !g) { printf("cannot open %s or %s\n", in, out); return 2; }
    uint32_t nPrev, nNow, sPrev, sNow;
    int cases = 0;
    while (fscanf(f, "%u %u %u %u", &nPrev, &nNow, &sPrev, &sNow) == 4) {
        PlacementSnapshot a, b;
        if (!read_snapshot(f, a, nPrev) || !read_snapshot(f, b, nNow) || !read_spheres(f, a, sPrev) || !read_spheres(f, b, sNow)) {
            printf("case %d is cut short\n", cases);
            return 2;
        }
        const MotionTable t = motion_table(a, b);
        fprintf(g, "%u %u %u %u %u %u\n", t.objectCount, t.sphereCount, t.movedObjects, t.replacedObjects, t.movedSpheres, t.replacedSpheres);
        for (uint32_t o = 0; o < t.objectCount; o++) {
            for (uint32_t k = 0; k < RT_MOTION_OBJECT_RECORDS; k++) {
                const float4 r = t.objects[(size_t)o * RT_MOTION_OBJECT_RECORDS + k];
                fprintf(g, "%08x %08x %08x %08x ", bits(r.x), bits(r.y), bits(r.z), bits(r.w));
            }
            fprintf(g, "\n");
        }
        for (uint32_t s = 0; s < t.sphereCount; s++) {
            for (uint32_t k = 0; k < RT_MOTION_SPHERE_RECORDS; k++) {
                const float4 r = t.spheres[(size_t)s * RT_MOTION_SPHERE_RECORDS + k];
                fprintf(g, "%08x %08x %08x %08x ", bits(r.x), bits(r.y), bits(r.z), bits(r.w));
            }
            fprintf(g, "\n");
        }
        cases++;
    }
    fclose(f);
    fclose(g);
    printf("%d cases\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3) return from_file(argv[1], argv[2]);
    worked_cases();
    return check_finish("temporal motion ok");
}
