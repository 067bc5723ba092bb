// post_passes.cpp — the host logic of the AOV, denoising and temporal passes (post_passes.h). Host only.

#include "post_passes.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "rt_det_math.h"

// ---------------------------------------------------------------- frame geometry
CameraPlane camera_plane(const CameraInfo& ci) {
    CameraPlane p;
    p.planeHeight = ci.nearPlane * rt_tan(rt_radians(ci.fov * 0.5f)) * 2.f;
    p.planeWidth = p.planeHeight * ci.aspectRatio;
    p.bottomLeft[0] = -p.planeWidth / 2.f;
    p.bottomLeft[1] = -p.planeHeight / 2.f;
    p.bottomLeft[2] = 0.1f;
    return p;
}

TemporalCamera temporal_camera(const CameraInfo& ci) {
    TemporalCamera t{};
    const CameraPlane p = camera_plane(ci);
    memcpy(t.rot, ci.cameraRotation, 64);
    memcpy(t.pos, ci.pos, 12);
    t.planeWidth = p.planeWidth;
    t.planeHeight = p.planeHeight;
    memcpy(t.bottomLeft, p.bottomLeft, 12);
    return t;
}

namespace {
const char* bad_frame(uint32_t width, uint32_t height) {   // what is wrong with a frame's geometry, or NULL
    if (width == 0 || height == 0) return ": bad image geometry";
    if ((uint64_t)width * height >= (1ull << 30) || height > 65535u * 16u) return ": image too large";
    return nullptr;
}

// what the ctx owns of a kind, as a pass over the whole width x height frame may read it
std::string check_owned(const char* fn, const char* what, const char* never, const OwnedRows& o, uint32_t width, uint32_t height) {
    if (!o.valid) return std::string(fn) + ": " + never;
    if (o.rows.whole(width, height)) return "";
    char m[256];
    snprintf(m, sizeof(m), "%s: %s: rows %u + k*%u, k < %u of a %u x %u image, not the whole %u x %u frame", fn, what, o.rows.row0,
             o.rows.rowStride, o.rows.nRows, o.rows.width, o.rows.height, width, height);
    return m;
}
}  // namespace

// ---------------------------------------------------------------- parameter checks
std::string check_denoise(uint32_t width, uint32_t height, const RtDenoiseParams& p, bool sceneUploaded, const char* fn) {
    const std::string f(fn);
    if (const char* m = bad_frame(width, height)) return f + m;
    if (p.iterations > 10) return f + ": iterations must be 0..10";
    if (!(std::isfinite(p.sigmaLuminance) && p.sigmaLuminance > 0.f)) return f + ": sigmaLuminance must be finite and > 0";
    if (!(std::isfinite(p.sigmaNormal) && p.sigmaNormal >= 0.f)) return f + ": sigmaNormal must be finite and >= 0";
    if (!(std::isfinite(p.sigmaDepth) && p.sigmaDepth > 0.f)) return f + ": sigmaDepth must be finite and > 0";
    if (!sceneUploaded) return f + " before rt_upload_scene";
    return "";
}

std::string check_temporal(uint32_t width, uint32_t height, const CameraInfo* cam, const RtTemporalParams& p, bool sceneUploaded, const char* fn) {
    const std::string f(fn);
    if (const char* m = bad_frame(width, height)) return f + m;
    if (!cam) return f + ": the camera the frame was rendered with is required";
    if (p.maxHistory == 0) return f + ": maxHistory must be >= 1";
    if (!(p.normalCos >= -1.f && p.normalCos <= 1.f)) return f + ": normalCos must be in [-1, 1]";
    if (!(std::isfinite(p.depthTolerance) && p.depthTolerance > 0.f)) return f + ": depthTolerance must be finite and > 0";
    if (!sceneUploaded) return f + " before rt_upload_scene";
    return "";
}

std::string check_sample_map(uint32_t width, uint32_t height, const RtSampleMapParams& p, bool momentsGiven, const OwnedRows& owned, const char* fn) {
    const std::string f(fn);
    if (const char* m = bad_frame(width, height)) return f + m;
    if (p.minSamples > p.baseSamples) return f + ": minSamples must be <= baseSamples";
    if (p.baseSamples > p.maxSamples) return f + ": baseSamples must be <= maxSamples";
    if (!(std::isfinite(p.targetRelError) && p.targetRelError > 0.f)) return f + ": targetRelError must be finite and > 0";
    if (!(std::isfinite(p.luminanceFloor) && p.luminanceFloor > 0.f)) return f + ": luminanceFloor must be finite and > 0";
    if (!momentsGiven) return check_owned(fn, "the ctx moments", NO_OWNED_MOMENTS, owned, width, height);
    return "";
}

std::string check_sampled(const RayTracerData& td, bool mapGiven) {
    if (mapGiven && td.debug >= 0) return "rt_render_sampled: the debug heat maps take no sample map";
    return "";
}

// ---------------------------------------------------------------- the passes over a tile's camera rays
std::string check_tile(const char* fn, const RayTracerData& td, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride, uint32_t nRows,
                       const UploadedScene& scene) {
    const std::string f(fn);
    if (width == 0 || height == 0 || rowStride == 0) return f + ": bad image geometry";
    if (nRows && (uint64_t)row0 + (uint64_t)(nRows - 1) * rowStride >= height) return f + ": rows exceed the image";
    if (!scene.uploaded) return f + " before rt_upload_scene";
    if (td.sphereCount > scene.sphereCount) return "rayTraceParams.sphereCount exceeds the uploaded spheres";
    if (td.objectCount > scene.objectCount) return "rayTraceParams.objectCount exceeds the uploaded objects";
    return "";
}

std::string check_tile_slots(const char* fn, uint32_t width, uint32_t nRows) {
    if ((uint64_t)nRows * width >= (1ull << 30)) return std::string(fn) + ": tile too large (slot ids are 30 bits)";
    return "";
}

std::string check_guides(const RayTracerData& td, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride, uint32_t nRows,
                         uint32_t maxBounces, const RtAovBuffers* guides, const RtAovBuffers* firstHit, const UploadedScene& scene) {
    const char* const fn = "rt_render_guides";
    if (maxBounces > RT_GUIDE_MAX_BOUNCES) return std::string(fn) + ": maxBounces must be 0..8";
    std::string e = check_tile(fn, td, width, height, row0, rowStride, nRows, scene);
    if (e.empty()) e = check_tile_slots(fn, width, nRows);
    if (!e.empty() || !guides || !firstHit) return e;
    static const char* const names[AOV_PLANES] = {"normalDepth", "position", "albedo", "rayDir", "ids"};
    const size_t bytes = (size_t)nRows * width * sizeof(float4);
    for (int g = 0; g < AOV_PLANES; g++)
        for (int h = 0; h < AOV_PLANES; h++) {
            const void *a = aov_plane(*guides, (AovPlane)g), *b = aov_plane(*firstHit, (AovPlane)h);
            if (a && b && overlap(a, b, bytes)) return std::string(fn) + ": d_guides." + names[g] + " overlaps d_firstHit." + names[h];
        }
    return "";
}

// ---------------------------------------------------------------- the planes a pass reads
PassInputs resolve_inputs(const char* fn, uint32_t width, uint32_t height, const float* rgba, const RtAovBuffers* aovs, bool needPosition,
                          const OwnedRows& fb, const OwnedRows& aov) {
    PassInputs in;
    const size_t n = (size_t)width * height;
    in.rgba = (const float4*)rgba;
    if (!rgba) {
        if (!(in.error = check_owned(fn, "the ctx framebuffer", NO_OWNED_FRAMEBUFFER, fb, width, height)).empty()) return in;
        in.rgba = (const float4*)fb.base;
    }
    const auto plane = [&](AovPlane k) { return aovs ? aov_plane(*aovs, k) : aov_plane(aov.base, k, n); };
    if (!aovs) {
        if (!(in.error = check_owned(fn, "the ctx AOV planes", NO_OWNED_AOVS, aov, width, height)).empty()) return in;
    } else if (!aovs->normalDepth || (needPosition && !aovs->position) || !aovs->albedo || !aovs->ids) {
        in.error = std::string(fn) + ": d_aovs needs the normalDepth, " + (needPosition ? "position, " : "") + "albedo and ids planes";
        return in;
    }
    in.normalDepth = (const float4*)plane(AOV_NORMAL_DEPTH);
    if (needPosition) in.position = (const float4*)plane(AOV_POSITION);
    in.albedo = (const float4*)plane(AOV_ALBEDO);
    in.ids = (const uint4*)plane(AOV_IDS);
    return in;
}

// ---------------------------------------------------------------- overlap
bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

std::string check_overlap(const char* fn, const PassInputs& in, const char* anOutput, const NamedPlane* outs, int nOuts, size_t bytes) {
    for (int o = 0; o < nOuts; o++) {
        if (!outs[o].p) continue;
        for (const void* i : {(const void*)in.rgba, (const void*)in.normalDepth, (const void*)in.position, (const void*)in.albedo, (const void*)in.ids})
            if (i && overlap(outs[o].p, i, bytes)) return std::string(fn) + ": " + anOutput + " overlaps an input";
    }
    for (int a = 0; a < nOuts; a++)
        for (int b = a + 1; b < nOuts; b++)
            if (outs[a].p && outs[b].p && overlap(outs[a].p, outs[b].p, bytes)) return std::string(fn) + ": " + outs[a].name + " overlaps " + outs[b].name;
    return "";
}

// ---------------------------------------------------------------- the temporal history
void TemporalHistory::reset() {
    histValid = false;   // host state only: the next call reads no history, and the ctx stream orders it after the last one
    snapValid = false;
}

void TemporalHistory::set_tracking(bool on) {
    if (track == on) return;
    track = on;
    reset();   // the history of the other mode has no snapshot to go with it, or one nobody kept up
}

void TemporalHistory::set_object_placements(const float4* fwd, const float4* inv, const uint32_t* bvhIndex, uint32_t n) {
    now.fwd.assign(fwd, fwd + 3 * (size_t)n);
    now.inv.assign(inv, inv + 3 * (size_t)n);
    now.bvhIndex.assign(bvhIndex, bvhIndex + n);
}

void TemporalHistory::set_sphere_placements(const float4* spheres, uint32_t n) { now.spheres.assign(spheres, spheres + n); }

void TemporalHistory::meshes_refit(const uint32_t* bvhIndex, uint32_t n) {
    for (uint32_t& b : snap.bvhIndex)
        for (uint32_t k = 0; k < n; k++)
            if (b == bvhIndex[k]) b = 0xffffffffu;
}

TemporalHistory::Step TemporalHistory::begin(uint32_t w, uint32_t h, bool historyBuffersFit) {
    if (width != w || height != h || !historyBuffersFit) reset();   // a history of another size is none, nor is one whose buffer was replaced
    width = w; height = h;   // (here and not in commit: after the reset above, the history still valid at this point has this size)
    Step s{histValid ? cur : -1, 1 - cur, {}};
    // what moved since the call that wrote the history: only then the motion kernel, else the launch of a call without tracking
    if (track && histValid && snapValid) s.motion = motion_table(snap, now);
    moved[0] = s.motion.movedObjects; moved[1] = s.motion.replacedObjects; moved[2] = s.motion.movedSpheres + s.motion.replacedSpheres;
    return s;
}

void TemporalHistory::commit(const CameraInfo& c) {
    if (track) { snap = now; snapValid = true; }
    cur = 1 - cur;
    histValid = true;
    cam = temporal_camera(c);
}
