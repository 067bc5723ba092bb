// post_passes.h — the host logic of the passes that run on finished frames (rt_render_aovs' planes, rt_denoise,
// rt_temporal_accumulate): the image plane of a camera, the parameter checks, which planes a pass reads and whether its outputs
// keep clear of them, and the state of the temporal history; and what the passes over a tile's camera rays (rt_render,
// rt_render_aovs, rt_render_guides) refuse of the tile. Nothing in this pair of files needs a device or dereferences a plane:
// rt_device.hip gathers the facts, asks here, and allocates, copies and launches; tests/post_passes_check.cpp pins every message
// and transition on the CPU, with made-up addresses.
// rt_kernels.hip.h includes this header for TemporalCamera, so device compilations read it too: keep it to declarations, plain
// structs and inline host functions, with no host-only construct at namespace scope (no static object with a constructor).
#pragma once

#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_amd.h"
#include "temporal_motion.h"

// ---------------------------------------------------------------- frame geometry
// the rows y = row0 + k*rowStride, k in [0,nRows) of a width x height image
struct RowsOf {
    uint32_t width = 0, height = 0, row0 = 0, rowStride = 0, nRows = 0;
    bool whole(uint32_t w, uint32_t h) const { return width == w && height == h && row0 == 0 && rowStride == 1 && nRows == h; }
};

// The image plane of a camera (host side of raytrace.comp:547-556; primary_dir is the device side). The one place that computes it:
// a frame's rays (frame_camera) and the temporal pass's way back through the previous camera agree bit for bit.
struct CameraPlane { float planeWidth, planeHeight, bottomLeft[3]; };
CameraPlane camera_plane(const CameraInfo& ci);

struct TemporalCamera {   // the previous call's camera, as frame_camera has it (a kernel argument of the temporal pass)
    float rot[16];
    float pos[3];
    float planeWidth, planeHeight;
    float bottomLeft[3];
};
TemporalCamera temporal_camera(const CameraInfo& ci);

// ---------------------------------------------------------------- parameter checks
struct OwnedRows;
// What rt_denoise and rt_denoise_host, rt_temporal_accumulate and rt_temporal_accumulate_host (fn) refuse before anything else:
// geometry, parameters, then a missing scene (its material table says which hits are emitters). Empty: accepted.
std::string check_denoise(uint32_t width, uint32_t height, const RtDenoiseParams& p, bool sceneUploaded, const char* fn);
std::string check_temporal(uint32_t width, uint32_t height, const CameraInfo* cam, const RtTemporalParams& p, bool sceneUploaded, const char* fn);

// What rt_build_sample_map and rt_build_sample_map_host (fn) refuse: geometry, then the parameters. momentsGiven: the caller passed
// a moments plane; else `owned` is the ctx's own of the last rt_temporal_accumulate(…, d_moments = NULL), which must be there and be
// this whole frame. Empty: accepted.
std::string check_sample_map(uint32_t width, uint32_t height, const RtSampleMapParams& p, bool momentsGiven, const OwnedRows& owned, const char* fn);
// what rt_render_sampled refuses beyond rt_render's checks: a map with the debug heat maps, which count work per pixel
std::string check_sampled(const RayTracerData& td, bool mapGiven);

// ---------------------------------------------------------------- the passes over a tile's camera rays
// What rt_render, rt_render_aovs and rt_render_guides (fn) refuse of a tile and its scene counts: the rows y = row0 + k*rowStride,
// k in [0,nRows) must lie in the width x height image, a scene must be uploaded and rayTraceParams must not count more spheres or
// objects than it holds. Empty: accepted.
struct UploadedScene { bool uploaded; uint32_t sphereCount, objectCount; };
std::string check_tile(const char* fn, const RayTracerData& td, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride, uint32_t nRows,
                       const UploadedScene& scene);
// a tile's pixels must fit the 30 bits of a slot id (rt_render_aovs, rt_render_guides)
std::string check_tile_slots(const char* fn, uint32_t width, uint32_t nRows);
// What rt_render_guides refuses before anything is allocated: maxBounces beyond RT_GUIDE_MAX_BOUNCES, then check_tile and
// check_tile_slots, then a plane of d_guides that shares a byte with a plane of d_firstHit (either may be NULL, and so may any
// field: such planes are not written).
enum { RT_GUIDE_MAX_BOUNCES = 8 };
std::string check_guides(const RayTracerData& td, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride, uint32_t nRows,
                         uint32_t maxBounces, const RtAovBuffers* guides, const RtAovBuffers* firstHit, const UploadedScene& scene);

// ---------------------------------------------------------------- the planes a pass reads
// The ctx-owned AOV planes are one buffer of AOV_PLANES planes of nPixels 16-byte records, in this order (rt_render_aovs writes
// them, rt_read_aovs and the passes find them by it).
enum AovPlane { AOV_NORMAL_DEPTH, AOV_POSITION, AOV_ALBEDO, AOV_RAY_DIR, AOV_IDS, AOV_PLANES };
inline void* aov_plane(const void* base, AovPlane k, size_t nPixels) { return (char*)base + (size_t)k * nPixels * sizeof(float4); }
inline void* aov_plane(const RtAovBuffers& b, AovPlane k) {   // the same plane of a caller's set
    void* const planes[AOV_PLANES] = {b.normalDepth, b.position, b.albedo, b.rayDir, b.ids};
    return planes[k];
}

// what a read or a pass says of a plane the ctx was never asked to keep
inline const char* const NO_OWNED_FRAMEBUFFER = "no ctx-owned framebuffer: rt_render was never called with d_rgba = NULL";
inline const char* const NO_OWNED_AOVS = "no ctx-owned AOV planes: rt_render_aovs was never called with d_out = NULL";
inline const char* const NO_OWNED_GUIDES = "no ctx-owned guide planes: rt_render_guides was never called with d_guides = NULL";
inline const char* const NO_OWNED_MOMENTS = "no ctx-owned moments: rt_temporal_accumulate was never called with d_moments = NULL";

// What the ctx owns of a kind (its framebuffer; its AOV planes): where, whether a pass ever wrote it, and the rows it holds
struct OwnedRows { const void* base; bool valid; RowsOf rows; };
// The inputs of a pass over a whole width x height frame: the caller's planes as they are, or, where the caller passes NULL, the
// ctx's own, which must hold the whole frame. position only where the pass reads it (NULL otherwise). error: the refusal.
struct PassInputs {
    const float4 *rgba = nullptr, *normalDepth = nullptr, *position = nullptr, *albedo = nullptr;
    const uint4* ids = nullptr;
    std::string error;
};
PassInputs resolve_inputs(const char* fn, uint32_t width, uint32_t height, const float* rgba, const RtAovBuffers* aovs, bool needPosition,
                          const OwnedRows& fb, const OwnedRows& aov);

// ---------------------------------------------------------------- overlap
bool overlap(const void* a, const void* b, size_t bytes);   // two planes of `bytes` bytes share a byte
// The outputs of a pass (a NULL one is the ctx's own plane and skipped) against its inputs, then against each other. Empty: disjoint.
// Else "<fn>: <anOutput> overlaps an input" (the caller's phrase for any of its outputs) or "<fn>: <name> overlaps <name>".
struct NamedPlane { const char* name; const void* p; };
std::string check_overlap(const char* fn, const PassInputs& in, const char* anOutput, const NamedPlane* outs, int nOuts, size_t bytes);

// ---------------------------------------------------------------- the temporal history
// The two histories a call reads and writes in turn, seen from the host: which one the last accepted call wrote, at what size and
// through which camera; with tracking on, the placements that call saw (the snapshot) beside the ones now on the device. The rules,
// which hold because nothing else writes these fields: a refused call changes nothing (it reaches neither begin nor commit); a
// history of another size is none; with tracking on, a history without a snapshot is none; the snapshot goes with the history.
class TemporalHistory {
public:
    struct Step {
        int read, write;       // the history this call reads (-1: none) and the one it writes
        MotionTable motion;    // what moved since the call that wrote `read`; any() says the motion kernel is needed
    };
    void reset();                   // rt_temporal_reset, and a new scene: nothing of the old frames is history
    void set_tracking(bool on);     // rt_temporal_track_motion: the same value changes nothing, another one resets
    // the placements behind the tables now on the device: rows 0..2 of every object's matrix and of its inverse, and its bvhIndex
    // (set_objects); every sphere's {centre, radius} (set_spheres)
    void set_object_placements(const float4* fwd, const float4* inv, const uint32_t* bvhIndex, uint32_t n);
    void set_sphere_placements(const float4* spheres, uint32_t n);
    // rt_update_points refit these meshes (bvhIndex values): in the snapshot the objects that show them get a bvhIndex no mesh has,
    // so the next begin finds "another mesh" there (RT_MOTION_REPLACED: no history); the commit after it takes the true ones again
    void meshes_refit(const uint32_t* bvhIndex, uint32_t n);
    // An accepted call, once its buffers exist. historyBuffersFit: neither history buffer had to be (re)allocated for this size.
    // Drops a history of another size or of a replaced buffer, then records the size: a begin without a commit (a failed upload
    // or launch) leaves the old history valid only where it has this very size, and it was not written to.
    Step begin(uint32_t width, uint32_t height, bool historyBuffersFit);
    // Its launch was accepted: what it wrote is the history, `cam` its camera, and with tracking on the placements its snapshot
    void commit(const CameraInfo& cam);

    const TemporalCamera& camera() const { return cam; }     // of the call that wrote the history
    const uint32_t* moved_counts() const { return moved; }   // the last begin's: moved objects, replaced objects, moved or new spheres

private:
    int cur = 0;
    bool histValid = false, snapValid = false, track = false;
    uint32_t width = 0, height = 0;
    TemporalCamera cam{};
    PlacementSnapshot snap, now;
    uint32_t moved[3] = {0, 0, 0};
};
