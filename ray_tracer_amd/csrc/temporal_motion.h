// temporal_motion.h — what rt_temporal_accumulate needs to follow moved objects and spheres ("Temporal accumulation",
// "Moved objects and spheres"): the placement snapshot the ctx keeps beside the history, and the pure function that turns
// (snapshot of the previous call, placements now on the device) into the motion table k_tp_accumulate_motion reads. Nothing in
// this pair of files needs a device: rt_device.hip uploads what motion_table returns, tests/temporal_motion_check.cpp checks it
// on the CPU.
#pragma once

#include <hip/hip_vector_types.h>
#include <stdint.h>

#include <vector>

// ---------------------------------------------------------------- flags of a motion record
#define RT_MOTION_UNMOVED 0u    // P~ = P and n~ = n, exactly
#define RT_MOTION_MOVED 1u      // the record carries the transform back to the previous placement
#define RT_MOTION_REPLACED 2u   // another mesh, or an index one of the two calls did not have: no history
#define RT_MOTION_OBJECT_RECORDS 7u   // float4 records per object
#define RT_MOTION_SPHERE_RECORDS 2u   // float4 records per sphere

// The placements a call saw: per object rows 0..2 of transformMatrix and of its inverse exactly as layout_objects produced them
// for the device tables (ObjectLayout::fwd, ::inv), and bvhIndex; per sphere {centre, radius} as layout_spheres has it.
struct PlacementSnapshot {
    std::vector<float4> fwd, inv;      // 3 per object
    std::vector<uint32_t> bvhIndex;    // per object; its size is the object count
    std::vector<float4> spheres;       // per sphere; its size is the sphere count
};

// The motion table, for the objects and spheres of `now` (an index at or above these counts is replaced: the kernel decides
// that from the counts).
//   objects : 7 x float4 per object   {flag, -, -, -} then, when flagged moved, rows 0..2 of D = Fwd' Inv (3 x 4 affine, the
//                                     previous placement's world from this one's) and rows 0..2 of G = Inv'^T Fwd^T (3 x 3, w = 0:
//                                     the inverse transpose of D's linear part, which carries normals); zeros otherwise
//   spheres : 2 x float4 per sphere   {c, r' / r} {c', flag}: this call's centre, the previous radius over this one's, the
//                                     previous centre; zeros beside the flag unless moved
// Primes are the previous call's. D and G are multiplied in double from the fp32 rows and rounded once to fp32.
struct MotionTable {
    std::vector<float4> objects, spheres;
    uint32_t objectCount = 0, sphereCount = 0;   // of `now`
    // objects / spheres treated as moved and as replaced; an index that only one of the two calls had counts as replaced
    uint32_t movedObjects = 0, replacedObjects = 0, movedSpheres = 0, replacedSpheres = 0;
    bool any() const { return movedObjects || replacedObjects || movedSpheres || replacedSpheres; }
};
MotionTable motion_table(const PlacementSnapshot& prev, const PlacementSnapshot& now);
