// mesh_topology.h — the host logic of the signed point queries (rt_upload_topology, rt_query_nearest_signed, rt_scene_topology,
// rt_nearest_side_host; DESIGN.md, "Signed point queries"): the per-triangle topology table the side rule reads
// (include/rt_point_side.h has its format), the per-object orientation, the statistics, what the entry points refuse, and the
// rule applied to given records in a plain loop. Nothing in this pair of files needs a device: rt_device.hip uploads what
// build_topology returns; tests/mesh_topology_check.cpp pins rows, statistics and messages on the CPU.
//
// How the table is made, per mesh (a distinct RenderObject.bvhIndex; two objects that place one mesh share its rows):
//  1. the points the mesh's triangles use are welded by equal position: equal float values, -0 == +0, NaN equal to nothing;
//  2. a triangle is degenerate when two of its welded corners coincide or its object-space cross product (in double) is zero. It
//     takes no part in anything below: no neighbours, no flags;
//  3. an edge is the unordered pair of welded ends. Shared by exactly two triangles, each names the other as its neighbour; one
//     triangle: a boundary edge; three or more: a non-manifold edge. Neither of the last two kinds has neighbour words;
//  4. components: triangles connected through shared edges (of any multiplicity);
//  5. a component is signable when every edge of it has exactly two triangles, a walk over its edges (from its lowest triangle,
//     breadth first) can wind neighbours consistently, and its signed volume about the object-space origin is not zero. The walk
//     gives each triangle a FLIP bit; a negative volume inverts them all, so the flip-corrected normals point outward. Cavities
//     are not modelled: an inner shell is a component of its own with outward normals of its own;
//  6. corner k's fan bit: the walk around the welded vertex, across the neighbour words, comes back to the triangle within
//     RT_SIDE_MAX_FAN triangles AND has then seen every non-degenerate triangle that touches the vertex.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rt_amd.h"
#include "scene_layout.h"

enum { RT_TOPOLOGY_MAX_TRIANGLES = 1 << 30 };   // a neighbour word is triangle << 2 | edge

struct TopologyTables {
    std::string error;                   // empty: accepted
    std::vector<uint4> rows;             // one per triangle of the scene's arrays (at least one entry)
    std::vector<int32_t> orientation;    // one per object (at least one entry)
    std::vector<RtMeshTopology> stats;   // one per object
};
// fn: the entry point the refusal names. Refuses: a triangle count of 2^30 or more; arrays that index out of range.
TopologyTables build_topology(const char* fn, const RtSceneArrays& s);

// +1, -1, or 0 for a zero or non-finite determinant of the forward 3x3 (column-major transformMatrix), in double
int32_t object_orientation(const float* transformMatrix);
std::vector<int32_t> layout_orientation(const RenderObject* o, uint32_t n);

// What ties an uploaded table to the scene it was made for
struct TopologyCounts { uint32_t objects = 0, triangles = 0, nodes = 0; };
inline bool operator==(const TopologyCounts& a, const TopologyCounts& b) { return a.objects == b.objects && a.triangles == b.triangles && a.nodes == b.nodes; }

// What a signed point query (fn) refuses before anything is allocated or written, in check_point_query's order and words, with
// two more after the scene: no uploaded scene; "no topology uploaded"; "topology does not match the uploaded scene"; a NULL
// batch; points, the output or side NULL with n > 0; n >= 2^30. Empty: accepted (n == 0 is, whatever the pointers).
std::string check_signed_query(const char* fn, bool sceneUploaded, bool topologyUploaded, const TopologyCounts& topology, const TopologyCounts& scene,
                               const RtPointBatch* points, const void* out, const void* side);
