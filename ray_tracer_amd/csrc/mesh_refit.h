// mesh_refit.h — deforming meshes in place (rt_update_points, rt_scene_update_points; DESIGN.md, "Deforming meshes"): new points
// under the kept topology, and every BVH box refit bottom-up. Nothing in this pair of files needs a device: rt_device.hip uploads
// the plan and runs it with the kernels of rt_refit.hip.h, scene.cpp runs refit_nodes_host on the host scene's own arrays,
// tests/mesh_refit_check.cpp checks both on the CPU.
//
// The refit rule, stated once (host, device and the test's numpy restate it):
//   leaf     : start from the builder's sentinels lo = +1e30, hi = -1e30 and grow by the leaf's triangles in order, corners v0, v1,
//              v2, with the builder's comparisons  lo = p < lo ? p : lo;  hi = hi < p ? p : hi   (scene.cpp: Box::grow_point)
//   interior : the left child's box, then grown by the right child's with the same comparisons (Box::grow_box)
// No fminf / fmaxf: of two zeros of different sign the comparisons keep the first, everywhere the same one, so the tables a refit
// leaves on the device equal, byte for byte, the tables a fresh upload of the refit host scene makes.
// The builder gives every node the exact min / max of its triangles' vertices, so the rule reproduces the builder's boxes for the
// builder's topology (by value: the builder itself is only fixed up to the sign of a zero bound).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "scene_layout.h"

#define RT_REFIT_LO 1e30f
#define RT_REFIT_HI -1e30f

// One mesh: a distinct object.bvhIndex. The reference half (root .. triCount) is what the host refit needs, the device half
// indexes RefitPlan's lists. Hot pairs interleave the meshes' top levels at the front of the device numbering, so a mesh's
// nodes are index lists, not ranges.
struct RefitMesh {
    uint32_t root = 0;                        // reference node index
    uint32_t pointFirst = 0, pointEnd = 0;    // its triangles use point indices of [pointFirst, pointEnd) only
    uint32_t triFirst = 0, triCount = 0;      // its triangles: one contiguous range
    uint32_t rootDev = 0;                     // device index of the root
    uint32_t leafOff = 0, inlineLeaves = 0, bigLeaves = 0;   // RefitPlan::leaves[leafOff, ...): the leaves whose W0 holds {count <= 7, first}, then the others
    uint32_t interiorOff = 0, interiorCount = 0;             // RefitPlan::interior[interiorOff, ...): deepest level first
    uint32_t levelOff = 0, levelCount = 0;    // RefitPlan::levels[levelOff, levelOff + levelCount]: where each level starts in the mesh's
                                              // interior list (relative to interiorOff), and the list's end; the last level is the root's
};

struct RefitPlan {
    std::string error;
    std::vector<RefitMesh> meshes;            // sorted by root
    std::vector<uint32_t> leaves, interior;   // device node indices
    std::vector<uint32_t> levels;
    uint32_t pointCount = 0;
};

// The meshes of a scene with the reference half filled in. Refuses (error) a mesh that shares nodes with another mesh or with
// itself, and one whose triangles are not one contiguous range: neither can be refit on its own.
std::vector<RefitMesh> refit_meshes(const RtSceneArrays& s, std::string& error);
// ... and the device half from the numbering of layout_meshes (`l` is the layout of `s`)
RefitPlan plan_refit(const RtSceneArrays& s, const MeshLayout& l);

// What rt_update_points and rt_scene_update_points refuse in their arguments ("" : accepted). `fn` starts the message.
std::string check_update_points(const char* fn, uint32_t pointCount, const TrianglePoint* points, uint32_t first, uint32_t count);
// The meshes (indices into `meshes`) that use a point of [first, first + count): an intersection of ranges, which may name a mesh
// whose triangles use none of the replaced points
std::vector<uint32_t> touched_meshes(const std::vector<RefitMesh>& meshes, uint32_t first, uint32_t count);

// The rule on the reference's own nodes: refits the subtree of `root` in place from triangles and points; index and triCount stay.
void refit_nodes_host(BVHNode* nodes, const Triangle* triangles, const TrianglePoint* points, uint32_t root);
