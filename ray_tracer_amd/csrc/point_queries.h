// point_queries.h — the host logic of the point queries (rt_query_nearest, rt_query_nearest_host) and the exhaustive host form
// (rt_nearest_exhaustive_host): what they refuse, in which order and with which words, the block and byte arithmetic of a batch,
// the per-object pruning records of the device traversal and the choice of its stack. Nothing in this pair
// of files needs a device: the checks do pointer arithmetic only and never dereference an array of a batch. rt_device.hip
// gathers the facts, asks here, and allocates, copies and launches; tests/point_queries_check.cpp pins every message and figure
// on the CPU, with made-up addresses. The rule itself (distances, the bound, the pruning test) is include/rt_point_query.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "rt_amd.h"
#include "scene_layout.h"

enum { RT_NEAREST_MAX_POINTS = 1 << 30 };   // as a ray batch's: one lane per point, indices and block counts stay in 32 bits
enum { RT_NEAREST_STACK = 24, RT_NEAREST_STACK_DEEP = 64 };   // entries of the two instantiations of k_nearest_points

// What a point query entry point (fn) refuses before anything is allocated or written, in check_ray_query's order and words: no
// uploaded scene; a NULL batch; points or the output NULL with n > 0; n >= 2^30. Empty: accepted (n == 0 is, whatever the pointers).
std::string check_point_query(const char* fn, bool sceneUploaded, const RtPointBatch* points, const void* out);

// A batch of n points on the device: one lane per point in work-groups of `threads`, and the bytes of its arrays (size_t
// throughout: 2^30 - 1 records of sizeof(RtNearest) bytes are past 32 bits)
struct PointShape {
    uint32_t blocks;
    size_t pointBytes;     // 12 n
    size_t limitBytes;     // 4 n
    size_t outBytes;       // sizeof(RtNearest) n
};
PointShape point_shape(uint32_t n, uint32_t threads);

// The stack k_nearest_points needs for a scene whose deepest leaf is at maxLeafDepth (MeshLayout::maxLeafDepth: the traversal
// pushes far siblings only, one per level at most): RT_NEAREST_STACK, RT_NEAREST_STACK_DEEP, or 0 with the refusal in *error
uint32_t nearest_stack(const char* fn, uint32_t maxLeafDepth, std::string* error);

// Per-object pruning record, derived in double from the object's float32 matrix:
//   sMin  the smallest singular value of the forward 3x3, reduced by the relative margin RT_NEAREST_SMIN_MARGIN: world distance
//         >= sMin x object-space distance. A matrix that is not finite gives 0 (nothing of the object is ever discarded)
//   padQ  |fl(inv q) - inverse(M) q|, Euclidean, <= padQ max(|q|_inf, 1): the entries of rt_mat4_inverse(M) against the exact
//         inverse by the count of tests/brute_force.py: inverse_error_unit (10 u E1), and 4 u |inv| for the three products and
//         three sums of a row
//   an identity object (RT_OBJ_FWD_IDENTITY) has sMin = 1 and padQ = 0 exactly
#define RT_NEAREST_SMIN_MARGIN 1e-6
struct NearestPrune { float sMin, padQ; };
NearestPrune nearest_prune(const float* transformMatrix, bool fwdIdentity);

// The table k_nearest_points reads, 3 x float4 per object: {lo.xyz, sMin} {hi.xyz, padQ} {mag, 0, 0, 0}. [lo, hi] is the world
// box an object is skipped by: objBox of an RT_OBJ_BOX object (already padded), the exact root box of an identity object, and
// (-inf, +inf) for anything else (never skipped). mag bounds |M| |[v; 1]| over the root box's corners and the world box's own
// coordinates: the scale the fp32 rounding of the object's world corners goes with (+inf where that is not finite).
std::vector<float4> layout_nearest(const ObjectLayout& l, const RenderObject* o, uint32_t n, const std::vector<RootInfo>& rootOf);

// The triangles of every object of the host arrays, for the exhaustive loops: the leaf ranges {first, count} under its root, in
// index order. false: a root, a node, a leaf range or a triangle's point index lies outside its array, or the nodes are no tree.
typedef std::vector<std::pair<uint32_t, uint32_t>> TriangleRanges;
bool object_triangle_ranges(const RtSceneArrays& s, std::vector<TriangleRanges>* rangesOf);
// rows 0..2 of the column-major matrix are the identity's: the object's corners are used as they are
bool matrix_rows_identity(const float* m);
