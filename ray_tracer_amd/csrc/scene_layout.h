// scene_layout.h — the device scene tables, built on the host: the formats the kernels read (DevScene, rt_kernels.hip.h) are
// defined here, and so are the pure functions that derive the tables from the ABI structs of rt_amd.h. Nothing in this pair of
// files needs a device: rt_device.hip uploads what they return, tests/scene_layout_check.cpp checks it on the CPU.
// A function that can refuse its input returns the message in `error` (empty: accepted).
#pragma once

#include <hip/hip_vector_types.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rt_amd.h"

// ---------------------------------------------------------------- node words
// W0 of a node (nodes[2 i].w): the index of the child pair (interior), or the leaf reference the kernels push and decode:
// LEAF | count << 28 | firstTriangle (count <= 7), or LEAF | nodeIndex for bigger leaves (first triangle in leafFirst[])
#define RT_LEAF_BIT 0x80000000u
#define RT_LEAF_CNT_SHIFT 28
#define RT_LEAF_IDX_MASK 0x0fffffffu
#define RT_HOT_PAIRS 192u          // child pairs of the meshes' top levels that come first in the device numbering; k_trace_pw<HOT> keeps the first HOT of them in LDS
#define RT_OBJTREE_LEVELS 8   // blocks of up to 256 objects in the object hierarchy (DevScene::objTree)

// ---------------------------------------------------------------- per-object words
// objMeta[i].w, and its low 16 bits again in objBox[2 i].w
#define RT_OBJ_IDENTITY 1u       // inverse(transformMatrix) is exactly the identity: the traversal may reuse the world-space ray
#define RT_OBJ_BOX 2u            // general-transform object whose padded world-space box (objBox) is valid
#define RT_OBJ_MASKABLE 4u       // the box may clear the object's bit in a ray's object mask (identity object: its exact root box)
#define RT_OBJ_FWD_IDENTITY 8u   // transformMatrix itself is exactly the identity as well (reconstruct_hit applies neither matrix)
#define RT_OBJ_SAMPLER_SHIFT 16  // bits 16..: RenderObject.samplerIndex
#define RT_OBJ_SAMPLER_MASK 0xffffu
// objAlpha[i]: the alpha map of the object's material and the object's sampler
#define RT_OBJALPHA_NONE 0xffffffffu
#define RT_OBJALPHA_SLOT_MASK 0xffu
#define RT_OBJALPHA_CLAMP 0x100u   // sampler 1: clamp to edge
// DevScene::mapFlags: the kinds of map the scene binds at all
#define RT_MAP_METALNESS 1u
#define RT_MAP_ALPHA 2u
#define RT_MAP_BUMP 4u

// device-side {index,triCount} of a mesh root, keyed by its reference node index
struct RootInfo { uint32_t idx, cnt; float lo[3], hi[3]; uint32_t triFirst, triTotal; };  // triTotal = ~0u: the mesh's triangles are not one contiguous range

// ---------------------------------------------------------------- meshes (rt_upload_scene)
//   nodes   : 2 x float4 per BVH node  {min.xyz, W0} {max.xyz, triCount}; the children of an interior node are adjacent and
//             64-byte aligned. The child pairs of the top levels of every mesh come first (breadth first over all roots, at most
//             RT_HOT_PAIRS of them: indices below hotNodes); a root that is not in such a pair sits on an odd slot
//   nodesPk : the same child pairs, interleaved for packed fp32 math: pair at even node index p -> 4 float4 at 2p:
//             {L.minx L.miny L.maxx L.maxy} {R.minx R.miny R.maxx R.maxy} {L.minz L.maxz R.minz R.maxz} {L.W0 R.W0 - -}
//   triPos  : 3 x float4 per triangle   {v0.xyz, frontOnly} {v1.xyz,-} {v2.xyz,-}, in the reference's (builder-permuted) order
//   triNrm  : 3 x float4 per triangle   vertex normals
//   triUV   : 2 x float4 per triangle   {u0 v0 u1 v1} {u2 v2 - -}
struct MeshLayout {
    std::string error;
    std::vector<float4> nodes, nodesPk, triPos, triNrm, triUV;
    std::vector<uint32_t> leafFirst;          // first triangle of a leaf, per device node
    std::vector<uint32_t> nodeRemap;          // reference node index -> device node index
    std::vector<RootInfo> rootOf;             // per reference node; idx = ~0u unless a mesh root (a distinct object.bvhIndex)
    uint32_t nodeCount = 0, hotNodes = 0, maxLeafDepth = 0;
};
MeshLayout layout_meshes(const RtSceneArrays& s);

// ---------------------------------------------------------------- objects (rt_update_objects)
//   inv, fwd : 3 x float4 per object    rows 0..2 of inverse(transformMatrix) and of transformMatrix
//   meta     : uint4 per object         {root W0, root triCount, materialIndex, RT_OBJ_* | samplerIndex << 16}
//   box      : 2 x float4 per object    {lo.xyz, RT_OBJ_* bits} {hi.xyz, root triCount}: the padded world-space box of a general-transform
//                                       object (RT_OBJ_BOX), the exact root box of an identity one under maskIdentity; else zeros
//   maskBox  : 32 x 2 float4            the RT_OBJ_MASKABLE objects of the mask window [maskBase, maskBase + 32), compact:
//                                       {lo.xyz, position in the window} {hi.xyz, -}; reachCount entries (0 unless cull)
//   skipCost : 33 x uint2               {box tests, triangle tests} the reference spends on objects [maskBase, maskBase + i) when a ray
//                                       misses them all: two box tests per interior root, the root's triangles per leaf root
//   cost     : (n + 1) x uint2          the same prefix sums over all objects
//   tree     : level k (1..treeLevels) holds at tree[2 * (treeOff[k] + (object >> k))] the union {lo.xyz, 1} {hi.xyz, -} of the boxes
//              of an aligned block of 2^k objects that all have RT_OBJ_BOX and not RT_OBJ_IDENTITY (w = 0: not such a block).
//              treeLevels = 0: fewer than objTreeMin general-transform objects, or objTreeMin = 0
struct ObjectLayout {
    std::string error;
    std::vector<float4> inv, fwd, box, maskBox, tree;
    std::vector<uint4> meta;
    std::vector<uint2> skipCost, cost;
    uint32_t treeOff[RT_OBJTREE_LEVELS + 1] = {};
    uint32_t treeLevels = 0, reachCount = 0, maskBase = 0;
    float cullOriginLimit = 0.f;   // 1e3 x the smallest size-and-position scale among the padded boxes (0: none)
    bool cull = false;             // two general-transform objects or more, or maskIdentity with an object under the mask
};
ObjectLayout layout_objects(const RenderObject* o, uint32_t n, const std::vector<RootInfo>& rootOf, uint32_t materialCount,
                            int objTreeMin, int maskIdentity);
void dump_object_tree(const ObjectLayout& l, uint32_t n);   // to stderr (RT_DEBUG_OBJTREE)

// Everything rt_upload_scene can refuse: the meshes, the scene's own checks (at least one material, the spheres' material
// indices) and the objects against the new meshes
struct SceneLayout {
    std::string error;
    MeshLayout meshes;
    ObjectLayout objects;
};
SceneLayout layout_scene(const RtSceneArrays& s, int objTreeMin, int maskIdentity);

// ---------------------------------------------------------------- materials, spheres, textures
//   mats    : 3 x float4 per material   {albedo, reflectance} {emission, strength} {ior, albedoIndex, metalnessIndex, bumpIndex (bits of the ints)}
std::vector<float4> layout_materials(const RayMaterial* m, uint32_t n);

struct SphereLayout {
    std::vector<float4> spheres;   // {center, radius}
    std::vector<uint32_t> mat;
    uint32_t testMask = 0;         // all but the spheres whose {center, radius} repeat an earlier sphere's bit for bit (DevScene::sphereTestMask)
};
SphereLayout layout_spheres(const Sphere* s, uint32_t n);

struct TextureLayout {
    std::string error;
    std::vector<uint4> info;       // per slot {first texel, width, height, -}
    std::vector<uint32_t> texels;  // all slots back to back, R8G8B8A8
};
TextureLayout layout_textures(const RtTexture* tex, uint32_t n);

// ---------------------------------------------------------------- maps and emitters (follow materials, spheres, objects and textures)
struct SceneSources {   // host copies of what the two are derived from
    std::vector<RayMaterial> mats;
    std::vector<uint32_t> sphereMat, objMat, objRoot, objSampler;
};
struct MapLayout {
    std::vector<uint32_t> objAlpha;   // per object: slot | RT_OBJALPHA_CLAMP, or RT_OBJALPHA_NONE
    uint32_t mapFlags = 0;            // RT_MAP_*: a slot < 0 or beyond the texture table binds nothing
};
MapLayout layout_maps(const SceneSources& src, uint32_t texCount);

// The emitter list of the light queries (rt_kernels.hip.h: emitter_min_t2): every triangle of every object whose material is
// emissive ({object, triangle}, sorted by object), and the emissive spheres. "Emissive" is what lightSamplePDF asks
// (raytrace.comp:392): emissionStrength != 0. mode 0: no list, every light query is traversed in full.
struct EmitterLayout {
    uint32_t mode = 0, sphereMask = 0;
    std::vector<uint2> tris;
};
EmitterLayout layout_emitters(const SceneSources& src, const std::vector<RootInfo>& rootOf, uint32_t texCount);
