/*
 * rt_amd.h — C ABI of the MI355X path tracer (librt_amd.so).
 *
 * Two halves:
 *
 *  (1) Scene surface (host only, no GPU touched). Keeps the reference's scene
 *      surface: the AoS structs of src/vk_engine.h:49-79,117-123,145-189 with
 *      the same field names and std140 / push-constant layouts,
 *      and the scene builders of src/vk_engine.cpp (read_obj :800-1037,
 *      read_mtl :1060-1167, cornell_box :638-678, prepare_storage_buffers
 *      :680-758, build_bvh :1169-1337, camera matrix of run_compute
 *      :1631-1661).
 *
 *  (2) Device half. Replaces the Vulkan seam of the reference:
 *        copy_buffer   (src/vk_engine.cpp:1401-1444)  -> rt_upload_scene
 *        update_buffer (src/vk_engine.cpp:1446-1475)  -> rt_update_*
 *        run_compute   (src/vk_engine.cpp:1623-1676)  -> rt_render
 *      The per-pixel megakernel shaders/raytrace.comp is replaced by a
 *      wavefront pipeline of HIP kernels for gfx950.
 *
 * All entry points are extern "C", take plain pointers and sizes, return an
 * int status (0 = ok, <0 = error; message via rt_last_error) and never abort
 * (the reference's VK_CHECK aborts, src/vk_engine.cpp:20-27).
 * A ctx is bound to one GPU and is not thread-safe; one process per GPU.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Scene structs — byte-compatible with the reference's host structs   */
/* ------------------------------------------------------------------ */

/* src/vk_engine.h:49-53 (std140, 32 B) */
typedef struct Sphere {
    float position[3];
    float radius;            /* @12 */
    uint32_t materialIndex;  /* @16 */
    uint32_t _pad[3];
} Sphere;

/* src/vk_engine.h:55-62 (48 B). binormal/tangent are never initialised by
 * the reference (calculate_binormal assigns nothing) and never read. */
typedef struct Triangle {
    uint32_t v0, v1, v2;
    uint32_t frontOnly;
    float binormal[3]; float _pad0; /* @16 */
    float tangent[3];  float _pad1; /* @32 */
} Triangle;

/* src/vk_engine.h:64-67 (32 B): uv.x is position.w, uv.y is normal.w */
typedef struct TrianglePoint {
    float position[4];
    float normal[4];
} TrianglePoint;

/* src/vk_engine.h:69-79 (64 B) */
typedef struct RayMaterial {
    float albedo[3]; float _pad0;  /* @0  default (1,1,1) */
    float emissionColor[3];        /* @16 default (0,0,0) */
    float emissionStrength;        /* @28 */
    float reflectance;             /* @32 */
    float ior;                     /* @36 default -1 */
    int32_t albedoIndex;           /* @40 default -1 */
    int32_t metalnessIndex;        /* @44 */
    int32_t alphaIndex;            /* @48 */
    int32_t bumpIndex;             /* @52 */
    uint32_t _pad1[2];
} RayMaterial;

/* src/vk_engine.h:117-123 (80 B); transformMatrix is column-major */
typedef struct RenderObject {
    float transformMatrix[16];
    uint32_t smoothShade;    /* @64 */
    uint32_t bvhIndex;       /* @68 */
    uint32_t materialIndex;  /* @72 */
    uint32_t samplerIndex;   /* @76 */
} RenderObject;

/* src/vk_engine.h:185-189 (32 B). triCount == 0: interior, index = left
 * child, right child = index + 1; else leaf, index = first triangle. */
typedef struct BVHNode {
    float boundsX[2], boundsY[2], boundsZ[2]; /* (min,max) per axis */
    uint32_t index, triCount;
} BVHNode;

/* src/vk_engine.h:145-151 (96 B) */
typedef struct CameraInfo {
    float cameraRotation[16];
    float pos[3];            /* @64 default (0,-0.5,-3.5) */
    float nearPlane;         /* @76 default 0.1 */
    float aspectRatio;       /* @80 */
    float fov;               /* @84 default 50 */
    float _pad[2];
} CameraInfo;

/* src/vk_engine.h:153-158 (64 B) */
typedef struct EnvironmentData {
    float horizonColor[4];   /* w = sun focus */
    float zenithColor[4];    /* w = sun intensity */
    float groundColor[3]; float _pad0;
    float lightDir[4];       /* w = environment on */
} EnvironmentData;

/* src/vk_engine.h:160-171 (40 B); the two bools occupy 4-byte slots */
typedef struct RayTracerData {
    uint32_t progressive;
    uint32_t singleRender;
    int32_t debug;           /* -1 off, 0 box heat map, 1 tri heat map, 2 both */
    uint32_t raysPerPixel;
    uint32_t bounceLimit;
    uint32_t sphereCount;
    uint32_t objectCount;
    uint32_t triangleCap;
    uint32_t boxCap;
    uint32_t sampleLimit;
} RayTracerData;

/* src/vk_engine.h:173-178 (208 B) */
typedef struct PushConstants {
    CameraInfo camInfo;          /* @0   */
    EnvironmentData environment; /* @96  */
    RayTracerData rayTraceParams;/* @160 */
    uint32_t frameCount;         /* @200 */
    uint32_t _pad;
} PushConstants;

/* src/vk_engine.h:125-132 (the placement half of ImGuiObject) */
typedef struct RtPlacement {
    float position[3];
    float rotation[3];       /* Euler degrees, applied T*Rx*Ry*Rz*S */
    float scale[3];
    uint32_t samplerIndex;
    uint32_t frontOnly;
} RtPlacement;

enum { RT_MAX_TEXTURES = 64, RT_MAX_MATERIALS = 10, RT_MAX_SPHERES = 10, RT_BVH_BINS = 20 };
/* Light queries (rt_set_tuning "light_queries") are answered from the list of emissive primitives while the scene's objects
 * with an emissive material have at most this many triangles between them; beyond it every query is traversed in full. */
enum { RT_EMIT_MAX_TRIS = 32 };

/* Borrowed views of the scene's host vectors (VulkanEngine members
 * spheres / rayMaterials / triPoints / triangles / objects / bvhNodes,
 * src/vk_engine.h:270-283). */
typedef struct RtSceneArrays {
    const Sphere* spheres;              uint32_t sphereCount;
    const RayMaterial* materials;       uint32_t materialCount;
    const TrianglePoint* triPoints;     uint32_t triPointCount;
    const Triangle* triangles;          uint32_t triangleCount;
    const RenderObject* objects;        uint32_t objectCount;
    const BVHNode* bvhNodes;            uint32_t bvhNodeCount;
} RtSceneArrays;

/* ------------------------------------------------------------------ */
/* (1) Scene surface — host only                                        */
/* ------------------------------------------------------------------ */
typedef struct rt_scene rt_scene;

int  rt_scene_create(rt_scene** out);
void rt_scene_destroy(rt_scene* s);
const char* rt_scene_last_error(const rt_scene* s);

/* rayMaterials.push_back (src/vk_engine.cpp:717-722); returns the index or <0 */
int  rt_scene_add_material(rt_scene* s, const RayMaterial* m);
/* a default-constructed RayMaterial (src/vk_engine.h:69-79) */
void rt_material_default(RayMaterial* m);
/* spheres[i] = ... (src/vk_engine.cpp:682-686); i < RT_MAX_SPHERES */
int  rt_scene_set_sphere(rt_scene* s, uint32_t i, const float position[3], float radius, uint32_t materialIndex);
void rt_placement_default(RtPlacement* p);

/* VulkanEngine::read_obj (src/vk_engine.cpp:800-1037). `material` is the
 * fallback material index for files without usemtl. A missing file is a
 * silent no-op returning 1 (the reference returns silently, :834). */
int  rt_scene_read_obj(rt_scene* s, const char* filePath, const RtPlacement* placement, int material);
/* VulkanEngine::read_mtl (src/vk_engine.cpp:1060-1167) without the image
 * uploads: map_* lines only claim texture slots (textures are never sampled
 * by the shader at this snapshot). */
int  rt_scene_read_mtl(rt_scene* s, const char* filePath);
/* A programmatic mesh goes through the same triangle/centroid/BVH path as an
 * OBJ group. positions/normals: 9 floats per triangle (corner-major);
 * uvs: 6 floats per triangle or NULL. */
int  rt_scene_add_mesh(rt_scene* s, const char* key, const float* positions, const float* normals,
                       const float* uvs, uint32_t triCount, const RtPlacement* placement, int material);
/* VulkanEngine::cornell_box (src/vk_engine.cpp:638-678); assetDir holds
 * light2.obj, plane.obj, ceiling.obj */
int  rt_scene_cornell_box(rt_scene* s, const char* assetDir);
/* VulkanEngine::prepare_storage_buffers (src/vk_engine.cpp:680-758): ten
 * zeroed spheres, the six built-in materials, the two cubes, cornell_box. */
int  rt_scene_prepare_default(rt_scene* s, const char* assetDir);
int  rt_scene_get_arrays(const rt_scene* s, RtSceneArrays* out);
/* The texture slots the MTL files claimed, in slot order (textures[texturesUsed], src/vk_engine.cpp:1109-1141): the host
 * decodes file i to RGBA8 (the reference: stb_image, STBI_rgb_alpha, src/vk_textures.cpp:103-113) and hands all of them to
 * rt_upload_textures. rt_scene_add_texture claims the next slot for a file no MTL names (bind it with a material's
 * albedoIndex); rt_scene_set_material overwrites rayMaterials[i] (the material editor's in-place edit, :1536-1545). */
uint32_t rt_scene_texture_count(const rt_scene* s);
const char* rt_scene_texture_path(const rt_scene* s, uint32_t i);
int  rt_scene_add_texture(rt_scene* s, const char* path);
int  rt_scene_set_material(rt_scene* s, uint32_t i, const RayMaterial* m);
/* rt_update_points (below) on the scene's own arrays: replaces triPoints[first, first + count) and refits, by the same rule, the boxes
 * of bvhNodes of every mesh that uses one of these points; triangles, leaf ranges and node numbering stay. rt_scene_get_arrays then
 * describes what a context holds after the same rt_update_points: for the oracle, a later plain rt_upload_scene, the other ranks of
 * a multi-GPU run. Refused with a message, the arrays untouched: a range past the point count; points NULL with count > 0; a
 * position component that is not finite; and, of the scene itself (the builders make none of these): a mesh that shares BVH nodes
 * with another mesh, a mesh whose triangles are not one contiguous range, a BVH child, leaf triangle or triangle point index out of
 * range. count == 0 succeeds and changes nothing. */
int  rt_scene_update_points(rt_scene* s, const TrianglePoint* points, uint32_t first, uint32_t count);
/* index of a material loaded from an MTL file, key "<mtlpath>/<name>"; -1 if absent */
int  rt_scene_find_material(const rt_scene* s, const char* key);
/* BVH build statistics of the most recent build (printed by the reference, :1187-1193) */
int  rt_scene_last_bvh_stats(const rt_scene* s, uint32_t* nodeCount, uint32_t* maxDepth, uint32_t* minDepth, uint32_t* maxTri);

/* BVH builder plug. The scene half builds every mesh's BVH on the host, as the reference does
 * (build_bvh / subdivide / find_split_plane, src/vk_engine.cpp:1169-1337). A hook replaces that step for the meshes added
 * after it is set: it receives the mesh's triangles and centroids (the last `count` elements of the scene arrays, the
 * triangles' v0/v1/v2 indexing `points`), must reorder both the way the reference's partition loop does, write the
 * nodes in the reference's numbering (children of the node at nodeBase + i at nodeBase + nodes[i].index ... as absolute
 * indices, leaves with absolute triangle indices from triIndex0) and report {maxDepth, minDepth, maxTriCount}.
 * rt_bvh_hook is such a hook: the same tree, built on the GPU of the rt_ctx passed as `user` (rt_bvh_build). */
typedef int (*RtBvhBuildHook)(void* user, const TrianglePoint* points, uint32_t pointCount, Triangle* triangles, float* centroids,
                              uint32_t count, uint32_t triIndex0, uint32_t nodeBase, BVHNode* nodesOut, uint32_t nodeCapacity,
                              uint32_t* nodeCountOut, uint32_t statsOut[3]);
int  rt_scene_set_bvh_hook(rt_scene* s, RtBvhBuildHook hook, void* user);

/* Camera/constants half of run_compute (src/vk_engine.cpp:1631-1661):
 * cameraRotation = rotY * rotX * rotZ from Euler degrees. */
void rt_camera_rotation(const float anglesDeg[3], float outMat4[16]);
/* defaults of src/vk_engine.h:145-171,325 (angles {4,0,0}) with aspect = W/H */
void rt_push_constants_default(PushConstants* pc, uint32_t width, uint32_t height);
/* object.transformMatrix = T*Rx*Ry*Rz*S (src/vk_engine.cpp:1012-1016) */
void rt_transform_matrix(const RtPlacement* p, float outMat4[16]);

/* ------------------------------------------------------------------ */
/* (2) Device half                                                      */
/* ------------------------------------------------------------------ */
typedef struct rt_ctx rt_ctx;

/* Global counters summed over every closest-hit query the device executed
 * since the last rt_reset_counters. */
typedef struct RtCounters {
    uint64_t boxTests;      /* reference stats[0] semantics, raytrace.comp:338, all queries */
    uint64_t triTests;      /* reference stats[1] semantics, raytrace.comp:310, all queries */
    uint64_t raysTraced;    /* scene queries executed on the device: main rays, and the light queries (NEE ray, cosine probe) that
                             * their creators could not answer from the emitter list; boxTests / triTests count these queries,
                             * the light queries up to the hit that answers them */
    uint64_t raysHit;       /* of those, queries that reported a hit */
    uint64_t raysReference; /* queries the reference megakernel would have issued for the same paths */
    uint64_t paths;         /* trace() calls finished (pixel samples) */
    uint64_t segments;      /* path segments shaded */
    uint64_t traceLaunches; /* launches of the traversal kernel */
    uint64_t emitterTests;  /* emissive primitives tested directly by the creators of light queries (NEE ray, cosine probe) */
    uint64_t skippedBoxTests; /* of boxTests: the two tests the reference makes on the children of an object's root, charged for objects
                             * a ray was taken past without entering them (object masks, padded world boxes, the object hierarchy);
                             * boxTests - skippedBoxTests were executed. 0 for scenes without placed objects */
} RtCounters;

/* One closest-hit record of calculateIntersections (raytrace.comp:276-353) */
typedef struct RtHit {
    float dst;              /* RT_MISS_DST on miss */
    uint32_t didHit;
    uint32_t isSphere;
    uint32_t objectHitIndex;/* object index, or sphere index when isSphere */
    uint32_t triHitIndex;
    uint32_t materialIndex;
    uint32_t frontFace;
    float hitPoint[3];
    float normal[3];
    uint32_t boxTests;      /* this query's stats[0] */
    uint32_t triTests;      /* this query's stats[1] */
} RtHit;

int  rt_device_count(int* out);
int  rt_create(int device, rt_ctx** out);
void rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL = ctx's own */
int  rt_set_stream(rt_ctx* ctx, void* hipStream);

/* copy_buffer x6 (src/vk_engine.cpp:686,753-757): takes the reference's AoS
 * host arrays, converts to the device layouts, uploads. Borrowed for the call. */
int  rt_upload_scene(rt_ctx* ctx, const RtSceneArrays* scene);
/* Deforming meshes in place ("Deforming meshes"). rt_upload_scene_dynamic does what rt_upload_scene does and keeps on the
 * device what a later refit needs: a copy of triPoints, the triangles' {v0, v1, v2, frontOnly} and the refit plan (per mesh, i.e. per
 * distinct bvhIndex: its leaves and its interior nodes level by level in the device numbering). Refused with a message, the context
 * left as it was: a scene rt_upload_scene refuses; a mesh that shares BVH nodes with another mesh; a mesh whose triangles are not one
 * contiguous range. It resets the temporal history as rt_upload_scene does.
 * rt_update_points replaces triPoints[first, first + count) of the scene uploaded that way: positions, normals and both uv halves.
 * Topology is kept (triangles, leaf ranges, node numbering, hot pairs); the boxes of every mesh that uses one of these points are
 * refit bottom-up on the device. The rule: a leaf's box starts from the builder's sentinels (+1e30, -1e30) and grows by its triangles
 * in order, corners v0, v1, v2, with the builder's comparisons (lo = p < lo ? p : lo, hi = hi < p ? p : hi); an interior node's box is
 * its left child's grown by its right child's with the same comparisons. The builder gives every node the exact min / max of its
 * triangles' vertices, so these are the boxes it would give this topology.
 * Contract: when the call returns, every device table equals, byte for byte, what rt_upload_scene would upload for the same arrays
 * with the points replaced and the boxes of bvhNodes refit by the rule (rt_scene_update_points makes exactly those arrays): nodes,
 * the interleaved pairs, triangle positions / normals / uvs, and through the roots' boxes the padded world boxes, the mask boxes, the
 * object hierarchy, the origin limit of the skipping code and the emitter list's triangles. Every entry point reads those tables.
 * The measured ray cost, the textures and the tuning stay. Synchronous, like rt_upload_scene. The temporal history is not reset:
 * with rt_temporal_track_motion on, every object whose mesh was refit since the last rt_temporal_accumulate has no history in the
 * next one (RT_MOTION_REPLACED, counted in replacedObjects); with it off the pass takes the scene to be static, as after an
 * rt_update_objects: call rt_temporal_reset.
 * What a refit does not do: it keeps the topology the builder chose for the old shape. Under large deformations the boxes overlap
 * more and rays test more of them (boxTests per ray in rt_get_counters shows it); the cure is a rebuild and rt_upload_scene_dynamic.
 * Refused with a message before anything is written: a scene not uploaded with rt_upload_scene_dynamic; a range that runs past the
 * point count; points NULL with count > 0; a position component that is not finite (the builder's comparisons and the kernels'
 * treat NaN differently). count == 0 succeeds and does nothing. */
int  rt_upload_scene_dynamic(rt_ctx* ctx, const RtSceneArrays* scene);
int  rt_update_points(rt_ctx* ctx, const TrianglePoint* points, uint32_t first, uint32_t count);
/* Textures (bindings raytrace.comp:122,148, upload src/vk_textures.cpp:103-200). Slot i of the scene's texture
 * table, as R8G8B8A8_SRGB texels, rows top to bottom (what stbi_load(..., STBI_rgb_alpha) returns). The snapshot's shader
 * computes hit.uv (raytrace.comp:249-256) and never samples; the semantics here are this build's declared choice
 * ("parity unpinned"): a triangle hit whose material has albedoIndex >= 0 multiplies the material's albedo by
 * the texel at (u, 1 - v) of hit.uv — OBJ's v runs upwards, the image's rows downwards; with the flip dread.obj shows its
 * plate, bolts and wheels where the reference's renders/dread_texture.png has them — nearest filter, sampler
 * RenderObject.samplerIndex (0 = repeat, 1 = clamp to edge, :525-531), sRGB -> linear. Spheres are not textured.
 * The other three slots a material carries (src/vk_engine.cpp:1109-1141: map_Ks -> metalnessIndex, map_d -> alphaIndex,
 * map_bump -> bumpIndex) are declared likewise, all on the red channel of the texel at hit.uv (rt_det_math.h, "the other three
 * map slots"): alpha — a triangle hit whose texel decodes below 0.5 is no hit, for every ray (inside calculateIntersections'
 * triangle loop, raytrace.comp:305-322); metalness — the decoded texel replaces RayMaterial.reflectance (which the shader only
 * compares with 0, :509); bump — the decoded texel is a height and the interpolated normal is tilted by the height steps to the
 * next texel of the row and of the column along the triangle's dP/du, dP/dv (rt_bump_normal). A slot < 0 or beyond the uploaded
 * table binds nothing. A scene that binds one of the three is rendered by the multi-kernel pipeline (k_shade_maps,
 * k_trace_pw_alpha) whatever "pipeline" says, unless "fused_maps" is 1 (rt_set_tuning): then it picks its pipeline as any other
 * scene does and the fused one runs k_render_fused_maps. One whose emissive material has an alpha map traces its light queries
 * in full.
 * Borrowed for the call; n = 0 removes all textures. */
typedef struct RtTexture {
    uint32_t width, height;
    const uint8_t* rgba8;   /* width * height * 4 bytes */
} RtTexture;
int  rt_upload_textures(rt_ctx* ctx, const RtTexture* textures, uint32_t n);
/* update_buffer (src/vk_engine.cpp:1545,1572,1603) */
int  rt_update_materials(rt_ctx* ctx, const RayMaterial* m, uint32_t n);
int  rt_update_spheres(rt_ctx* ctx, const Sphere* s, uint32_t n);
int  rt_update_objects(rt_ctx* ctx, const RenderObject* o, uint32_t n);

/* run_compute: one dispatch of the path tracer over rows
 * y = row0 + k*rowStride, k in [0,nRows) of a width x height image, using the
 * global pixel index for the RNG seed so any tiling gives identical pixels.
 * samples per pixel = singleRender ? sampleLimit : raysPerPixel (:570).
 * d_rgba: device pointer to nRows*width*4 floats (RGBA fp32, before any 8-bit
 * step), or NULL to use the ctx's own framebuffer (rt_read_rgba_f32).
 * Asynchronous on the ctx stream; rt_sync waits. The call returns as soon as the dispatch is enqueued: the multi-kernel
 * pipeline enqueues every round it can need (each kernel reads its queue length on the device and leaves at once when
 * there is nothing left) in up to "lanes" parts on streams of their own, forked from and joined to the ctx stream, and
 * never waits for the device (tests/test_async_contract.py: the host is held for less than a tenth of the dispatch's
 * time on the bench frame in either pipeline). One exception: a context's first dispatch of >= 8 M pixel-samples of a
 * scene whose ray cost it has not measured yet is preceded by a small blocking probe dispatch (a few ms, rt_ray_cost;
 * "probe" 0 turns it off). */
int  rt_render(rt_ctx* ctx, const PushConstants* pc, uint32_t width, uint32_t height,
               uint32_t row0, uint32_t rowStride, uint32_t nRows, float* d_rgba);
/* nFrames consecutive progressive dispatches of the same tile — the same pixels, bit for bit, as nFrames calls of rt_render
 * with frameCount = pc->frameCount, pc->frameCount + 1, ... (the reference's frame loop, src/vk_engine.cpp:1782-1814, runs them
 * one after the other and waits for each). Frames are independent until they are blended (each has its own RNG seeds,
 * raytrace.comp:562-564), and a pixel's samples are serial, so what fills a GPU is paths: the frames' paths share one dispatch
 * (one launch of the fused kernel, or the queues of every round of the multi-kernel pipeline; the pipeline is chosen by the
 * paths of all the frames together) and the frames are blended into d_rgba in order afterwards. A 1/8-height tile of a
 * 1080p frame has fewer pixels than the GPU has resident lanes; eight frames of it run like a whole frame, and the
 * traversal gets cheaper per ray the more paths a dispatch holds. Not for the debug heat maps (rendered frame by frame then).
 * "frames_per_launch" (rt_set_tuning) caps the frames per dispatch (0 = as many as fit), "frames_max_mslots" the paths of
 * one dispatch in millions (default 24: 5.8 GB of path state); more frames than that go in several dispatches. */
int  rt_render_frames(rt_ctx* ctx, const PushConstants* pc, uint32_t width, uint32_t height,
                      uint32_t row0, uint32_t rowStride, uint32_t nRows, uint32_t nFrames, float* d_rgba);
/* rt_render_frames with a sample count per pixel. d_sampleMap: device pointer to nRows*width counts in d_rgba's pixel order (row k,
 * column x at k*width + x), read by the dispatch, so it stays valid and unchanged until the stream has passed it. With S what
 * rt_render would use (singleRender ? sampleLimit : raysPerPixel) and n_p = min(map[p], S):
 *  - n_p >= 1: pixel p is written, bit for bit, as rt_render_frames would write it with the same arguments and S replaced by n_p
 *    (a pixel's samples are serial and its RNG seed depends on its global pixel index and frameCount only): the mean over n_p
 *    samples, the progressive blend with what d_rgba holds, NaN -> magenta, frameCount + f for frame f;
 *  - n_p = 0: pixel p of d_rgba is not written, rgb or alpha, in any of the nFrames frames, and no path is made for it (a hole in
 *    the multi-kernel pipeline's queues; a lane of the fused kernel that takes its next pixel at once);
 *  - d_sampleMap NULL: rt_render_frames, exactly.
 * Both pipelines, 1..4 parts, camera_reuse on and off, scenes with maps, the ctx framebuffer (d_rgba NULL) and row tiling work as
 * in rt_render. A call rt_render_frames would split (frames_per_dispatch) uses the same map for every piece. The launch policy
 * sees S as the dispatch's sample count, and the multi-kernel pipeline enqueues up to S * (bounceLimit + 1) rounds as before; the
 * ray-cost probe ignores the map. `paths` grows by the sum of n_p per frame, the other counters by the work done. Refused with a
 * message: the debug heat maps (rayTraceParams.debug >= 0) with a map. Asynchronous on the ctx stream, checked like rt_render. */
int  rt_render_sampled(rt_ctx* ctx, const PushConstants* pc, uint32_t width, uint32_t height,
                       uint32_t row0, uint32_t rowStride, uint32_t nRows, uint32_t nFrames,
                       const uint32_t* d_sampleMap, float* d_rgba);
int  rt_sync(rt_ctx* ctx);
/* forget the ctx's own framebuffer: the next rt_render(…, NULL) starts a new progressive history from a zeroed image */
int  rt_clear_framebuffer(rt_ctx* ctx);
/* copies the ctx's own framebuffer of the last rt_render(…, NULL) to host */
int  rt_read_rgba_f32(rt_ctx* ctx, float* hostOut, size_t nFloats);
/* 8-bit sRGB-encoded RGBA of the same framebuffer (the reference's display format) */
int  rt_read_rgba8_srgb(rt_ctx* ctx, uint8_t* hostOut, size_t nBytes);

/* calculateIntersections for n caller-supplied rays (host arrays, 3 floats
 * each), for kernel-level parity tests. Synchronous. */
int  rt_trace_rays(rt_ctx* ctx, uint32_t n, const float* origins, const float* dirs, RtHit* hitsOut);

/* First-hit AOVs: one pass over the rows y = row0 + k*rowStride, k in [0,nRows) of a width x height image, as rt_render has
 * them. It shoots each pixel's camera ray (origin camInfo.pos, the direction every sample of the pixel starts with in
 * rt_render: the reference does not jitter, raytrace.comp:547-556) and writes calculateIntersections' closest hit for it into
 * per-pixel planes: the same record, bit for bit, as rt_trace_rays returns for that ray, with the counts of rayTraceParams and
 * alpha maps cutting hits out as in rendering. Each non-NULL field holds nRows*width*4 elements; pixel (k, x) starts at
 * (k*width + x)*4, the order of rt_render's d_rgba. */
typedef struct RtAovBuffers {
    float*    normalDepth; /* xyz: hit normal as RtHit has it (unit, turned towards the side the ray came from, bump-tilted where
                            * a bump map binds); w: hit dst along the unit camera ray. Miss: (0, 0, 0, RT_MISS_DST) */
    float*    position;    /* xyz: hit point (world); w: 1 on a hit. Miss: all 0 */
    float*    albedo;      /* rgb: the material's albedo; a triangle hit whose material binds an uploaded albedo map multiplies it
                            * by the texel as the diffuse branch of shading does. Spheres are untextured. a: 1 on a hit. Miss: all 0 */
    float*    rayDir;      /* xyz: the camera ray's direction; w: 0 */
    uint32_t* ids;         /* x: object index, or sphere index; y: triangle index (0 for spheres); z: material index;
                            * w: bit 0 hit, bit 1 sphere, bit 2 frontFace. Miss: (~0u, ~0u, ~0u, 0) */
} RtAovBuffers;
/* Asynchronous on the ctx stream, like rt_render, and checked like it (geometry, rows, scene, counts). d_out: device planes
 * (NULL fields are skipped), or NULL: the ctx keeps all five (rt_read_aovs). The pass runs the ordinary traversal kernel
 * (rt_last_kernel names it) and changes nothing a later rt_render produces: not the ctx framebuffer nor its progressive
 * history, not the pipeline, parts or ray-cost choices. Its traversal work goes to boxTests, triTests, skippedBoxTests,
 * raysTraced, raysHit and traceLaunches of rt_get_counters, from a counter block of its own that the ray-cost measurement
 * never reads; rt_reset_counters clears it. */
int  rt_render_aovs(rt_ctx* ctx, const PushConstants* pc, uint32_t width, uint32_t height,
                    uint32_t row0, uint32_t rowStride, uint32_t nRows, const RtAovBuffers* d_out);
/* copies the ctx-owned planes of the last rt_render_aovs(…, NULL) to the non-NULL host fields (nPixels = nRows*width of that
 * pass); blocks */
int  rt_read_aovs(rt_ctx* ctx, const RtAovBuffers* hostOut, size_t nPixels);

/* Mirror-following guide planes ("Mirror-following guide planes"): the planes rt_denoise should be guided by where the
 * camera ray meets a mirror, which has one normal field, one depth ramp and one albedo and so tells an edge-stopping filter nothing
 * of the image it shows. A mirror segment of a path is deterministic (a plain reflect, no random number, radiance 1), so every
 * sample of a pixel runs the same chain of mirror segments from the camera to the first surface that is no mirror, and this pass
 * traces it once. Per pixel, segment 0 is rt_render_aovs' camera ray; segment j's hit is calculateIntersections' closest hit (the
 * record rt_trace_rays returns for the ray, alpha cut-outs as in rendering). A segment continues when it hit, j < maxBounces and
 * the hit is a mirror for shading: reflectance != 0, the reflectance being the metalness texel on a triangle hit whose material
 * binds an uploaded metalness map. The next ray is the one shading would trace, bit for bit: direction reflect(dir, normal) with
 * the (bump-tilted) normal of the hit, origin hitPoint + (normal * 1) * 0.00001. The chain ends at the first segment that does
 * not continue; L, 0 <= L <= maxBounces, is the number of segments before it. Dielectrics branch on a random draw: a chain stops
 * on them as on any other surface.
 * The guide planes have RtAovBuffers' layout and may be passed as rt_denoise's d_aovs: normalDepth.xyz, position, albedo and
 * ids.xyz are the final segment's, exactly as rt_render_aovs would write them for that ray; normalDepth.w is the path length
 * ((d0 + d1) + d2) + ... in fp32 on a final hit, and a final miss writes the miss record unchanged (RT_MISS_DST, not a sum); rayDir
 * is the final segment's direction; ids.w keeps bits 0-2 of the final hit, bit 3 says the chain was cut (the final hit is itself a
 * mirror: j reached maxBounces), bits 8-11 hold L. With maxBounces = 0, or in a scene without mirrors, the guide planes equal
 * rt_render_aovs' bit for bit, except ids.w bit 3 on mirror hits.
 * maxBounces 0..8. d_guides: device planes (NULL fields are skipped), or NULL: a ctx-owned set of their own (rt_read_guides), which
 * is not the set rt_render_aovs keeps: rt_denoise(d_aovs = NULL) still means the first-hit planes. d_firstHit: device planes that
 * receive what rt_render_aovs would write for the tile, bit for bit, from the same first traversal (NULL fields are skipped), or
 * NULL: not wanted. No plane of d_guides may overlap one of d_firstHit. rt_temporal_accumulate keeps taking the first-hit planes: a
 * guide position is a point seen in a mirror, which does not reproject through the camera.
 * Asynchronous on the ctx stream and checked like rt_render_aovs; the host never learns how many chains are alive: it enqueues
 * maxBounces + 1 traversal launches, each over the rays still alive, and one without rays costs its launches. Like rt_render_aovs
 * the pass changes nothing a later rt_render produces (framebuffer, progressive history, pipeline, parts and ray-cost choices,
 * rt_last_parts, rt_last_pipeline) and nothing rt_render_aovs keeps; its traversal work goes to the same counters from the same
 * block, traceLaunches counting one per round. */
int  rt_render_guides(rt_ctx* ctx, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                      uint32_t nRows, uint32_t maxBounces, const RtAovBuffers* d_guides, const RtAovBuffers* d_firstHit);
/* copies the ctx-owned guide planes of the last rt_render_guides(…, d_guides = NULL) to the non-NULL host fields (nPixels =
 * nRows*width of that pass); blocks */
int  rt_read_guides(rt_ctx* ctx, const RtAovBuffers* hostOut, size_t nPixels);

/* Ray queries on batches of the caller's own rays ("Ray queries"): the closest hit, or only whether anything is hit
 * within a limit. The arrays of a batch are packed: ray i's origin at origins[3 i .. 3 i + 2], likewise dirs (rt_trace_rays'
 * layout; a contiguous (n, 3) fp32 tensor). */
typedef struct RtRayBatch {
    const float* origins;  /* n x 3 floats, packed */
    const float* dirs;     /* n x 3; not renormalised: distances are in units of |dir|, as in rt_trace_rays */
    const float* tmax;     /* n floats, or NULL: no limit */
    uint32_t n;
} RtRayBatch;
/* Contract. Ray i with limit T (tmax[i]; RT_MISS_DST when tmax is NULL) runs calculateIntersections (raytrace.comp:276-353) with
 * its running closest distance started at T instead of at the miss distance: the sphere loop accepts a sphere with dst < T, a box is
 * entered on d < best and a triangle accepted on dst < best as ever, and alpha maps cut hits out as in rendering.
 *  - rt_query_closest, tmax NULL: d_hits[i] equals what rt_trace_rays returns for the ray, bit for bit, in every field except
 *    boxTests and triTests, which are 0 (the pass runs the kernels without per-ray counters, the ones rendering runs). With a
 *    limit: that same record when its dst < T, otherwise the miss record (dst == RT_MISS_DST, didHit == 0, the rest zero).
 *  - rt_query_occluded: d_occluded[i] is 1 exactly when that search, started at T, accepts any primitive, else 0. Until the first
 *    acceptance the bound is the constant T, so the answer does not depend on the order primitives are visited in, and therefore
 *    not on the kernel, the knobs, the parts or the object hierarchy. Hence occluded => (closest.didHit && closest.dst < T) on
 *    every ray, exactly; the converse holds except where closest.dst lies within the box tests' rounding below T. The search ends
 *    at the first acceptance (the early exit of the light queries).
 *  - A limit that is NaN or <= 0 makes the ray a miss / unoccluded without being traced. n == 0 succeeds and does nothing.
 * The struct is read on the host; with the plain names its three arrays and the output are device pointers and the call is
 * asynchronous on the ctx stream (the arrays stay valid and unchanged until the stream has passed it); the _host names take host
 * arrays and block. Both run in path-state slots [0, n), as rt_render_aovs does, always through the persistent-wave traversal
 * kernels (k_trace_pw...; rt_last_kernel names the one that ran) whatever "trace_variant" says: k_trace starts every ray at the
 * miss distance. They count into the AOV passes' counter block (raysTraced: the rays that had to be traversed; raysHit: of a
 * closest pass the rays that hit, of an occlusion pass the traversed rays that came out unoccluded) and change nothing a later
 * rt_render, rt_render_aovs, rt_denoise or rt_temporal_accumulate produces or chooses: not the framebuffer or its progressive
 * history, not rt_last_pipeline, rt_last_parts or the ray cost.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; origins, dirs or the output NULL with
 * n > 0; n >= 2^30 (the slot ids). */
int  rt_query_closest(rt_ctx* ctx, const RtRayBatch* d_rays, RtHit* d_hits);
int  rt_query_occluded(rt_ctx* ctx, const RtRayBatch* d_rays, uint8_t* d_occluded);
int  rt_query_closest_host(rt_ctx* ctx, const RtRayBatch* rays, RtHit* hits);
int  rt_query_occluded_host(rt_ctx* ctx, const RtRayBatch* rays, uint8_t* occluded);

/* All-hit ray queries ("All-hit ray queries"; include/rt_ray_hits.h states the rule, both sides compile it): every
 * surface a ray crosses below its limit, the first k of them in order, and how many there are.
 * Contract. Ray i has the limit T (tmax[i]; RT_MISS_DST when tmax is NULL). Its candidate set C is what calculateIntersections
 * (raytrace.comp:276-353) accepts when its bound is the constant T and never shrinks:
 *  - spheres: sphereIntersection's arithmetic, both roots. The entry root (b - sqrtd) / a counts when it is >= 0: a front face, the
 *    record the reference gives. The exit root (b + sqrtd) / a counts when it is >= 0: a back face, normal -normalize(p - c). Each
 *    must also be < T. From inside a sphere only the exit exists, as in the reference.
 *  - objects in index order, the ray taken to object space as ever, the object's root entered untested; a child box is entered
 *    when boxIntersection(...) < T; a triangle is a candidate when triangleIntersection says didHit, dst < T and its alpha texel
 *    does not cut it out (as in rendering).
 * The bound is constant, so C does not depend on the order anything is visited in: not on the kernel, the stack, the knobs or the
 * device's node numbering.
 *  - d_counts[i] = |C|, exact whatever k is.
 *  - d_hits[i * k .. i * k + k - 1]: the first min(k, |C|) members of C in ascending order of the key (dst as an fp32 compare;
 *    spheres before triangles; the lower sphere or object index; the lower triHitIndex; a sphere's entry before its exit), then
 *    the miss record (dst == RT_MISS_DST, everything else 0) in the remaining slots.
 *  - A member's record is the RtHit rt_query_closest builds for that primitive (hitPoint and normal through the forward matrix,
 *    bump maps as in rendering, materialIndex and frontFace as ever, boxTests and triTests 0): for the primitive rt_query_closest
 *    reports it equals rt_query_closest's record byte for byte.
 *  - The closest hit is always a member of C: every box the shrinking search enters passes d < best <= T.
 *  - hits[0].dst <= closest.dst on every ray. It can be strictly less: a shrinking bound can prune a box whose fp32 distance
 *    rounds above the dst of a triangle inside it, and the constant bound does not.
 *  - k == 0 is allowed: counts only, d_hits may be NULL. A limit that is NaN or <= 0 gives count 0 and miss records without a
 *    search. n == 0 succeeds and does nothing.
 * rt_query_hits: the struct is read on the host, its arrays, d_hits and d_counts are device pointers, asynchronous on the ctx
 * stream (the arrays stay valid and unchanged until the stream has passed it). rt_query_hits_host takes host arrays, stages them
 * through a ctx buffer and blocks. One lane per ray, no path state: the search (k_ray_hits) and, with k > 0, a resolve pass of
 * one lane per slot (k_ray_hits_resolve). rt_last_kernel names the search that ran: k_ray_hits<24, false> while the scene's
 * deepest BVH leaf is at most 24 levels down, k_ray_hits<64, true> beyond (its list lives in a ctx buffer instead of LDS; a scene
 * deeper than 64 is refused). The pass adds to the AOV passes' counter block: boxTests, triTests, raysTraced (the rays searched),
 * raysHit (the rays with count > 0), and changes nothing a later render or query produces or chooses.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; (n == 0 succeeds here;) origins or
 * dirs NULL; k > RT_HITS_MAX_K; d_counts NULL, or d_hits NULL with k > 0; n >= 2^30.
 * rt_hits_walk_host: the definition as a plain loop over the host arrays (bvhNodes in the host's numbering, an explicit stack, the
 * constant bound), no ctx, no GPU; sphereCount and objectCount as rayTraceParams gives them (at most the arrays' counts);
 * textures as rt_upload_textures takes them (NULL, 0: no maps). -1: a NULL argument, k > RT_HITS_MAX_K, n >= 2^30, or arrays
 * that index out of range. */
#define RT_HITS_MAX_K 8
int  rt_query_hits(rt_ctx* ctx, const RtRayBatch* d_rays, uint32_t k, RtHit* d_hits, uint32_t* d_counts);
int  rt_query_hits_host(rt_ctx* ctx, const RtRayBatch* rays, uint32_t k, RtHit* hits, uint32_t* counts);
int  rt_hits_walk_host(const RtSceneArrays* scene, uint32_t sphereCount, uint32_t objectCount, const RtTexture* textures,
                       uint32_t nTextures, const RtRayBatch* rays, uint32_t k, RtHit* hits, uint32_t* counts);

/* Radiance queries: the path-traced radiance along the caller's own rays ("Radiance queries"): what rt_render
 * estimates for the pinhole camera's rays, for any batch of rays: baking, probes, other camera models, jittered pixels, rays
 * made on the device. */
typedef struct RtRadianceParams {
    uint32_t samples;      /* >= 1: paths per ray; every sample starts with the same ray, its RNG state running on (raytrace.comp:571-573) */
    uint32_t bounceLimit;  /* as rayTraceParams.bounceLimit; < 2^28 - 1 */
    uint32_t progressive;  /* 0: out = mean; 1: blended with what d_radiance holds, weight 1 / (frameCount + 1), as rt_render */
    uint32_t frameCount;   /* seeds the frame (startingSeed) and weighs the blend */
} RtRadianceParams;
void rt_radiance_params_default(RtRadianceParams* p);   /* 1, 8, 0, 0 */
/* Contract. Ray i runs trace() (raytrace.comp:495-534) `samples` times from origin origins[3 i ..] and direction dirs[3 i ..].
 * The direction is used as given: the estimator assumes unit length and nothing renormalises it. The RNG state of the ray's
 * first draw is (d_ids ? d_ids[i] : i) + startingSeed, startingSeed = uint(random(frameCount) * 23892183) as rt_render computes
 * it. d_radiance[4 i .. 4 i + 3] receives what rt_render gives a pixel (raytrace.comp:574-593): rgb the sum over the samples
 * divided by (float)samples, blended with what d_radiance[4 i ..] holds when `progressive`, (1, 0, 1) where that is NaN or Inf;
 * alpha 1.
 *  - Hence a batch of the camera rays of a W x H frame (origin camInfo.pos, directions the rayDir plane of rt_render_aovs) with
 *    ids gy * W + gx equals rt_render's image for the same constants, bit for bit.
 *  - A ray's result depends on (origin, dir, id, params, env, scene) only: not on n, its place in the batch, the parts,
 *    "camera_reuse", "light_queries" or the traversal knobs.
 *  - tmax of the batch must be NULL: a reach limit on a path has no meaning. env NULL: the environment is off. The sphere and
 *    object counts are the uploaded scene's, as in the ray queries; texture maps take part as in rendering.
 * The pass always runs the multi-kernel pipeline (k_radiance_rays, rounds of the persistent-wave traversal and k_shade_rays,
 * k_radiance_resolve), in parts as a dispatch of n paths would, ray i in path-state slot i. A batch of more than
 * "radiance_max_kslots" x 1024 rays (rt_set_tuning) runs as consecutive pieces of at most that many rays, each in slots
 * [0, piece), with the same bits. The struct, the params and env are read on the host. With the plain name the arrays, d_ids and
 * d_radiance (16-byte aligned, as rt_render's image) are device pointers and the call is asynchronous on the ctx stream: the arrays stay valid and unchanged until the
 * stream has passed it (the origins are read again wherever a sample ends). The _host name takes host arrays, stages them
 * through a ctx buffer and blocks.
 * It changes nothing a later rt_render, rt_render_aovs, rt_denoise or rt_temporal_accumulate produces or chooses: not the ctx
 * framebuffer or its progressive history, not rt_last_pipeline, rt_last_parts or rt_ray_cost (no snapshot, no probe). Its
 * counters go to the AOV passes' block, all fields of them: rt_get_counters' paths grows by n x samples. rt_last_kernel names
 * the traversal kernel that ran.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch or NULL params; (n == 0 succeeds here
 * and does nothing;) origins, dirs or the output NULL; tmax not NULL; samples 0; bounceLimit >= 2^28 - 1; n >= 2^30. */
int  rt_query_radiance(rt_ctx* ctx, const RtRayBatch* d_rays, const uint32_t* d_ids, const RtRadianceParams* params,
                       const EnvironmentData* env, float* d_radiance);
int  rt_query_radiance_host(rt_ctx* ctx, const RtRayBatch* rays, const uint32_t* ids, const RtRadianceParams* params,
                            const EnvironmentData* env, float* radiance);

/* Baked light at points ("Irradiance and SH probes"; include/rt_irradiance.h states the rule, both sides compile it):
 * the irradiance at surface points with normals (a lightmap texel, a baked vertex colour), and the spherical-harmonic
 * coefficients of the radiance around free points (the probes of an irradiance volume). Each point shoots `samples` rays by a
 * fixed rule, rt_query_radiance's pipeline estimates the radiance along each with one path, and the records are summed in a
 * fixed order. */
typedef struct RtPointNormalBatch {
    const float* points;   /* n x 3 floats, packed */
    const float* normals;  /* n x 3; used as given (unit length is assumed); the probe form ignores it, may be NULL */
    uint32_t n;
} RtPointNormalBatch;
typedef struct RtIrradianceParams {
    uint32_t samples;      /* S, rays per point: 1 .. 2^24 - 1, and at most one radiance piece ("radiance_max_kslots" x 1024) */
    uint32_t bounceLimit;  /* as rayTraceParams.bounceLimit; < 2^28 - 1 */
    uint32_t progressive;  /* 0: the estimate; 1: blended with what the output holds, weight 1 / (frameCount + 1), as rt_render */
    uint32_t frameCount;   /* seeds the directions and the paths, and weighs the blend */
    float bias;            /* irradiance form: the origin is p + (n * 1) * bias; finite, >= 0 */
} RtIrradianceParams;
void rt_irradiance_params_default(RtIrradianceParams* p);   /* 64, 8, 0, 0, 0.00001f (the next-ray origin of shading) */
/* Contract. Point i has the id pid = d_ids ? d_ids[i] : i. Its sample s (0 <= s < S) is a ray:
 *  - directions, a shifted Hammersley set per point: st = rt_ao_state(pid, 0, frameCount); u1 = rt_random(&st), u2 = rt_random(&st);
 *    r1 = ((float)s + u1) / (float)S; r2 = v + u2, minus 1 when >= 1, v = (float)(bitreverse32(s) >> 8) * 2^-24.
 *    Irradiance form: cosineHemisphereDir's arithmetic (raytrace.comp:405-424, as rt_cosine_hemisphere_dir evaluates it) about the
 *    normal, r1 under the square roots and r2 the azimuth: density cos / pi over the hemisphere.
 *    Probe form: z = 1 - 2 r1, rho = rt_sqrt(rt_max(0, 1 - z z)), phi = 2 pi r2, dir = (rho cos phi, rho sin phi, z) in world axes:
 *    density 1 / (4 pi) over the sphere.
 *  - origin: p + (n * 1) * bias (irradiance form), p itself (probe form).
 *  - L_s: the rgb rt_query_radiance gives that ray with the RNG id pid * S + s (32 bits, wrapping), one sample, `bounceLimit`,
 *    `frameCount`, not blended, under `env`: (1, 0, 1) where the path's radiance is NaN or Inf.
 *  - rt_query_irradiance: d_out[4 i .. 4 i + 2] = E = pi * (sum of L_s) / (float)S, d_out[4 i + 3] = 1.
 *  - rt_query_sh_probes: d_out[27 i + 3 j + c] = 4 pi * (sum of L_s[c] * Y_j(dir_s)) / (float)S for the nine real spherical
 *    harmonics of bands 0 to 2 in the order 1, y, z, x, xy, yz, 3 z^2 - 1, x z, x^2 - y^2, with the constants 0.282095, 0.488603,
 *    1.092548, 0.315392, 0.546274, in world axes (the scene's "up" is -y).
 *  - the sum's order is part of the rule: partial[l] = the terms with s = l (mod 64) in ascending s, from +0; then 64 -> 1 by halves,
 *    partial[l] += partial[l + 32], then 16, ..., 1. The host forms below evaluate the same text in the same order, so
 *    rt_irradiance_gather_host(rt_query_radiance(rt_irradiance_rays_host(...))) equals the device's answer in every bit.
 *  - with `progressive` every output float but the alpha is old * (1 - w) + new * w, w = 1 / ((float)frameCount + 1).
 *  - a point's answer depends on (position, normal, pid, params, env, scene) only: not on n, its place in the batch, or the chunks.
 * The batch runs in chunks of whole points, as many as keep chunk x S within one radiance piece ("radiance_max_kslots" x 1024
 * rays; by default what "frames_max_mslots" allows): k_irradiance_rays<SPHERE> writes the chunk's rays into a ctx buffer (44 bytes
 * per ray: origin, direction, id, radiance record), the radiance pipeline runs them as rt_query_radiance would, and
 * k_irradiance_gather<SPHERE> sums, one wave per point. The struct, the params and env are read on the host. With the plain
 * names the arrays, d_ids and d_out (16-byte aligned for the irradiance form) are device pointers and the call is asynchronous on
 * the ctx stream: the arrays stay valid and unchanged until the stream has passed it. The _host names take host arrays, stage
 * them through a ctx buffer and block.
 * The pass changes nothing a later render or query produces or chooses: not the ctx framebuffer or its progressive history, not
 * rt_last_pipeline, rt_last_parts or rt_ray_cost. Its counters go to the AOV passes' block (paths grows by n x S). rt_last_kernel
 * names the traversal kernel that ran.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch or NULL params; (n == 0 succeeds here
 * and does nothing;) points, normals (irradiance form) or the output NULL; samples 0 or >= 2^24; bounceLimit >= 2^28 - 1; bias
 * not finite or < 0; samples above the rays of one piece; n >= 2^30. */
int  rt_query_irradiance(rt_ctx* ctx, const RtPointNormalBatch* d_batch, const uint32_t* d_ids, const RtIrradianceParams* params,
                         const EnvironmentData* env, float* d_out);
int  rt_query_irradiance_host(rt_ctx* ctx, const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params,
                              const EnvironmentData* env, float* out);
int  rt_query_sh_probes(rt_ctx* ctx, const RtPointNormalBatch* d_batch, const uint32_t* d_ids, const RtIrradianceParams* params,
                        const EnvironmentData* env, float* d_out);
int  rt_query_sh_probes_host(rt_ctx* ctx, const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params,
                             const EnvironmentData* env, float* out);
/* The host forms of the rule: no ctx, no GPU. `sphere` != 0: the probe form. rt_irradiance_rays_host: the rays of points
 * [first, first + count) of the batch, ray (i - first) * S + s at origins / dirs [3 ray ..] and rayIds[ray] (count x S of each).
 * rt_irradiance_gather_host: radiance holds 4 floats per ray of the whole batch (ray i * S + s), out 4 n or 27 n floats, read as
 * the previous result when `progressive`; the probe form reads no array of the batch. -1: a NULL argument, samples 0 or
 * >= 2^24, a bias that is not finite or < 0, first + count > n. */
int  rt_irradiance_rays_host(const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params, int sphere,
                             uint32_t first, uint32_t count, float* origins, float* dirs, uint32_t* rayIds);
int  rt_irradiance_gather_host(const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params, int sphere,
                               const float* radiance, float* out);

/* Lightmap texels ("Lightmap texels"; include/rt_texels.h states the rule, both sides compile it): the surface point
 * and shading normal behind every texel of a W x H map laid over one object's uv layout, the batch rt_query_irradiance takes, the
 * way back into the map, and gutter texels around the charts. */
typedef struct RtTexel {
    float point[3];  uint32_t state;     /* world position; state: 0 empty, 1 covered, 3 covered and overlapped */
    float normal[3]; uint32_t triIndex;  /* the shading normal; the owner, as RtHit.triHitIndex numbers triangles */
    float uv[2];     uint32_t _pad[2];   /* the owner's barycentrics (u, v) at the texel's centre; 0 */
} RtTexel;                               /* 48 bytes, three 16-byte stores; an empty record is all 0 */
typedef struct RtTexelStats {
    uint32_t covered;           /* records with state != 0 */
    uint32_t overlapped;        /* records with state == 3 */
    uint32_t skippedTriangles;  /* triangles of the object that cover nothing by the rule: a uv that is not finite, |X| or |Y| >= 2^27, area 0 */
    uint32_t degenerateTexels;  /* texels whose owner gives no finite normal: left empty */
} RtTexelStats;
/* Contract (the rule in full: include/rt_texels.h).
 *  - The map is width x height, each 1 .. 8192, rows top to bottom; record y * width + x is texel (x, y), whose centre is
 *    u = (x + 0.5) / W, v = 1 - (y + 0.5) / H: the texel rt_tex_index(u, W), rt_tex_index(1 - v, H) picks for that uv.
 *  - Coverage in exact integers on a grid of 256 sub-texels: a uv corner snaps to X = rint(u * 256 W), Y = rint((1 - v) * 256 H) in
 *    doubles, ties to even; a centre (256 x + 128, 256 y + 128) is covered by a triangle when its three edge functions, normalised to
 *    the winding that makes the doubled area A positive, are > 0, or == 0 on a top or left edge. Either winding works; a centre on
 *    an edge two triangles share belongs to exactly one of them. Triangles with a uv that is not finite, |X| or |Y| >= 2^27, or A = 0
 *    are skipped and counted.
 *  - The owner is the lowest triangle index that covers the centre, `overlapped` (state 3) when two or more do: functions of the
 *    scene alone.
 *  - uv = (u, v) = ((float)(E1 / A), (float)(E2 / A)) in doubles, w = (1 - u) - v; point = rt_bary_point of the world corners as
 *    rt_query_nearest places them; normal = rt_normalize(fwd x ((n0 w + n1 u) + n2 v)), reconstruct_hit's for a front-face hit
 *    without the bump map; where that is not finite the normalised world face normal on the side of the vertex normals' sum; where
 *    that is not finite either the texel stays empty and is counted in degenerateTexels.
 * rt_bake_texels: d_texels is device memory, 16-byte aligned, 48 bytes per texel; asynchronous on the ctx stream, except that a
 * statsOut (host memory) makes the call wait for them. Kernels: k_texel_bins (one lane per triangle: the 8 x 8-texel blocks its
 * box touches), an exclusive scan, k_texel_cover (one wave per (triangle, block), one lane per texel, atomicMin on an owner plane
 * in ctx scratch), k_texel_resolve (one lane per texel: the record). rt_bake_texels_host: host memory, blocks. They read the
 * scene tables as they are (after rt_update_objects and rt_update_points too) and change nothing a later render or query
 * produces or chooses. rt_texels_exhaustive_host: the same rule in plain loops over the host arrays, no ctx, no GPU; -1: a NULL
 * argument, an object, a size or indices out of range, or a mesh whose triangles are not one contiguous range.
 * rt_texels_compact: the covered texels in ascending texel index (by a scan, not by atomics) as packed points and normals
 * (RtPointNormalBatch's layout) and d_index[j] = y * W + x, which rt_query_irradiance takes as ids, so a texel's light depends on
 * its place in the map and never on which other texels are covered; d_countOut[0] (device) = how many. Each array holds nTexels
 * entries' worth.
 * rt_texels_scatter: d_rgba[d_index[j]] = d_values4[j] (4 floats) and d_fill[d_index[j]] = 1 for j < nCovered; every other texel
 * (0, 0, 0, 0) and fill 0.
 * rt_dilate_texels: `passes` (<= 254) passes in ping-pong through a ctx plane; pass k (from 1): a texel with fill 0 and at least
 * one 8-neighbour (no wrap) with fill != 0 gets the sum of those neighbours' rgb, in the order (-1,-1), (0,-1), (1,-1), (-1,0),
 * (1,0), (-1,1), (0,1), (1,1) from +0, divided by (float)count, alpha 0, fill 1 + k. rt_dilate_texels_host: the same, host memory,
 * no ctx, no GPU; -1: a NULL plane, a size out of range, passes > 254.
 * rt_bake_lightmap: rt_bake_texels, rt_texels_compact, rt_query_irradiance(ids = index), rt_texels_scatter, rt_dilate_texels,
 * in that order through ctx scratch, equal to the composition by hand in every bit; d_rgba (16-byte aligned, 16 bytes per texel)
 * and d_fill (1 byte per texel) are device memory. It waits once, for the count of covered texels. One shot: params->progressive
 * != 0 is refused.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL output; object >= the object count; width or
 * height 0 or > 8192; an object whose mesh's triangles are not one contiguous range; then, for rt_bake_lightmap, NULL params,
 * progressive, dilatePasses > 254 and rt_query_irradiance's own refusals. rt_texels_compact / _scatter / rt_dilate_texels refuse
 * NULL arrays and nTexels (width x height) 0 or > 8192 x 8192, nCovered > nTexels, passes > 254. */
int  rt_bake_texels(rt_ctx* ctx, uint32_t object, uint32_t width, uint32_t height, RtTexel* d_texels, RtTexelStats* statsOut);
int  rt_bake_texels_host(rt_ctx* ctx, uint32_t object, uint32_t width, uint32_t height, RtTexel* texels, RtTexelStats* stats);
int  rt_texels_exhaustive_host(const RtSceneArrays* scene, uint32_t object, uint32_t width, uint32_t height, RtTexel* texels, RtTexelStats* stats);
int  rt_texels_compact(rt_ctx* ctx, uint32_t nTexels, const RtTexel* d_texels, float* d_points, float* d_normals, uint32_t* d_index, uint32_t* d_countOut);
int  rt_texels_scatter(rt_ctx* ctx, uint32_t nTexels, uint32_t nCovered, const uint32_t* d_index, const float* d_values4, float* d_rgba, uint8_t* d_fill);
int  rt_dilate_texels(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t passes, float* d_rgba, uint8_t* d_fill);
int  rt_dilate_texels_host(uint32_t width, uint32_t height, uint32_t passes, float* rgba, uint8_t* fill);
int  rt_bake_lightmap(rt_ctx* ctx, uint32_t object, uint32_t width, uint32_t height, const RtIrradianceParams* params, const EnvironmentData* env,
                      uint32_t dilatePasses, float* d_rgba, uint8_t* d_fill, RtTexelStats* statsOut);

/* Point queries ("Point queries"): how far each of the caller's points is from the scene, and where the nearest surface
 * is. The search is not a ray's: a best-first descent pruned by box distance, in a kernel of its own (k_nearest_points) over the
 * tables the scene already has on the device. */
typedef struct RtPointBatch {
    const float* points;   /* n x 3 floats, packed */
    const float* maxDist;  /* n floats, or NULL: no limit */
    uint32_t n;
} RtPointBatch;
typedef struct RtNearest {
    float dst;              /* world distance; RT_MISS_DST when found == 0 */
    uint32_t found, isSphere;
    uint32_t objectIndex;   /* object, or sphere index when isSphere */
    uint32_t triIndex;      /* as RtHit.triHitIndex numbers triangles */
    float uv[2];            /* barycentrics of the point on that triangle; 0 for a sphere */
    float point[3];         /* the closest point, world space */
    uint32_t _pad[2];       /* 0: the record is 48 bytes, three 16-byte stores */
} RtNearest;                /* not found: dst = RT_MISS_DST, everything else 0 */
/* Contract (include/rt_point_query.h states the rule; both sides compile it). The scene's surfaces are every sphere with
 * radius > 0 (the sphere table's zeroed slots are none) and every triangle of every object, its corners placed in fp32 by the
 * object's forward matrix (rt_xform_point; an identity object's corners are used as they are). Distances are Euclidean in world
 * space whatever the object's scale or shear; frontOnly, materials and alpha maps play no part. Point i with limit T (maxDist[i];
 * none when maxDist is NULL) keeps a bound best2 started at fl(T * T) (+inf without a limit); a primitive whose squared distance
 * (rt_point_sphere, rt_point_triangle) is strictly less than best2 replaces the answer; found = 1 when one did and
 * dst = rt_sqrt(best2). A limit that is NaN or <= 0 gives the not-found record without a search.
 *  - dst and found do not depend on the order primitives are visited in, nor on the BVH: rt_query_nearest equals
 *    rt_nearest_exhaustive_host in both, bit for bit (the traversal discards a subtree only where the derivation in DESIGN.md
 *    shows that it cannot hold a nearer primitive).
 *  - Which primitive is reported where several are equally near in fp32 (a closest point on a shared edge or vertex) depends on
 *    the order: it is a minimiser, not a particular one; point and uv belong to the one reported (point = w a + u b + v c of
 *    its world corners, w = (1 - u) - v).
 * rt_query_nearest: the struct is read on the host, its arrays and d_out are device pointers, asynchronous on the ctx stream (the
 * arrays stay valid and unchanged until the stream has passed it). rt_query_nearest_host takes host arrays, stages them through a
 * ctx buffer and blocks. One lane per point, no path state. rt_last_kernel names the instantiation that ran: k_nearest_points<24,
 * true> while the scene's deepest BVH leaf is at most 24 levels down, k_nearest_points<64, false> beyond (a scene deeper than
 * that is refused). The pass adds to the AOV passes' counter block: boxTests (box distances evaluated), triTests
 * (rt_point_triangle calls), raysTraced (points searched), raysHit (points found), and changes nothing a later rt_render,
 * rt_render_aovs, rt_denoise, rt_temporal_accumulate or ray query produces or chooses. It reads the tables of the scene as they
 * are: after rt_update_objects or rt_update_points, the moved and the refit ones.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; points or the output NULL with n > 0;
 * n >= 2^30. n == 0 succeeds and does nothing.
 * rt_nearest_exhaustive_host: the same rule in a plain loop over the host arrays: every sphere in index order, then every triangle
 * of every object in index order, no pruning; no ctx, no GPU (the BVH only says which triangles an object has). -1: a NULL
 * argument, n >= 2^30, or arrays that index out of range. */
int  rt_query_nearest(rt_ctx* ctx, const RtPointBatch* d_points, RtNearest* d_out);
int  rt_query_nearest_host(rt_ctx* ctx, const RtPointBatch* points, RtNearest* out);
int  rt_nearest_exhaustive_host(const RtSceneArrays* scene, const RtPointBatch* points, RtNearest* out);

/* Signed point queries ("Signed point queries"; include/rt_point_side.h states the rule, both sides compile it): the
 * record of rt_query_nearest, bit for bit, and one byte side[i]: +1 outside, -1 inside, 0 unknown or nothing found.
 *  - A sphere: l = |q - c| as rt_point_sphere computes it: +1 when l > r, -1 when l < r, 0 when l == r.
 *  - A triangle: relative to the closed COMPONENT the reported triangle belongs to: the triangles of one mesh connected through
 *    shared edges, after the mesh's points are welded by equal position (equal float values: -0 == +0, NaN welds with nothing).
 *    A component is signable when every edge of it is shared by exactly two non-degenerate triangles, it is orientable and its
 *    signed volume in object space is not zero. Orientation is repaired, never the geometry: a walk over the edges winds each
 *    signable component consistently and then so that its volume is positive (normals outward); a triangle whose stored winding
 *    disagrees carries a FLIP bit. Cavities (inner shells) are not modelled, overlapping solids are not a union: the sign is
 *    relative to the nearest component alone.
 *  - side = sign(dot(q - p, N)) x the object's orientation (+1, or -1 when det(fwd 3x3) < 0), p = rt_bary_point(a, b, c, u, v),
 *    N the angle-weighted pseudo-normal (Baerentzen and Aanaes) of the feature p lies on (rt_point_triangle_feature): the face's
 *    normal, the sum of the two unit face normals at an edge, the sum of corner angle x unit face normal over the fan of a vertex;
 *    normals and angles from the world corners rt_xform_point(fwd, v) in fp32, as the nearest kernel places them.
 *  - 0 for: a component that is not signable (open quads, non-manifold or non-orientable meshes); a degenerate triangle; a vertex
 *    whose fan is not one closed cycle of at most RT_SIDE_MAX_FAN triangles; a matrix with a zero or non-finite determinant;
 *    a pseudo-normal that is not finite; a dot product of exactly 0.
 * rt_scene_topology: per object (the first nObjects) the statistics of its mesh's table and its orientation; no ctx, no GPU.
 * -1: a NULL argument, 2^30 triangles or more, or arrays that index out of range.
 * rt_nearest_side_host: the rule applied to GIVEN records in a plain loop, no ctx, no GPU: fed rt_query_nearest_signed's own
 * records it reproduces its side byte for byte (the side is a function of the point and the reported record alone). -1: a NULL
 * argument with n > 0, n >= 2^30, a record or arrays that index out of range.
 * rt_upload_topology: builds the table and the per-object orientations from the host arrays of the uploaded scene and uploads
 * them; explicit, so rt_upload_scene keeps its cost. A later rt_upload_scene or rt_upload_scene_dynamic drops them.
 * rt_update_points keeps the table (the topology is kept by contract: the caller keeps coincident points coincident);
 * rt_update_objects keeps it and refreshes the orientations. Refused: before rt_upload_scene; 2^30 triangles or more.
 * rt_query_nearest_signed: rt_query_nearest, then the side pass (k_nearest_side, one lane per point) on the same stream;
 * asynchronous as rt_query_nearest is; d_side is n bytes of device memory. rt_last_kernel names k_nearest_side<256>. The pass adds
 * what rt_query_nearest adds to the AOV passes' counter block and, in its `segments` field (which no ray or point query writes
 * and the ray-cost measurement never reads), the points it gave a sign other than 0. It changes nothing a later render or query
 * produces. Refused with a message, nothing written, in this order: no uploaded scene; "no topology uploaded"; "topology does not
 * match the uploaded scene" (the object, triangle or node counts differ); a NULL batch; points, the output or side NULL with
 * n > 0; n >= 2^30. n == 0 succeeds and does nothing. rt_query_nearest_signed_host takes host arrays and blocks. */
/* (RT_SIDE_MAX_FAN is 256: include/rt_point_side.h) */
typedef struct RtMeshTopology {
    uint32_t triangles;            /* of the object's mesh */
    uint32_t weldedVertices;       /* distinct positions among the points its triangles use */
    uint32_t components;           /* edge-connected sets of non-degenerate triangles */
    uint32_t signableComponents;
    uint32_t signableTriangles;
    uint32_t boundaryEdges;        /* edges with one triangle */
    uint32_t nonManifoldEdges;     /* edges with three or more */
    uint32_t flippedTriangles;     /* FLIP bits among the signable triangles */
    uint32_t degenerateTriangles;
    int32_t orientation;           /* +1, -1, or 0: the sign of det(transformMatrix 3x3); 0 when it is zero or not finite */
} RtMeshTopology;
int  rt_scene_topology(const RtSceneArrays* scene, RtMeshTopology* out, uint32_t nObjects);
int  rt_nearest_side_host(const RtSceneArrays* scene, const RtPointBatch* points, const RtNearest* recs, int8_t* side);
/* the same loop, and beside side what the rule met (either array may be NULL): feature[i], the region code of
 * rt_point_triangle_feature (0 face, 1-3 vertices a b c, 4-6 edges ab ac bc; 255: a sphere, nothing found, or a triangle the rule
 * left unsigned before classifying it), and fan[i], the triangles walked around a vertex (0 otherwise). For measurements. */
int  rt_nearest_side_features_host(const RtSceneArrays* scene, const RtPointBatch* points, const RtNearest* recs, int8_t* side,
                                   uint8_t* feature, uint16_t* fan);
int  rt_upload_topology(rt_ctx* ctx, const RtSceneArrays* scene);
int  rt_query_nearest_signed(rt_ctx* ctx, const RtPointBatch* d_points, RtNearest* d_out, int8_t* d_side);
int  rt_query_nearest_signed_host(rt_ctx* ctx, const RtPointBatch* points, RtNearest* out, int8_t* side);

/* Radius point queries ("Radius point queries"; include/rt_point_within.h states the rule, both sides compile it): every
 * surface within reach of a point, the first k of them nearest first, and how many there are: the point side's counterpart of
 * rt_query_hits.
 * Contract. Point i has the reach R (maxDist[i]; none when maxDist is NULL: every surface is a member) and the bound
 * R2 = rt_nearest_start(...), the very function rt_query_nearest starts with: fl(R * R), or +inf without a reach. A reach that
 * is NaN or <= 0 means no search. Its member set C:
 *  - every sphere with rt_sphere_is_surface(r) whose rt_point_sphere squared distance is STRICTLY < R2;
 *  - every triangle of every object whose rt_point_triangle squared distance is < R2, its world corners placed through the
 *    forward matrix in fp32 exactly as rt_query_nearest places them.
 * Nothing else plays a part: no frontOnly, no materials, no alpha maps. R2 never shrinks, so C is a function of the point and the
 * scene alone: not of the visiting order, the BVH, the kernel, the stack or any knob.
 *  - d_counts[i] = |C|, exact whatever k is.
 *  - d_out[i * k .. i * k + k - 1]: the first min(k, |C|) members in ascending order of the key, then the not-found record
 *    (dst == RT_MISS_DST, everything else 0) in the remaining slots. The key, compared lexicographically: the squared distance as
 *    an fp32 compare; spheres before triangles; the lower sphere or object index; the lower triangle index (rt_hits_before of
 *    include/rt_ray_hits.h on {d2, primitive word, triangle}).
 *  - A member's record is an RtNearest with found = 1, dst = rt_sqrt(d2), and uv, point and the indices exactly as
 *    rt_query_nearest builds them for that primitive; 48 bytes, padding 0.
 *  - The key is total, so unlike rt_query_nearest the reported primitives are particular ones, and rt_query_within equals
 *    rt_within_exhaustive_host in every byte of every record and count.
 *  - Hence, bit for bit: counts[i] > 0 iff rt_query_nearest with maxDist = R has found; out[i * k].dst has the bits of its dst;
 *    the primitive it reports is a member and, with count <= k, is in the list with its record byte for byte; counts are the same
 *    for every k; the list at a smaller k is the head of the list at a larger one; for R1 < R2 the list at R1 is the prefix of the
 *    list at R2 whose squared distances are < fl(R1 * R1).
 *  - k runs from 0 to RT_WITHIN_MAX_K. k == 0: counts only, d_out may be NULL. n == 0 succeeds and does nothing.
 * rt_query_within: the struct is read on the host, its arrays, d_out (16-byte aligned) and d_counts are device pointers,
 * asynchronous on the ctx stream (the arrays stay valid and unchanged until the stream has passed it). rt_query_within_host takes
 * host arrays, stages them through a ctx buffer and blocks. One lane per point, no path state: the search (k_points_within,
 * pruned as k_nearest_points prunes, with the bound held constant) and, with k > 0, a resolve pass of one lane per slot
 * (k_points_within_resolve). rt_last_kernel names the search that ran: k_points_within<24, false> while the scene's deepest BVH
 * leaf is at most 24 levels down, k_points_within<64, true> beyond (its lists live in a ctx buffer instead of LDS; a scene deeper
 * than 64 is refused). The pass adds to the AOV passes' counter block: boxTests (box distances evaluated), triTests
 * (rt_point_triangle calls), raysTraced (points searched), raysHit (points with count > 0), and changes nothing a later render
 * or query produces or chooses. It reads the tables of the scene as they are: after rt_update_objects or rt_update_points, the
 * moved and the refit ones.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; (n == 0 succeeds here;) points NULL
 * ("points and the output are required"); k > RT_WITHIN_MAX_K; d_counts NULL, or d_out NULL with k > 0 ("counts and, with k > 0,
 * the output are required"); n >= 2^30.
 * rt_within_exhaustive_host: the definition as a plain loop over the host arrays: every sphere in index order, then every
 * triangle of every object in index order, no pruning; no ctx, no GPU. -1: what rt_nearest_exhaustive_host refuses, and
 * k > RT_WITHIN_MAX_K. */
#define RT_WITHIN_MAX_K 8
int  rt_query_within(rt_ctx* ctx, const RtPointBatch* d_points, uint32_t k, RtNearest* d_out, uint32_t* d_counts);
int  rt_query_within_host(rt_ctx* ctx, const RtPointBatch* points, uint32_t k, RtNearest* out, uint32_t* counts);
int  rt_within_exhaustive_host(const RtSceneArrays* scene, const RtPointBatch* points, uint32_t k, RtNearest* out, uint32_t* counts);

/* Box queries ("Box queries"; include/rt_box_overlap.h states the rule, both sides compile it): every surface that an
 * axis-aligned box touches, the first k of them in index order, and how many there are: voxelisation, broad-phase candidates,
 * selection by a volume.
 * Contract. Box i is [lo[3 i .. 3 i + 2], hi[3 i .. 3 i + 2]], closed. It is valid when its six numbers are finite and lo <= hi on
 * every axis; flat and point boxes are valid. Any other box is not searched: count 0, empty records, not counted in raysTraced.
 * The surfaces are rt_query_nearest's: every sphere with rt_sphere_is_surface(r), and every triangle of every object, its world
 * corners rt_xform_point(fwd, v) in fp32 (an identity object's corners as they are). No frontOnly, no materials, no alpha maps.
 * Touching counts: every "separated" decision is a strict inequality, an axis that comes out zero separates nothing, and a
 * comparison with a NaN operand is false. The member set C of a valid box:
 *  - every triangle that rt_box_triangle keeps: the 13-axis separating-axis test in a fixed order: the three box axes by
 *    comparisons alone (out when max(a_i, b_i, c_i) < lo_i or min(a_i, b_i, c_i) > hi_i; exact); then, with the centre
 *    fl(lo 0.5 + hi 0.5), the half-extent fl(hi 0.5 - lo 0.5) and the corners relative to the centre, the plane axis e0 x e1; then
 *    the nine axes e_j x unit_i, each a two-term projection against h . |axis|. A triangle with two equal corners is its segment,
 *    with three its point;
 *  - every sphere that rt_box_sphere keeps: the surface is the shell: d2min <= fl(r r) <= d2max, d2min = rt_point_box2(centre,
 *    lo, hi), d2max the squared distance to the farthest corner summed in x, y, z order. A box wholly inside a ball is no member.
 * C is a function of the box and the scene alone: not of the visiting order, the BVH, the kernel, the stack or any knob.
 *  - d_counts[i] = |C|, exact whatever k is.
 *  - d_out[i * k .. i * k + k - 1]: the first min(k, |C|) members in ascending order of the key, then empty records (all 0). The
 *    key: spheres before triangles; the lower sphere or object index; the lower triangle index (rt_hits_before of
 *    include/rt_ray_hits.h with a constant first word). A member's record: found = 1, isSphere, objectIndex (the sphere's or
 *    the object's index), triIndex (0 for a sphere).
 *  - The key is total, so rt_query_boxes equals rt_boxes_exhaustive_host in every byte of every record and count. Counts are the
 *    same for every k, and the list at a smaller k is the head of the list at a larger one.
 *  - k runs from 0 to RT_BOXES_MAX_K; the count says when a box must be subdivided. k == 0: counts only, d_out may be NULL.
 *    n == 0 succeeds and does nothing.
 * rt_query_boxes: the struct is read on the host, its arrays, d_out (16-byte aligned) and d_counts are device pointers,
 * asynchronous on the ctx stream (the arrays stay valid and unchanged until the stream has passed it). rt_query_boxes_host takes
 * host arrays, stages its four parts through a ctx buffer and blocks. One lane per box, no path state, one kernel
 * (k_boxes_overlap; it writes the records itself): the descent discards a subtree by box-against-box overlap only, exact for an
 * identity object and padded by a derived multiple of the rounding unit for a placed one. rt_last_kernel names the search that
 * ran: k_boxes_overlap<24, false> while the scene's deepest BVH leaf is at most 24 levels down, k_boxes_overlap<64, true> beyond
 * (its lists live in a ctx buffer instead of LDS; a scene deeper than 64 is refused). The pass adds to the AOV passes' counter
 * block: boxTests (box-against-box tests, the object boxes among them), triTests (rt_box_triangle calls), raysTraced (boxes
 * searched), raysHit (boxes with count > 0), and changes nothing a later render or query produces or chooses. It reads the tables
 * of the scene as they are: after rt_update_objects or rt_update_points, the moved and the refit ones.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; (n == 0 succeeds here;) lo or hi NULL
 * ("lo and hi are required"); k > RT_BOXES_MAX_K; d_counts NULL, or d_out NULL with k > 0 ("counts and, with k > 0, the output
 * are required"); n >= 2^30.
 * rt_boxes_exhaustive_host: the definition as a plain loop over the host arrays: every sphere in index order, then every
 * triangle of every object in index order, no pruning; no ctx, no GPU. -1: what rt_within_exhaustive_host refuses. */
typedef struct RtBoxBatch {
    const float* lo;   /* n x 3, packed */
    const float* hi;   /* n x 3, packed */
    uint32_t n;
} RtBoxBatch;
typedef struct RtOverlap { uint32_t found, isSphere, objectIndex, triIndex; } RtOverlap;   /* 16 bytes, one 16-byte store; no member: all 0 */
#define RT_BOXES_MAX_K 8
int  rt_query_boxes(rt_ctx* ctx, const RtBoxBatch* d_boxes, uint32_t k, RtOverlap* d_out, uint32_t* d_counts);
int  rt_query_boxes_host(rt_ctx* ctx, const RtBoxBatch* boxes, uint32_t k, RtOverlap* out, uint32_t* counts);
int  rt_boxes_exhaustive_host(const RtSceneArrays* scene, const RtBoxBatch* boxes, uint32_t k, RtOverlap* out, uint32_t* counts);

/* Oriented box queries ("Oriented box queries"; include/rt_obb_overlap.h states the rule, both sides compile it): the
 * box queries for a box placed by a frame: an overlap box with a rotation, a link's bounding box, a selection volume aligned
 * with an object or a camera, the cells of a grid in an object's own coordinates.
 * Contract. Box i is the set { p : lo_i <= F_i p <= hi_i }, closed. F_i is the world-to-box frame: sixteen floats in
 * RenderObject.transformMatrix's layout (column-major), frames[16 i ..], or frames[0 .. 15] for every box when sharedFrame is 1
 * (a grid in one frame). F p is rt_xform_point(F, p) of include/rt_det_math.h in fp32; it reads twelve of the sixteen floats,
 * the other four (m[3], m[7], m[11], m[15]) are never read. A frame and a local box, not a centre, axes and half-extents: the
 * rule needs no inverse, an object's inverse matrix can be passed as it is (the box is then in object coordinates), and the
 * cells of a grid in one frame share F and their face values bit for bit. F need not be orthonormal or even invertible: a
 * singular frame is not refused, the rule applies as written.
 * Box i is valid when the twelve frame numbers that are read are finite and lo, hi are a valid box of rt_query_boxes (six finite
 * numbers, lo <= hi). Any other box is not searched: count 0, empty records, not counted in raysTraced.
 * The surfaces are rt_query_nearest's; a triangle's world corners are rt_xform_point(fwd, v) in fp32 (an identity object's as
 * they are). The member set C of a valid box:
 *  - every triangle that rt_box_triangle(lo, hi, F a, F b, F c) keeps: rt_query_boxes' 13-axis rule on the corners taken into the
 *    box's frame (a linear map takes triangles to triangles);
 *  - every sphere that rt_box_sphere(lo, hi, F centre, fl(r s)) keeps, s = rt_sqrt((m[0] m[0] + m[1] m[1]) + m[2] m[2]) the
 *    length of the frame's first column. This is the geometry of the shell exactly when the linear part of F is a rotation or
 *    reflection times a uniform scale; for any other frame it is this formula and no more.
 * C is a function of the box, its frame and the scene alone. Key, records, k from 0 to RT_BOXES_MAX_K, counts exact for every k
 * and the list at a smaller k the head of the list at a larger one: all as rt_query_boxes states them, so
 * rt_query_oriented_boxes equals rt_obbs_exhaustive_host in every byte of every record and count. With an identity frame the
 * frame step is exact (products with 1 and 0, sums with 0), so on scenes with finite corners the answer equals rt_query_boxes'
 * in every byte; sharedFrame = 1 equals the same matrix repeated n times in every byte.
 * rt_query_oriented_boxes: the struct is read on the host, its arrays, d_out (16-byte aligned) and d_counts are device pointers,
 * asynchronous on the ctx stream. rt_query_oriented_boxes_host takes host arrays, stages its five parts (frames, lo, hi, out,
 * counts) through a ctx buffer and blocks. One kernel (k_obbs_overlap; it writes the records itself): the descent discards a
 * subtree only when its box, taken through F (through fl(F M) for a placed object) and padded by a derived multiple of the
 * rounding unit, lies apart from [lo, hi] on one of the box's own axes. rt_last_kernel names the search that ran:
 * k_obbs_overlap<24, false> while the scene's deepest BVH leaf is at most 24 levels down, k_obbs_overlap<64, true> beyond (a
 * scene deeper than 64 is refused). Counters as the box pass: boxTests (projected-box tests, the object boxes among them),
 * triTests (triangle-rule calls), raysTraced (boxes searched), raysHit (boxes with count > 0); nothing a later render or query
 * produces or chooses changes. It reads the tables of the scene as they are after rt_update_objects or rt_update_points.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; (n == 0 succeeds here;) frames, lo or
 * hi NULL ("frames, lo and hi are required"); k > RT_BOXES_MAX_K; sharedFrame > 1 ("sharedFrame = N is neither 0 nor 1");
 * d_counts NULL, or d_out NULL with k > 0; n >= 2^30.
 * rt_obbs_exhaustive_host: the definition as a plain loop over the host arrays: every sphere in index order, then every triangle
 * of every object in index order, no pruning; no ctx, no GPU. -1: what rt_boxes_exhaustive_host refuses, and sharedFrame > 1.
 * rt_object_frames_host: frames[16 i ..] = rt_mat4_inverse of the matrix of object objects[i] of the host arrays: the frame under
 * which lo and hi are in that object's own coordinates. No ctx, no GPU. -1: a NULL argument with n > 0, an index out of range. */
typedef struct RtObbBatch {
    const float* frames;   /* the world-to-box matrices: 16 floats each, RenderObject.transformMatrix's layout (column-major) */
    const float* lo;       /* n x 3, packed: the box in its frame's coordinates */
    const float* hi;       /* n x 3 */
    uint32_t n;
    uint32_t sharedFrame;  /* 0: frames holds n matrices; 1: one matrix for the whole batch (a grid in one frame) */
} RtObbBatch;
int  rt_query_oriented_boxes(rt_ctx* ctx, const RtObbBatch* d_batch, uint32_t k, RtOverlap* d_out, uint32_t* d_counts);
int  rt_query_oriented_boxes_host(rt_ctx* ctx, const RtObbBatch* batch, uint32_t k, RtOverlap* out, uint32_t* counts);
int  rt_obbs_exhaustive_host(const RtSceneArrays* scene, const RtObbBatch* batch, uint32_t k, RtOverlap* out, uint32_t* counts);
int  rt_object_frames_host(const RtSceneArrays* scene, const uint32_t* objects, uint32_t n, float* frames);

/* Triangle queries ("Triangle queries"; include/rt_tri_overlap.h states the rule, both sides compile it): every
 * surface that a caller's triangle touches, the first k of them in index order, and how many there are: the exact narrow phase
 * of a mesh against the scene, for a robot link, a tool, a character or a cloth.
 * Contract. Triangle i is the closed triangle of the corners p = corners[9 i .. 9 i + 2], q = corners[9 i + 3 ..], r =
 * corners[9 i + 6 ..]. It is valid when its nine numbers are finite; equal corners are valid. Any other triangle is not searched:
 * count 0, empty records, not counted in raysTraced. The surfaces are rt_query_nearest's: every sphere with
 * rt_sphere_is_surface(r), as a shell, and every triangle of every object, its world corners rt_xform_point(fwd, v) in fp32 (an
 * identity object's corners as they are). No frontOnly, no materials, no alpha maps. Touching counts: every "separated" decision
 * is a strict inequality, an axis that comes out zero separates nothing, and a comparison with a NaN operand is false. The member
 * set C of a valid triangle:
 *  - every triangle that rt_tri_triangle keeps: a separating-axis test over 17 axes in a fixed order. First the box of p, q, r
 *    against the box of a, b, c by comparisons alone (exact). Then, with all six corners relative to the centre
 *    fl(lo 0.5 + hi 0.5) of the query's box, the query's normal nQ, the triangle's normal nT, the nine eQi x eTj (i outer), the
 *    three nQ x eQi and the three nT x eTj, each by projecting all six corners; the last six decide coplanar pairs. A query with
 *    two or three equal corners is its segment or its point, except in a scene triangle's own plane, where the rule is the
 *    formula and no more;
 *  - every sphere that rt_tri_sphere keeps: d2min <= fl(rad rad) <= d2max, d2min = rt_point_triangle's answer at the centre, d2max
 *    the largest corner distance. A triangle wholly inside a ball is no member.
 * C is a function of the triangle and the scene alone: not of the visiting order, the BVH, the kernel, the stack or any knob.
 *  - d_counts[i] = |C|, exact whatever k is.
 *  - d_out[i * k .. i * k + k - 1]: the first min(k, |C|) members in ascending order of rt_query_boxes' key (spheres before
 *    triangles; the lower sphere or object index; the lower triangle index), then empty records (all 0). Records as rt_query_boxes'.
 *  - The key is total, so rt_query_triangles equals rt_tris_exhaustive_host in every byte of every record and count. Counts are
 *    the same for every k, and the list at a smaller k is the head of the list at a larger one.
 *  - k runs from 0 to RT_BOXES_MAX_K. k == 0: counts only, d_out may be NULL. n == 0 succeeds and does nothing.
 * rt_query_triangles: the struct is read on the host, corners, d_out (16-byte aligned) and d_counts are device pointers,
 * asynchronous on the ctx stream (the arrays stay valid and unchanged until the stream has passed it). rt_query_triangles_host
 * takes host arrays, stages its three parts (corners, out, counts) through a ctx buffer and blocks. One lane per triangle, no
 * path state, one kernel (k_tris_overlap; it writes the records itself): the descent discards a subtree whose box lies apart
 * from the query's box (exact for an identity object, padded for a placed one, as rt_query_boxes) or, "tri_plane" 1
 * (rt_set_tuning; the default), strictly on one side of the query's plane by more than a derived multiple of the rounding unit.
 * rt_last_kernel names the search that ran: k_tris_overlap<24, false> while the scene's deepest BVH leaf is at most 24 levels
 * down, k_tris_overlap<64, true> beyond (its lists live in the box queries' ctx buffer; a scene deeper than 64 is refused). The
 * pass adds to the AOV passes' counter block: boxTests (nodes tested by box and plane, the object boxes among them), triTests
 * (rt_tri_triangle calls), raysTraced (triangles searched), raysHit (triangles with count > 0), and changes nothing a later
 * render or query produces or chooses. It reads the tables of the scene as they are: after rt_update_objects or
 * rt_update_points, the moved and the refit ones.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; (n == 0 succeeds here;) corners NULL
 * ("corners are required"); k > RT_BOXES_MAX_K; d_counts NULL, or d_out NULL with k > 0 ("counts and, with k > 0, the output
 * are required"); n >= 2^30.
 * Not modelled: leaving a mesh's own neighbours out of a self-intersection check (a triangle touches itself and everything that
 * shares a corner with it); k above 8. The segment along which two triangles cross is rt_query_cuts' answer ("Triangle cuts").
 * rt_tris_exhaustive_host: the definition as a plain loop over the host arrays: every sphere in index order, then every
 * triangle of every object in index order, no pruning; no ctx, no GPU. -1: what rt_boxes_exhaustive_host refuses. */
typedef struct RtTriangleBatch {
    const float* corners;   /* n x 9, packed: p, q, r */
    uint32_t n;
} RtTriangleBatch;
int  rt_query_triangles(rt_ctx* ctx, const RtTriangleBatch* d_tris, uint32_t k, RtOverlap* d_out, uint32_t* d_counts);
int  rt_query_triangles_host(rt_ctx* ctx, const RtTriangleBatch* tris, uint32_t k, RtOverlap* out, uint32_t* counts);
int  rt_tris_exhaustive_host(const RtSceneArrays* scene, const RtTriangleBatch* tris, uint32_t k, RtOverlap* out, uint32_t* counts);

/* Triangle cuts ("Triangle cuts"; include/rt_tri_cut.h states the rule, both sides compile it): the segments along
 * which a caller's triangle crosses the triangles of the scene, the first k of them in index order, and how many there are:
 * intersection curves of a tool, a link or a cloth against the scene, contour lines of a cut surface, trim curves, contact lines.
 * Contract. The batch is rt_query_triangles', and so is what makes a triangle valid; a triangle that is not valid is not
 * searched: count 0, empty records, not counted in raysTraced. The surfaces are the scene's triangles as rt_query_triangles
 * places them. Spheres are never members (a circle arc is not a segment). A scene triangle is a member of query i when
 * rt_tri_cut_prepared gives the pair a cut:
 *  - the pair passes rt_tri_triangle_prepared, so every cut member is a member of rt_query_triangles, under the same key;
 *  - with all corners relative to the centre of the query's box, each triangle has candidate points on the other's plane: where
 *    an edge whose ends have heights of strictly opposite sign crosses it, lo + (hi - lo) (s_lo / (s_lo - s_hi)) with the edge's
 *    ends in the order of their coordinates (x, y, z), not of the winding, and every corner whose height is exactly 0. Three
 *    heights of 0: the pair is coplanar and has no cut. A query with two or three equal corners has no normal, is coplanar with
 *    everything, and has count 0;
 *  - on the common line nQ x nT each triangle's candidates span an interval; no cut if either has no candidate or the intervals
 *    are strictly apart; else a is the candidate of the larger lower end and b that of the smaller upper end, the query's on
 *    equal projections, then the lower edge index;
 *  - a, b in world coordinates fl(X + m); featA, featB: 0..2 the query's edge (p q, q r, r p) the end lies on, 3..5 the scene
 *    triangle's (for a corner, the edge that starts at it). A cut with a non-finite number is no member; a cut of length zero
 *    (a == b, bit for bit: the triangles touch in a point) is.
 * The end on an edge shared by two scene triangles is the same bits in both cuts, whatever their windings, so the cuts of one
 * query chain into polylines by comparing bits. (Not across queries: m differs.) The member set is a function of the triangle
 * and the scene alone.
 *  - d_counts[i]: the number of cuts, exact whatever k is.
 *  - d_out[i * k .. i * k + k - 1]: the first min(k, count) cuts in ascending order of rt_query_boxes' key (object index, then
 *    triangle index), then empty records (all 0). found = 1, objectIndex, triIndex as RtOverlap's, reserved = 0.
 *  - rt_query_cuts equals rt_cuts_exhaustive_host in every byte of every record and count. Counts are the same for every k, and
 *    the list at a smaller k is the head of the list at a larger one.
 *  - k runs from 0 to RT_BOXES_MAX_K. k == 0: counts only, d_out may be NULL. n == 0 succeeds and does nothing.
 * rt_query_cuts: the struct is read on the host, corners, d_out (16-byte aligned) and d_counts are device pointers, asynchronous
 * on the ctx stream. rt_query_cuts_host takes host arrays, stages its three parts (corners, out, counts) and blocks. One lane per
 * triangle, one kernel: k_tris_cut runs rt_query_triangles' descent with both of its prunings ("tri_plane" switches the plane's
 * here as there), keeps keys only, and after the search computes the kept cuts again and writes each record with three 16-byte
 * stores. rt_last_kernel names the search that ran: k_tris_cut<24, false> or k_tris_cut<64, true>, chosen as k_tris_overlap's.
 * Counters as the triangle pass counts them: boxTests, triTests (rule calls), raysTraced (triangles searched), raysHit (triangles
 * with a cut). Refused exactly as rt_query_triangles refuses, in its order and words, under these functions' names.
 * Not modelled: arcs on spheres; the overlap polygon of a coplanar pair; leaving out a mesh's own neighbours (point cuts at shared
 * corners are reported; callers filter); k above 8 (the count says when to subdivide).
 * rt_cuts_exhaustive_host: the definition as a plain loop: every triangle of every object in index order, no pruning; no ctx, no
 * GPU. -1: what rt_tris_exhaustive_host refuses. */
typedef struct RtCut {            /* 48 bytes, three 16-byte stores; no member: all 0 */
    float a[3]; uint32_t featA;   /* one end, world coordinates; the edge it lies on */
    float b[3]; uint32_t featB;   /* the other end */
    uint32_t found, objectIndex, triIndex, reserved;   /* reserved = 0 */
} RtCut;
int  rt_query_cuts(rt_ctx* ctx, const RtTriangleBatch* d_tris, uint32_t k, RtCut* d_out, uint32_t* d_counts);
int  rt_query_cuts_host(rt_ctx* ctx, const RtTriangleBatch* tris, uint32_t k, RtCut* out, uint32_t* counts);
int  rt_cuts_exhaustive_host(const RtSceneArrays* scene, const RtTriangleBatch* tris, uint32_t k, RtCut* out, uint32_t* counts);

/* Sphere sweeps ("Sphere sweeps"; include/rt_sweep.h states the rule, both sides compile it): a ball of radius
 * radius[i] whose centre moves along origins[i] + t dirs[i]; does it touch the scene, when and where? Sphere casts, thick rays,
 * continuous collision, the clearance of a path.
 * Contract. The surfaces are rt_query_nearest's: every sphere with rt_sphere_is_surface(r), every triangle of every object, its
 * world corners placed through the forward matrix in fp32 exactly as rt_query_nearest places them. Surfaces, not solids: a sweep
 * that starts inside a closed mesh or a scene sphere without touching it meets the surface from inside (for a scene sphere of
 * radius r > R, the shell r - R). frontOnly, materials and alpha maps play no part. dirs are not renormalised: t is in units of
 * |dir|, as in the ray queries. Ray i asks for the least t in [0, T) at which the centre is within R of a surface, T = tmax[i],
 * +inf when tmax is NULL. No search, and the not-found record, when the radius is NaN, infinite or <= 0, the limit NaN or <= 0,
 * or dot(d, d) not finite or not > 0.
 *  - Per primitive the rule gives one time or none (the slab of the triangle's plane, its vertex balls and edge cylinders; the
 *    balls r + R and r - R of a sphere), every quadratic solved about the point of the line nearest the primitive, and a time
 *    counts only when the point queries' own distance from the centre fl(o + t d) to that primitive is <= fl((R + sigma)^2),
 *    sigma = RT_SWEEP_SIGMA (48 x 2^-24) x the largest |coordinate| of the centre, the primitive and the step t d.
 *  - The answer is the primitive with the least key {t, spheres before triangles, the lower sphere or object index, the lower
 *    triangle index} (rt_hits_before) among those with t < T. The key is total and the device's pruning conservative by
 *    derivation, so rt_query_sweep equals rt_sweep_exhaustive_host in every byte of every record, whatever the BVH, the kernel
 *    or the visiting order.
 *  - The record: t; the primitive as in RtNearest; uv, point and gap (rt_sqrt of the squared distance) exactly as the point
 *    queries measure that primitive from the centre fl(o + t d), so rt_query_nearest at that centre returns dst <= gap;
 *    normal = normalize(centre - point), -normalize(dir) where they coincide; startsInContact = 1 when t == 0.
 *  - A sweep that starts in contact reports t = 0 and the lowest-keyed primitive it touches, not the nearest or the deepest:
 *    rt_query_nearest at the origin answers that.
 * rt_query_sweep: the struct is read on the host, its arrays and d_out (16-byte aligned) are device pointers, asynchronous on
 * the ctx stream. rt_query_sweep_host takes host arrays, stages them through a ctx buffer and blocks. One lane per ray, no path
 * state. rt_last_kernel names the instantiation that ran: k_sweep_spheres<24, true> while the scene's deepest BVH leaf is at most
 * 24 levels down, k_sweep_spheres<64, false> beyond (a scene deeper than 64 is refused). The pass adds to the AOV passes'
 * counter block: boxTests (grown boxes tested), triTests (calls of the triangle rule), raysTraced (rays searched), raysHit (rays
 * found), and changes nothing a later render or query produces or chooses. It reads the tables of the scene as they are: after
 * rt_update_objects or rt_update_points, the moved and the refit ones.
 * Refused with a message, nothing written, in this order: no uploaded scene; a NULL batch; (n == 0 succeeds here and does
 * nothing;) origins, dirs, radius or the output NULL; n >= 2^30.
 * rt_sweep_exhaustive_host: the definition as a plain loop over the host arrays: every sphere in index order, then every triangle
 * of every object in index order, no pruning; no ctx, no GPU. -1: what rt_nearest_exhaustive_host refuses. */
typedef struct RtSweepBatch {
    const float* origins;  /* n x 3, packed: the centre at t = 0 */
    const float* dirs;     /* n x 3; not renormalised: t is in units of |dir| */
    const float* radius;   /* n floats, required */
    const float* tmax;     /* n floats, or NULL: no limit */
    uint32_t n;
} RtSweepBatch;
typedef struct RtSweep {           /* 64 bytes, four 16-byte stores, output 16-byte aligned */
    float t;                       /* RT_MISS_DST when found == 0 */
    uint32_t found, isSphere, objectIndex;
    uint32_t triIndex; float uv[2]; float gap;   /* gap: distance from the centre at t to the surface, as the rule measured it */
    float point[3];                /* the contact point on the surface, world space */
    uint32_t startsInContact;      /* 1: already touching at t = 0 (then t == 0) */
    float normal[3];               /* unit, from point towards the centre at t; -normalize(dir) when they coincide */
    uint32_t _pad;                 /* 0 */
} RtSweep;                         /* not found: t = RT_MISS_DST, everything else 0 */
int  rt_query_sweep(rt_ctx* ctx, const RtSweepBatch* d_batch, RtSweep* d_out);
int  rt_query_sweep_host(rt_ctx* ctx, const RtSweepBatch* batch, RtSweep* out);
int  rt_sweep_exhaustive_host(const RtSceneArrays* scene, const RtSweepBatch* batch, RtSweep* out);

/* Ambient occlusion from first-hit planes ("Ray queries", "Ambient-occlusion plane"). Record i of the planes with
 * ids.w & 1 shoots `samples` occlusion queries: origin position + (normal * 1) * 0.00001 (the next-ray origin of shading),
 * direction the shader's cosineHemisphereDir about normalDepth.xyz (raytrace.comp:405-424, the arithmetic of the diffuse branch of
 * shading), drawn from an rt_random state seeded from (i, sample, seed) (include/rt_ao_rays.h: rt_ao_state), limit `radius`.
 * ao[i] = (float)(samples - k) / (float)samples with k the occluded ones; a record without the hit bit gets 1 and shoots nothing.
 * The record index seeds the RNG, so a plane belongs to one tile layout: the planes of one rt_render_aovs pass, in its order. */
typedef struct RtAoParams {
    uint32_t samples;   /* 1..64 */
    float    radius;    /* finite, > 0 */
    uint32_t seed;      /* any */
} RtAoParams;
void rt_ao_params_default(RtAoParams* p);                    /* 4, 0.5, 0 */
/* Asynchronous on the ctx stream: `samples` rounds of {make the rays, traverse, count}, then one kernel that writes the plane; the
 * host waits for none of them. d_aovs: device planes of rt_render_aovs' layout (position, normalDepth and ids are read), or NULL:
 * the ctx planes of the last rt_render_aovs(…, NULL), which must hold nPixels records. params NULL: the defaults. d_ao: nPixels
 * floats, or NULL: a ctx-owned plane (rt_read_ao). Counters, slots and what it leaves alone: as rt_query_occluded. Refused with a
 * message, in this order: no uploaded scene; samples outside 1..64 or a radius that is not finite and > 0; nPixels 0 or >= 2^30;
 * d_aovs without one of the three planes, or NULL without ctx planes of that size. */
int  rt_render_ao(rt_ctx* ctx, uint32_t nPixels, const RtAovBuffers* d_aovs, const RtAoParams* params, float* d_ao);
/* copies the ctx-owned plane of the last rt_render_ao(…, d_ao = NULL) (nFloats = nPixels of that call); blocks */
int  rt_read_ao(rt_ctx* ctx, float* hostOut, size_t nFloats);
/* Host only, no GPU: the rays of sample `sample` (< samples) as rt_render_ao shoots them, from host planes. origins, dirs:
 * nPixels x 3 floats (zeros where no ray is shot); valid: nPixels bytes, 1 where record i shoots. Returns 0, or -1 on a NULL
 * argument, a missing plane or parameters rt_render_ao refuses. */
int  rt_ao_rays_host(uint32_t nPixels, const RtAovBuffers* aovs, const RtAoParams* params, uint32_t sample,
                     float* origins, float* dirs, uint8_t* valid);

/* Edge-avoiding a-trous denoiser over a whole width x height frame (the spatial filter of SVGF, Schied et al. 2017, after
 * Dammertz et al. 2010; DESIGN.md, "Denoising"). Pixel p is filtered when ids.w & 1 (a hit), ids.z < the material count and
 * that material's emissionStrength == 0, all in the ctx's current material table; every other pixel (misses, emitters) is kept:
 * copied bit for bit and never anyone's neighbour. The filter demodulates e = rgb / max(albedo, 1e-3), estimates the luminance
 * variance over the 5 x 5 window and the depth gradient, runs `iterations` edge-stopping passes with steps 1, 2, 4, ... and
 * remodulates; alpha is copied. */
typedef struct RtDenoiseParams {
    uint32_t iterations;      /* K: a-trous passes, 0..10 (pass k steps 2^k pixels); 0 copies the frame */
    float    sigmaLuminance;  /* σl > 0 */
    float    sigmaNormal;     /* σn >= 0 (0: normals do not stop the filter) */
    float    sigmaDepth;      /* σz > 0 */
} RtDenoiseParams;
void rt_denoise_params_default(RtDenoiseParams* p);          /* 5, 4, 128, 1 (SVGF's published values) */
/* Asynchronous on the ctx stream. d_rgba: the noisy RGBA fp32 frame on the device, or NULL: the ctx framebuffer, whose last
 * rt_render / rt_render_frames(…, NULL) must have been the whole frame (row0 0, rowStride 1, nRows = height). d_aovs: device
 * planes of rt_render_aovs's layout (normalDepth, albedo and ids are read; the other fields are ignored), or NULL: the ctx
 * planes of the last rt_render_aovs(…, NULL), which must also have covered the whole frame. params NULL: the defaults. d_out:
 * the denoised RGBA fp32 frame, not overlapping the inputs, or NULL: a ctx-owned plane (rt_read_denoised_rgba_f32). Needs an
 * uploaded scene (the material table). Its work planes are its own; it changes no counter, no ray-cost figure, none of
 * rt_last_kernel / rt_last_parts / rt_last_pipeline and not the progressive history of the ctx framebuffer. */
int  rt_denoise(rt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba, const RtAovBuffers* d_aovs,
                const RtDenoiseParams* params, float* d_out);
/* copies the ctx-owned output of the last rt_denoise(…, NULL) (nFloats = width*height*4 of that call); blocks */
int  rt_read_denoised_rgba_f32(rt_ctx* ctx, float* hostOut, size_t nFloats);
/* rt_denoise of host arrays (rgba and out: width*height*4 floats; aovs: host planes as above); blocks */
int  rt_denoise_host(rt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const RtAovBuffers* aovs,
                     const RtDenoiseParams* params, float* out);

/* Temporal accumulation by reprojection over a whole width x height frame (the temporal half of SVGF; DESIGN.md, "Temporal
 * accumulation"), to run in front of rt_denoise while the camera moves. The ctx keeps a history: per pixel the accumulated
 * demodulated colour, two luminance moments, the history length N and the surface it showed (normal, depth, object / sphere /
 * material), with the camera of the call that wrote it. A call takes the noisy frame, its first-hit planes and the camera it was
 * rendered with; each filtered pixel (rt_denoise's set: a hit on a material with emissionStrength == 0) takes its world position
 * back through the previous call's camera, reads the four pixels around where it lands there (bilinear weights; a tap counts
 * when it is inside the image, has a history, shows the same object / sphere / material, a normal with n.n' >= normalCos and a
 * depth within depthTolerance, relative, of the pixel's distance to the previous camera), and blends with k = 1 / N,
 * N = min(N_history + 1, maxHistory); without a valid tap it starts again at N = 1. Kept pixels (misses, emitters) come out bit
 * for bit, with moments 0, and are never taps. The scene is taken to be static between calls: after an edit that moves or
 * recolours something, call rt_temporal_reset (rt_upload_scene does; rt_update_* leave that to their caller), or, for edits that
 * only move things, switch rt_temporal_track_motion on (below). */
typedef struct RtTemporalParams {
    uint32_t maxHistory;      /* >= 1: the blend factor never falls below 1 / maxHistory; 1 passes the frame through */
    float    normalCos;       /* in [-1, 1] */
    float    depthTolerance;  /* > 0, relative */
} RtTemporalParams;
void rt_temporal_params_default(RtTemporalParams* p);        /* 32, 0.9, 0.02 (this build's choice: DESIGN.md) */
/* Asynchronous on the ctx stream. cam: the camera the frame was rendered with (required; kept for the next call). d_rgba,
 * d_aovs: as rt_denoise has them (NULL: the ctx framebuffer / the ctx planes, each of the whole frame); normalDepth, position,
 * albedo and ids are read. params NULL: the defaults. d_out: the accumulated RGBA fp32 frame (alpha copied), which may go
 * straight to rt_denoise as its d_rgba; d_moments: per pixel (m1, m2, max(0, m2 - m1^2), N) of the demodulated luminance; either
 * may be NULL: a ctx-owned plane (rt_read_temporal_rgba_f32, rt_read_temporal_moments). Outputs overlap neither the inputs nor
 * each other. A first call, a call after rt_temporal_reset or rt_upload_scene, and a call with another width or height have no
 * history: N = 1 on every filtered pixel. Needs an uploaded scene (the material table). The pass changes no counter, no ray-cost
 * figure, none of rt_last_kernel / rt_last_parts / rt_last_pipeline, not the ctx framebuffer or its progressive history, no AOV
 * plane and not rt_denoise's output plane. A call refused for its arguments leaves the history as it was. */
int  rt_temporal_accumulate(rt_ctx* ctx, uint32_t width, uint32_t height, const CameraInfo* cam, const float* d_rgba,
                            const RtAovBuffers* d_aovs, const RtTemporalParams* params, float* d_out, float* d_moments);
/* forgets the history: the next rt_temporal_accumulate starts at N = 1 */
int  rt_temporal_reset(rt_ctx* ctx);
/* Following moved objects and spheres ("Temporal accumulation", "Moved objects and spheres"). default 0. Switching it
 * (to another value) forgets the history, as rt_temporal_reset does. While it is on, the ctx keeps beside the history a snapshot of
 * the placements every accepted rt_temporal_accumulate saw: per object the rows of transformMatrix and of its inverse as they are
 * in the device tables, and bvhIndex; per sphere its centre and radius. rt_update_objects and rt_update_spheres between two calls
 * then need no reset: a pixel on an object whose rows changed takes its position and normal back through that object's previous
 * placement (P~ = D P with D = Fwd' Inv, n~ = G n / |G n| with G the inverse transpose of D's linear part) before the previous
 * camera and the tap tests see them; a pixel on a sphere that moved or changed radius takes P~ = c' + (P - c) r' / r and its own
 * normal; an object whose bvhIndex changed, and an object or sphere index one of the two calls did not have, has no history
 * (N = 1); everything else is treated exactly as with tracking off, and a call between which and the previous one nothing moved
 * runs the same kernel with the same arguments as with tracking off. What is stored for the next call is this frame's own normal,
 * depth and ids. rt_temporal_reset, rt_upload_scene, another width or height and the switch drop the snapshot with the history; a
 * call refused for its arguments leaves both as they were.
 * Only the surface follows. Light that changes because something moved (shadows, reflections, the lit side of a turning object)
 * lags by up to maxHistory frames. Material edits still want rt_temporal_reset. */
int  rt_temporal_track_motion(rt_ctx* ctx, int enabled);
/* of the last rt_temporal_accumulate: how many objects / spheres it treated as moved and as replaced (all 0: it ran the static
 * kernel). replacedObjects counts the indices only one of the two calls had as well; movedSpheres counts the spheres that moved or
 * changed radius and the sphere indices only one of the two calls had. Any of the three may be NULL. */
int  rt_temporal_motion_state(const rt_ctx* ctx, uint32_t* movedObjects, uint32_t* replacedObjects, uint32_t* movedSpheres);
/* copy the ctx-owned output of the last rt_temporal_accumulate(…, d_out = NULL) / (…, d_moments = NULL)
 * (nFloats = width*height*4 of that call); block */
int  rt_read_temporal_rgba_f32(rt_ctx* ctx, float* hostOut, size_t nFloats);
int  rt_read_temporal_moments(rt_ctx* ctx, float* hostOut, size_t nFloats);
/* rt_temporal_accumulate of host arrays (rgba, out and moments: width*height*4 floats, moments may be NULL; aovs: host planes
 * as above) on the same history; blocks */
int  rt_temporal_accumulate_host(rt_ctx* ctx, uint32_t width, uint32_t height, const CameraInfo* cam, const float* rgba,
                                 const RtAovBuffers* aovs, const RtTemporalParams* params, float* out, float* moments);

/* Sample counts for rt_render_sampled from the moments of rt_temporal_accumulate ("Per-pixel sample counts"): where the
 * accumulated frame is still noisy the next frame gets more samples, where it has converged fewer. Per pixel, from its record
 * (m1, m2, var, N), all in fp32, in this order, without contraction:
 *   N = 0 (a kept pixel: a miss or an emitter, noise-free because the camera ray does not jitter)   -> minSamples
 *   0 < N < 2 (no variance known yet)                                                               -> baseSamples (counted in `unknown`)
 *   otherwise   d = max(m1, luminanceFloor); den = (N * (tau * tau)) * (d * d); q = (baseSamples * var) / den;
 *               n = max(minSamples, q < (float)maxSamples ? (q > 0 ? (uint)ceil(q) : 0) : maxSamples)
 *               (a NaN q gives maxSamples; a q <= 0, which only a negative N or variance gives, counts as 0 before the max)
 * q is the estimated relative variance of the accumulated mean over tau^2: a pixel at the target gets baseSamples, one r times
 * noisier r times as many. The map is in the pixel grid of the frame whose moments it read. */
typedef struct RtSampleMapParams {
    uint32_t baseSamples, minSamples, maxSamples;   /* minSamples <= baseSamples <= maxSamples */
    float    targetRelError;                        /* tau > 0 */
    float    luminanceFloor;                        /* > 0 */
} RtSampleMapParams;
void rt_sample_map_params_default(RtSampleMapParams* p);     /* 4, 1, 16, 0.05, 0.01 (this build's choice: DESIGN.md) */
/* Asynchronous on the ctx stream: one kernel over the width x height frame. d_moments: device plane of width*height records as
 * rt_temporal_accumulate writes them, or NULL: the ctx-owned plane of the last rt_temporal_accumulate(…, d_moments = NULL), which
 * must have this width and height. params NULL: the defaults. d_map: width*height counts, required. Changes no counter, no
 * history and no other plane. */
int  rt_build_sample_map(rt_ctx* ctx, uint32_t width, uint32_t height, const float* d_moments, const RtSampleMapParams* params,
                         uint32_t* d_map);
typedef struct RtSampleMapStats {
    uint64_t samples;                            /* the sum of the counts */
    uint32_t pixels, unknown, aboveMin, atMax;   /* width*height; pixels with 0 < N < 2; with a count > minSamples; == maxSamples */
} RtSampleMapStats;
/* of the last rt_build_sample_map; blocks */
int  rt_sample_map_stats(rt_ctx* ctx, RtSampleMapStats* out);
/* rt_build_sample_map of host arrays (moments: width*height*4 floats, map: width*height counts); blocks */
int  rt_build_sample_map_host(rt_ctx* ctx, uint32_t width, uint32_t height, const float* moments, const RtSampleMapParams* params,
                              uint32_t* map);

int  rt_get_counters(rt_ctx* ctx, RtCounters* out);
int  rt_reset_counters(rt_ctx* ctx);
/* When enabled, every traversal-kernel launch is bracketed by HIP events on
 * the launch stream; rt_get_trace_time_ms returns their summed duration and
 * launch count since the last reset (synchronises). */
int  rt_set_profiling(rt_ctx* ctx, int enabled);
int  rt_get_trace_time_ms(rt_ctx* ctx, double* msOut, uint64_t* launchesOut);
/* The time during which at least one bracketed traversal launch was running since profiling was switched on (the union
 * of the launches' spans: a dispatch of the multi-kernel pipeline runs in parts on several streams, whose launches
 * overlap, so the summed durations of rt_get_trace_time_ms can exceed the wall time). Synchronises. */
int  rt_get_trace_busy_ms(rt_ctx* ctx, double* msOut);
/* Performance knobs; none of them changes a pixel or a counter.
 *   "light_queries"  1 (default): the NEE ray and the cosine probe of a diffuse bounce, which only ask whether their
 *                    closest hit is emissive and how far it is (raytrace.comp:389-403,443-460), are answered from the list of
 *                    emissive primitives where that is possible and stop at the first hit that answers them; 0: every one of
 *                    them is a full closest-hit traversal. Same pixels either way.
 *   "camera_reuse"   1 (default): the samples of a pixel all start with the same camera ray (the shader does not jitter,
 *                    raytrace.comp:541-557,571-573), so its hit is kept from the first sample and the later samples of the
 *                    dispatch start from it without a traversal; 0: traced every time. Off for the debug heat maps.
 *   "pipeline"       -1 (default) pick by tile size, 0 = multi-kernel wavefront pipeline
 *                    (k_trace_pw + k_shade per round), 1 = wave-private fused pipeline
 *                    (k_render_fused: every wave runs the stages on its own 8x8 pixel blocks)
 *   "fused_maps"     0 (default): a scene that binds an alpha, metalness or bump map takes the multi-kernel pipeline whatever
 *                    "pipeline" says; 1: it picks its pipeline like any other scene, and the fused one reads the maps
 *                    (k_render_fused_maps: one configuration for every such scene, as k_trace_pw_alpha)
 *   "fused_below_pixels"  paths of a dispatch (tile pixels x frames) below which -1 picks the fused pipeline
 *   "fused_below_box_tests"  ... and box tests per ray (measured on the context's earlier dispatches of
 *                    the scene, copied back without waiting) below which it does so at any size
 *   "lanes"          multi-kernel pipeline: a dispatch of at least "lanes_min_kslots" x 1024 paths is rendered in this many
 *                    independent parts (contiguous ranges of path slots, each with its own queues and its own stream, forked
 *                    from and joined to the ctx stream), so that one part's shading kernel and the draining tail of its
 *                    traversal launch run under the other parts' traversal; 1..4; 0 (default) = 3, except one for
 *                    dispatches of >= 8 M paths of scenes whose long rays walk into many placed objects (they lose by it)
 *   "lane_grid_pct"  ... each part's traversal launch taking this share of the resident work-groups (10..100; 0 = default: 50 —
 *                    three parts oversubscribe the GPU 1.5 times, so a part in its shading kernel leaves no traversal slot
 *                    empty — and 40 for parts of fewer than 1.2 M paths).
 *                    The parts only overlap while their streams sit on different hardware queues: ROCm deals a process's
 *                    streams onto GPU_MAX_HW_QUEUES queues (default 4); a host with many streams of its own should start
 *                    with that variable raised (bench.py sets 8)
 *   "wide_min_kslots"  multi-kernel pipeline: a dispatch of at least this many x 1024 paths whose traversal kernel would be
 *                    k_trace_pw<20, .., 144, 5> (a BVH 17..20 levels deep, the top-level table of "hot_pairs" 2, no placed
 *                    objects, no heat map) runs it in work-groups of 768 threads, two per CU: six waves per SIMD instead of
 *                    five and all 192 top-level pairs in LDS (k_trace_pw_wide). Default 1024 (1 M paths, the size at which
 *                    a dispatch goes into parts); 0 = always; more than a dispatch can have = never
 *   "wide_grid_pct"  ... and the share of the resident wide work-groups each part's launch takes while "lane_grid_pct" is 0
 *                    (10..100, default 40; 0 = the parts' share as it is)
 *   "radiance_max_kslots"  rt_query_radiance: the most rays x 1024 of one piece of a batch; 0 (default) = the paths
 *                    "frames_max_mslots" allows one dispatch
 *   "tri_plane"      rt_query_triangles, rt_query_cuts: 1 (default): the descent also discards a node whose box lies strictly beside the
 *                    query's plane; 0: by box overlap only. Same records and counts; boxTests and triTests, which count what
 *                    the descent visited, are the one pair of counters a knob moves
 *   "trace_variant"  0 = one ray per lane (k_trace), 1 = persistent waves (k_trace_pw)
 *   "refill", "mk_refill", "chunk", "w_setup", "w_leaf", "fast_lanes", "lds_stack", "blocks_per_cu",
 *   "tile_slots", "phase_stats": traversal scheduling details, see DESIGN.md
 *   "fast_share"     sixteenths of the lanes that hold a ray which suffice to skip the vote (with "fast_lanes" as the
 *                    upper limit; 0 = "fast_lanes" only)
 *   "scatter"        fused pipeline: a block is made of chunks of this many consecutive slots taken from all
 *                    over the tile (0 = a block is neighbouring pixels; -1, default = 4 when a wave gets at
 *                    most two blocks, else 0)
 *   "pixel_refill"   fused pipeline: free lanes at which a wave resolves its finished pixels and reserves new ones,
 *                    1..64 (64 = a block at a time); 0 (default) = 8 when the scene's rays are long (the measure the
 *                    pipeline choice uses), else 64
 *   "batch_pixels"   fused pipeline: pixels per wave-private block, 1..64; 0 (default) = chosen per
 *                    launch so the blocks divide evenly over the resident waves ("batch_fixed" is
 *                    the fixed cost per block, in pixel units, that the chooser assumes) */
int  rt_set_tuning(rt_ctx* ctx, const char* key, int value);
/* The traversal kernel instantiation the last launch used, spelled as a demangler prints it ("k_trace_pw<20, false, false,
 * false, false, 144, 5>", "k_trace_pw_wide<20, 192, 768>", "k_render_fused<24, false, false, true>"): tests/test_instantiations.py forces every instantiation in
 * the library and compares it with the oracle. The string lives in the context. */
const char* rt_last_kernel(const rt_ctx* ctx);
/* parts (streams) the last dispatch of the multi-kernel pipeline ran in ("lanes") */
int  rt_last_parts(const rt_ctx* ctx);
/* pipeline the last rt_render used (0 or 1) */
int  rt_last_pipeline(const rt_ctx* ctx);
/* box tests per executed ray of the uploaded scene as this context measured them (the figure the launch parameters
 * follow); < 0 while unknown. Measured from the counters of earlier dispatches, or — before the first dispatch of
 * >= 8 M pixel-samples of a scene — by a probe dispatch of eight rows at one sample ("probe", 0 turns it off). */
double rt_ray_cost(const rt_ctx* ctx);
/* The reference's BVH builder on the GPU (csrc/bvh_build.hip.h): same nodes, same numbering, same triangle order as
 * the host builder of the scene half (a zero bound may differ in sign). Blocking. `seconds` (optional) = device time. */
int  rt_bvh_build(rt_ctx* ctx, const TrianglePoint* points, uint32_t pointCount, Triangle* triangles, float* centroids,
                  uint32_t count, uint32_t triIndex0, uint32_t nodeBase, BVHNode* nodesOut, uint32_t nodeCapacity,
                  uint32_t* nodeCountOut, uint32_t statsOut[3]);
int  rt_bvh_hook(void* ctx, const TrianglePoint* points, uint32_t pointCount, Triangle* triangles, float* centroids,
                 uint32_t count, uint32_t triIndex0, uint32_t nodeBase, BVHNode* nodesOut, uint32_t nodeCapacity,
                 uint32_t* nodeCountOut, uint32_t statsOut[3]);
/* milliseconds the last rt_bvh_build spent between its first upload and its last download */
double rt_bvh_last_build_ms(const rt_ctx* ctx);

/* ------------------------------------------------------------------ */
/* Several GPUs of one node: one process (and one ctx) per GPU            */
/* ------------------------------------------------------------------ */
/* The frame shards by image rows with no exchange while it renders (a pixel depends on its global index and the read-only
 * scene, raytrace.comp:563-564): rank r of N calls rt_render / rt_render_frames with row0 = r, rowStride = N into a strip of
 * its own, and one gather at the end brings the strips to one rank. These four calls are that gather, over RCCL (xGMI):
 *   rank 0:      rt_comm_unique_id(id), hands the RT_COMM_ID_BYTES to the other processes by any means it has
 *   every rank:  rt_comm_init(ctx, id, N, r)
 *   every rank:  rt_gather_strips(ctx, d_strip, W, H, root, d_frame)  — asynchronous on the ctx stream, rt_sync waits
 * RCCL is loaded on the first of these calls; a single-GPU host never needs it. */
enum { RT_COMM_ID_BYTES = 128 };   /* sizeof(ncclUniqueId) */
int  rt_comm_unique_id(void* idOut);
int  rt_comm_init(rt_ctx* ctx, const void* id, int nRanks, int rank);
int  rt_comm_destroy(rt_ctx* ctx);
/* d_strip: this rank's rows rank, rank + N, ... of a width x height RGBA fp32 frame, in that order (what rt_render wrote);
 * d_frame: the whole frame, on `root` only (NULL elsewhere). Every rank of the communicator must call it. */
int  rt_gather_strips(rt_ctx* ctx, const float* d_strip, uint32_t width, uint32_t height, int root, float* d_frame);
/* The second half of rt_gather_strips on its own, for a host that moves the strips by other means: d_strips holds the strips
 * of ranks 0 .. nRanks - 1 one after the other (rank r: its ceil((height - r) / nRanks) rows in order), d_frame receives the
 * frame's rows. Asynchronous on the ctx stream. (tests: the row arithmetic for heights that nRanks does not divide) */
int  rt_deinterleave_strips(rt_ctx* ctx, const float* d_strips, uint32_t width, uint32_t height, int nRanks, float* d_frame);
/* ... the same with host buffers (copied in and out; blocking) */
int  rt_deinterleave_strips_host(rt_ctx* ctx, const float* strips, uint32_t width, uint32_t height, int nRanks, float* frame);

/* device self-test of the deterministic-math build (must equal RT_SELFTEST_EXPECT) */
int  rt_device_selftest(rt_ctx* ctx, uint32_t* bitsOut);
uint32_t rt_host_selftest(void);
/* Raw values of every GLSL built-in the shader uses (include/rt_probe.h), evaluated on the device: n inputs of 32
 * floats, 64 floats out each. The tests compare them with independent numpy restatements of the GLSL 4.50 formulas. */
int  rt_device_math_probe(rt_ctx* ctx, uint32_t n, const float* in, float* out);
/* streaming-copy ceiling measured on this GPU (GB/s), quoted beside the 8 TB/s nominal */
int  rt_measure_copy_bandwidth(rt_ctx* ctx, size_t bytes, int iters, double* gbpsOut);

const char* rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
