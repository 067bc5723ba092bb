"""ctypes binding of librt_amd.so (the C ABI declared in include/rt_amd.h).

The structs mirror the reference's host structs byte for byte
(src/vk_engine.h:49-79,117-123,145-189; sizes checked in tests/test_layout.py).
The library is built in-tree by `__graft_entry__.build()`; importing this
module never falls back to another implementation: if the .so is missing the
import raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_AMD_LIB: another build of the same ABI, for A/B runs of two builds on one box (tools/)
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(_HERE, "librt_amd.so")


class Sphere(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("materialIndex", C.c_uint32),
                ("_pad", C.c_uint32 * 3)]


class Triangle(C.Structure):
    _fields_ = [("v0", C.c_uint32), ("v1", C.c_uint32), ("v2", C.c_uint32), ("frontOnly", C.c_uint32),
                ("binormal", C.c_float * 3), ("_pad0", C.c_float), ("tangent", C.c_float * 3), ("_pad1", C.c_float)]


class TrianglePoint(C.Structure):
    _fields_ = [("position", C.c_float * 4), ("normal", C.c_float * 4)]


class RayMaterial(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("_pad0", C.c_float), ("emissionColor", C.c_float * 3),
                ("emissionStrength", C.c_float), ("reflectance", C.c_float), ("ior", C.c_float),
                ("albedoIndex", C.c_int32), ("metalnessIndex", C.c_int32), ("alphaIndex", C.c_int32),
                ("bumpIndex", C.c_int32), ("_pad1", C.c_uint32 * 2)]


class RenderObject(C.Structure):
    _fields_ = [("transformMatrix", C.c_float * 16), ("smoothShade", C.c_uint32), ("bvhIndex", C.c_uint32),
                ("materialIndex", C.c_uint32), ("samplerIndex", C.c_uint32)]


class BVHNode(C.Structure):
    _fields_ = [("boundsX", C.c_float * 2), ("boundsY", C.c_float * 2), ("boundsZ", C.c_float * 2),
                ("index", C.c_uint32), ("triCount", C.c_uint32)]


class CameraInfo(C.Structure):
    _fields_ = [("cameraRotation", C.c_float * 16), ("pos", C.c_float * 3), ("nearPlane", C.c_float),
                ("aspectRatio", C.c_float), ("fov", C.c_float), ("_pad", C.c_float * 2)]


class EnvironmentData(C.Structure):
    _fields_ = [("horizonColor", C.c_float * 4), ("zenithColor", C.c_float * 4), ("groundColor", C.c_float * 3),
                ("_pad0", C.c_float), ("lightDir", C.c_float * 4)]


class RayTracerData(C.Structure):
    _fields_ = [("progressive", C.c_uint32), ("singleRender", C.c_uint32), ("debug", C.c_int32),
                ("raysPerPixel", C.c_uint32), ("bounceLimit", C.c_uint32), ("sphereCount", C.c_uint32),
                ("objectCount", C.c_uint32), ("triangleCap", C.c_uint32), ("boxCap", C.c_uint32),
                ("sampleLimit", C.c_uint32)]


class PushConstants(C.Structure):
    _fields_ = [("camInfo", CameraInfo), ("environment", EnvironmentData), ("rayTraceParams", RayTracerData),
                ("frameCount", C.c_uint32), ("_pad", C.c_uint32)]


class RtPlacement(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("rotation", C.c_float * 3), ("scale", C.c_float * 3),
                ("samplerIndex", C.c_uint32), ("frontOnly", C.c_uint32)]


class RtSceneArrays(C.Structure):
    _fields_ = [("spheres", C.POINTER(Sphere)), ("sphereCount", C.c_uint32),
                ("materials", C.POINTER(RayMaterial)), ("materialCount", C.c_uint32),
                ("triPoints", C.POINTER(TrianglePoint)), ("triPointCount", C.c_uint32),
                ("triangles", C.POINTER(Triangle)), ("triangleCount", C.c_uint32),
                ("objects", C.POINTER(RenderObject)), ("objectCount", C.c_uint32),
                ("bvhNodes", C.POINTER(BVHNode)), ("bvhNodeCount", C.c_uint32)]


class RtTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgba8", C.POINTER(C.c_uint8))]


class RtCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference",
                                          "paths", "segments", "traceLaunches", "emitterTests", "skippedBoxTests")]


class RtHit(C.Structure):
    _fields_ = [("dst", C.c_float), ("didHit", C.c_uint32), ("isSphere", C.c_uint32),
                ("objectHitIndex", C.c_uint32), ("triHitIndex", C.c_uint32), ("materialIndex", C.c_uint32),
                ("frontFace", C.c_uint32), ("hitPoint", C.c_float * 3), ("normal", C.c_float * 3),
                ("boxTests", C.c_uint32), ("triTests", C.c_uint32)]


class RtAovBuffers(C.Structure):
    _fields_ = [("normalDepth", C.c_void_p), ("position", C.c_void_p), ("albedo", C.c_void_p), ("rayDir", C.c_void_p),
                ("ids", C.c_void_p)]


class RtRayBatch(C.Structure):
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("tmax", C.c_void_p), ("n", C.c_uint32)]


class RtPointBatch(C.Structure):
    _fields_ = [("points", C.c_void_p), ("maxDist", C.c_void_p), ("n", C.c_uint32)]


class RtBoxBatch(C.Structure):
    _fields_ = [("lo", C.c_void_p), ("hi", C.c_void_p), ("n", C.c_uint32)]


class RtObbBatch(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p), ("n", C.c_uint32), ("sharedFrame", C.c_uint32)]


class RtTriangleBatch(C.Structure):
    _fields_ = [("corners", C.c_void_p), ("n", C.c_uint32)]


class RtOverlap(C.Structure):
    _fields_ = [("found", C.c_uint32), ("isSphere", C.c_uint32), ("objectIndex", C.c_uint32), ("triIndex", C.c_uint32)]


class RtCut(C.Structure):
    _fields_ = [("a", C.c_float * 3), ("featA", C.c_uint32), ("b", C.c_float * 3), ("featB", C.c_uint32),
                ("found", C.c_uint32), ("objectIndex", C.c_uint32), ("triIndex", C.c_uint32), ("reserved", C.c_uint32)]


class RtNearest(C.Structure):
    _fields_ = [("dst", C.c_float), ("found", C.c_uint32), ("isSphere", C.c_uint32), ("objectIndex", C.c_uint32),
                ("triIndex", C.c_uint32), ("uv", C.c_float * 2), ("point", C.c_float * 3), ("_pad", C.c_uint32 * 2)]


class RtSweepBatch(C.Structure):
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("radius", C.c_void_p), ("tmax", C.c_void_p), ("n", C.c_uint32)]


class RtSweep(C.Structure):
    _fields_ = [("t", C.c_float), ("found", C.c_uint32), ("isSphere", C.c_uint32), ("objectIndex", C.c_uint32),
                ("triIndex", C.c_uint32), ("uv", C.c_float * 2), ("gap", C.c_float), ("point", C.c_float * 3),
                ("startsInContact", C.c_uint32), ("normal", C.c_float * 3), ("_pad", C.c_uint32)]


class RtMeshTopology(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("triangles", "weldedVertices", "components", "signableComponents", "signableTriangles", "boundaryEdges",
                                          "nonManifoldEdges", "flippedTriangles", "degenerateTriangles")] + [("orientation", C.c_int32)]


class RtRadianceParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("bounceLimit", C.c_uint32), ("progressive", C.c_uint32), ("frameCount", C.c_uint32)]


class RtPointNormalBatch(C.Structure):
    _fields_ = [("points", C.c_void_p), ("normals", C.c_void_p), ("n", C.c_uint32)]


class RtIrradianceParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("bounceLimit", C.c_uint32), ("progressive", C.c_uint32), ("frameCount", C.c_uint32),
                ("bias", C.c_float)]


class RtTexel(C.Structure):
    _fields_ = [("point", C.c_float * 3), ("state", C.c_uint32), ("normal", C.c_float * 3), ("triIndex", C.c_uint32),
                ("uv", C.c_float * 2), ("_pad", C.c_uint32 * 2)]


class RtTexelStats(C.Structure):
    _fields_ = [("covered", C.c_uint32), ("overlapped", C.c_uint32), ("skippedTriangles", C.c_uint32), ("degenerateTexels", C.c_uint32)]


class RtAoParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("radius", C.c_float), ("seed", C.c_uint32)]


class RtDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigmaLuminance", C.c_float), ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float)]


class RtTemporalParams(C.Structure):
    _fields_ = [("maxHistory", C.c_uint32), ("normalCos", C.c_float), ("depthTolerance", C.c_float)]


class RtSampleMapParams(C.Structure):
    _fields_ = [("baseSamples", C.c_uint32), ("minSamples", C.c_uint32), ("maxSamples", C.c_uint32), ("targetRelError", C.c_float),
                ("luminanceFloor", C.c_float)]


class RtSampleMapStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("pixels", C.c_uint32), ("unknown", C.c_uint32), ("aboveMin", C.c_uint32), ("atMax", C.c_uint32)]


# every symbol include/rt_amd.h declares: name -> (restype, argtypes)
_P = C.POINTER
_vp = C.c_void_p
SYMBOLS = {
    "rt_scene_create": (C.c_int, [_P(_vp)]),
    "rt_scene_destroy": (None, [_vp]),
    "rt_scene_last_error": (C.c_char_p, [_vp]),
    "rt_scene_add_material": (C.c_int, [_vp, _P(RayMaterial)]),
    "rt_material_default": (None, [_P(RayMaterial)]),
    "rt_scene_set_sphere": (C.c_int, [_vp, C.c_uint32, _P(C.c_float), C.c_float, C.c_uint32]),
    "rt_placement_default": (None, [_P(RtPlacement)]),
    "rt_scene_read_obj": (C.c_int, [_vp, C.c_char_p, _P(RtPlacement), C.c_int]),
    "rt_scene_read_mtl": (C.c_int, [_vp, C.c_char_p]),
    "rt_scene_add_mesh": (C.c_int, [_vp, C.c_char_p, _P(C.c_float), _P(C.c_float), _P(C.c_float), C.c_uint32,
                                    _P(RtPlacement), C.c_int]),
    "rt_scene_cornell_box": (C.c_int, [_vp, C.c_char_p]),
    "rt_scene_prepare_default": (C.c_int, [_vp, C.c_char_p]),
    "rt_scene_get_arrays": (C.c_int, [_vp, _P(RtSceneArrays)]),
    "rt_scene_texture_count": (C.c_uint32, [_vp]),
    "rt_scene_texture_path": (C.c_char_p, [_vp, C.c_uint32]),
    "rt_scene_add_texture": (C.c_int, [_vp, C.c_char_p]),
    "rt_scene_set_material": (C.c_int, [_vp, C.c_uint32, _P(RayMaterial)]),
    "rt_scene_update_points": (C.c_int, [_vp, _P(TrianglePoint), C.c_uint32, C.c_uint32]),
    "rt_scene_find_material": (C.c_int, [_vp, C.c_char_p]),
    "rt_scene_last_bvh_stats": (C.c_int, [_vp, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "rt_scene_set_bvh_hook": (C.c_int, [_vp, _vp, _vp]),
    "rt_camera_rotation": (None, [_P(C.c_float), _P(C.c_float)]),
    "rt_push_constants_default": (None, [_P(PushConstants), C.c_uint32, C.c_uint32]),
    "rt_transform_matrix": (None, [_P(RtPlacement), _P(C.c_float)]),
    "rt_device_count": (C.c_int, [_P(C.c_int)]),
    "rt_create": (C.c_int, [C.c_int, _P(_vp)]),
    "rt_destroy": (None, [_vp]),
    "rt_last_error": (C.c_char_p, [_vp]),
    "rt_set_stream": (C.c_int, [_vp, _vp]),
    "rt_upload_scene": (C.c_int, [_vp, _P(RtSceneArrays)]),
    "rt_upload_scene_dynamic": (C.c_int, [_vp, _P(RtSceneArrays)]),
    "rt_update_points": (C.c_int, [_vp, _P(TrianglePoint), C.c_uint32, C.c_uint32]),
    "rt_upload_textures": (C.c_int, [_vp, _P(RtTexture), C.c_uint32]),
    "rt_update_materials": (C.c_int, [_vp, _P(RayMaterial), C.c_uint32]),
    "rt_update_spheres": (C.c_int, [_vp, _P(Sphere), C.c_uint32]),
    "rt_update_objects": (C.c_int, [_vp, _P(RenderObject), C.c_uint32]),
    "rt_render": (C.c_int, [_vp, _P(PushConstants), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    "rt_render_frames": (C.c_int, [_vp, _P(PushConstants), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    "rt_render_sampled": (C.c_int, [_vp, _P(PushConstants), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "rt_sync": (C.c_int, [_vp]),
    "rt_clear_framebuffer": (C.c_int, [_vp]),
    "rt_read_rgba_f32": (C.c_int, [_vp, _P(C.c_float), C.c_size_t]),
    "rt_read_rgba8_srgb": (C.c_int, [_vp, _P(C.c_uint8), C.c_size_t]),
    "rt_trace_rays": (C.c_int, [_vp, C.c_uint32, _P(C.c_float), _P(C.c_float), _P(RtHit)]),
    "rt_render_aovs": (C.c_int, [_vp, _P(PushConstants), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P(RtAovBuffers)]),
    "rt_read_aovs": (C.c_int, [_vp, _P(RtAovBuffers), C.c_size_t]),
    "rt_render_guides": (C.c_int, [_vp, _P(PushConstants), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   _P(RtAovBuffers), _P(RtAovBuffers)]),
    "rt_read_guides": (C.c_int, [_vp, _P(RtAovBuffers), C.c_size_t]),
    "rt_query_closest": (C.c_int, [_vp, _P(RtRayBatch), _vp]),
    "rt_query_occluded": (C.c_int, [_vp, _P(RtRayBatch), _vp]),
    "rt_query_closest_host": (C.c_int, [_vp, _P(RtRayBatch), _vp]),
    "rt_query_occluded_host": (C.c_int, [_vp, _P(RtRayBatch), _vp]),
    "rt_query_hits": (C.c_int, [_vp, _P(RtRayBatch), C.c_uint32, _vp, _vp]),
    "rt_query_hits_host": (C.c_int, [_vp, _P(RtRayBatch), C.c_uint32, _vp, _vp]),
    "rt_hits_walk_host": (C.c_int, [_P(RtSceneArrays), C.c_uint32, C.c_uint32, _P(RtTexture), C.c_uint32, _P(RtRayBatch), C.c_uint32, _vp, _vp]),
    "rt_query_nearest": (C.c_int, [_vp, _P(RtPointBatch), _vp]),
    "rt_query_nearest_host": (C.c_int, [_vp, _P(RtPointBatch), _vp]),
    "rt_nearest_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtPointBatch), _vp]),
    "rt_scene_topology": (C.c_int, [_P(RtSceneArrays), _P(RtMeshTopology), C.c_uint32]),
    "rt_nearest_side_host": (C.c_int, [_P(RtSceneArrays), _P(RtPointBatch), _vp, _vp]),
    "rt_nearest_side_features_host": (C.c_int, [_P(RtSceneArrays), _P(RtPointBatch), _vp, _vp, _vp, _vp]),
    "rt_upload_topology": (C.c_int, [_vp, _P(RtSceneArrays)]),
    "rt_query_nearest_signed": (C.c_int, [_vp, _P(RtPointBatch), _vp, _vp]),
    "rt_query_nearest_signed_host": (C.c_int, [_vp, _P(RtPointBatch), _vp, _vp]),
    "rt_query_within": (C.c_int, [_vp, _P(RtPointBatch), C.c_uint32, _vp, _vp]),
    "rt_query_within_host": (C.c_int, [_vp, _P(RtPointBatch), C.c_uint32, _vp, _vp]),
    "rt_within_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtPointBatch), C.c_uint32, _vp, _vp]),
    "rt_query_boxes": (C.c_int, [_vp, _P(RtBoxBatch), C.c_uint32, _vp, _vp]),
    "rt_query_boxes_host": (C.c_int, [_vp, _P(RtBoxBatch), C.c_uint32, _vp, _vp]),
    "rt_boxes_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtBoxBatch), C.c_uint32, _vp, _vp]),
    "rt_query_oriented_boxes": (C.c_int, [_vp, _P(RtObbBatch), C.c_uint32, _vp, _vp]),
    "rt_query_oriented_boxes_host": (C.c_int, [_vp, _P(RtObbBatch), C.c_uint32, _vp, _vp]),
    "rt_obbs_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtObbBatch), C.c_uint32, _vp, _vp]),
    "rt_query_triangles": (C.c_int, [_vp, _P(RtTriangleBatch), C.c_uint32, _vp, _vp]),
    "rt_query_triangles_host": (C.c_int, [_vp, _P(RtTriangleBatch), C.c_uint32, _vp, _vp]),
    "rt_tris_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtTriangleBatch), C.c_uint32, _vp, _vp]),
    "rt_query_cuts": (C.c_int, [_vp, _P(RtTriangleBatch), C.c_uint32, _vp, _vp]),
    "rt_query_cuts_host": (C.c_int, [_vp, _P(RtTriangleBatch), C.c_uint32, _vp, _vp]),
    "rt_cuts_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtTriangleBatch), C.c_uint32, _vp, _vp]),
    "rt_object_frames_host": (C.c_int, [_P(RtSceneArrays), _vp, C.c_uint32, _vp]),
    "rt_query_sweep": (C.c_int, [_vp, _P(RtSweepBatch), _vp]),
    "rt_query_sweep_host": (C.c_int, [_vp, _P(RtSweepBatch), _vp]),
    "rt_sweep_exhaustive_host": (C.c_int, [_P(RtSceneArrays), _P(RtSweepBatch), _vp]),
    "rt_radiance_params_default": (None, [_P(RtRadianceParams)]),
    "rt_query_radiance": (C.c_int, [_vp, _P(RtRayBatch), _vp, _P(RtRadianceParams), _P(EnvironmentData), _vp]),
    "rt_query_radiance_host": (C.c_int, [_vp, _P(RtRayBatch), _vp, _P(RtRadianceParams), _P(EnvironmentData), _vp]),
    "rt_irradiance_params_default": (None, [_P(RtIrradianceParams)]),
    "rt_query_irradiance": (C.c_int, [_vp, _P(RtPointNormalBatch), _vp, _P(RtIrradianceParams), _P(EnvironmentData), _vp]),
    "rt_query_irradiance_host": (C.c_int, [_vp, _P(RtPointNormalBatch), _vp, _P(RtIrradianceParams), _P(EnvironmentData), _vp]),
    "rt_query_sh_probes": (C.c_int, [_vp, _P(RtPointNormalBatch), _vp, _P(RtIrradianceParams), _P(EnvironmentData), _vp]),
    "rt_query_sh_probes_host": (C.c_int, [_vp, _P(RtPointNormalBatch), _vp, _P(RtIrradianceParams), _P(EnvironmentData), _vp]),
    "rt_irradiance_rays_host": (C.c_int, [_P(RtPointNormalBatch), _vp, _P(RtIrradianceParams), C.c_int, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "rt_irradiance_gather_host": (C.c_int, [_P(RtPointNormalBatch), _vp, _P(RtIrradianceParams), C.c_int, _vp, _vp]),
    "rt_bake_texels": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _P(RtTexelStats)]),
    "rt_bake_texels_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _P(RtTexelStats)]),
    "rt_texels_exhaustive_host": (C.c_int, [_P(RtSceneArrays), C.c_uint32, C.c_uint32, C.c_uint32, _vp, _P(RtTexelStats)]),
    "rt_texels_compact": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "rt_texels_scatter": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp]),
    "rt_dilate_texels": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "rt_dilate_texels_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "rt_bake_lightmap": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _P(RtIrradianceParams), _P(EnvironmentData), C.c_uint32, _vp, _vp,
                                   _P(RtTexelStats)]),
    "rt_ao_params_default": (None, [_P(RtAoParams)]),
    "rt_render_ao": (C.c_int, [_vp, C.c_uint32, _P(RtAovBuffers), _P(RtAoParams), _vp]),
    "rt_read_ao": (C.c_int, [_vp, _P(C.c_float), C.c_size_t]),
    "rt_ao_rays_host": (C.c_int, [C.c_uint32, _P(RtAovBuffers), _P(RtAoParams), C.c_uint32, _P(C.c_float), _P(C.c_float), _P(C.c_uint8)]),
    "rt_denoise_params_default": (None, [_P(RtDenoiseParams)]),
    "rt_denoise": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _P(RtAovBuffers), _P(RtDenoiseParams), _vp]),
    "rt_read_denoised_rgba_f32": (C.c_int, [_vp, _P(C.c_float), C.c_size_t]),
    "rt_denoise_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _P(RtAovBuffers), _P(RtDenoiseParams), _vp]),
    "rt_temporal_params_default": (None, [_P(RtTemporalParams)]),
    "rt_temporal_accumulate": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _P(CameraInfo), _vp, _P(RtAovBuffers), _P(RtTemporalParams), _vp, _vp]),
    "rt_temporal_reset": (C.c_int, [_vp]),
    "rt_temporal_track_motion": (C.c_int, [_vp, C.c_int]),
    "rt_temporal_motion_state": (C.c_int, [_vp, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "rt_read_temporal_rgba_f32": (C.c_int, [_vp, _P(C.c_float), C.c_size_t]),
    "rt_read_temporal_moments": (C.c_int, [_vp, _P(C.c_float), C.c_size_t]),
    "rt_temporal_accumulate_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _P(CameraInfo), _vp, _P(RtAovBuffers), _P(RtTemporalParams), _vp, _vp]),
    "rt_sample_map_params_default": (None, [_P(RtSampleMapParams)]),
    "rt_build_sample_map": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _P(RtSampleMapParams), _vp]),
    "rt_sample_map_stats": (C.c_int, [_vp, _P(RtSampleMapStats)]),
    "rt_build_sample_map_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, _P(RtSampleMapParams), _vp]),
    "rt_get_counters": (C.c_int, [_vp, _P(RtCounters)]),
    "rt_reset_counters": (C.c_int, [_vp]),
    "rt_set_profiling": (C.c_int, [_vp, C.c_int]),
    "rt_get_trace_time_ms": (C.c_int, [_vp, _P(C.c_double), _P(C.c_uint64)]),
    "rt_get_trace_busy_ms": (C.c_int, [_vp, _P(C.c_double)]),
    "rt_last_kernel": (C.c_char_p, [_vp]),
    "rt_last_parts": (C.c_int, [_vp]),
    "rt_set_tuning": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "rt_last_pipeline": (C.c_int, [_vp]),
    "rt_ray_cost": (C.c_double, [_vp]),
    "rt_bvh_build": (C.c_int, [_vp, _P(TrianglePoint), C.c_uint32, _P(Triangle), _P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, _P(BVHNode), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "rt_bvh_hook": (C.c_int, [_vp, _P(TrianglePoint), C.c_uint32, _P(Triangle), _P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, _P(BVHNode), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "rt_bvh_last_build_ms": (C.c_double, [_vp]),
    "rt_comm_unique_id": (C.c_int, [_vp]),
    "rt_comm_init": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "rt_comm_destroy": (C.c_int, [_vp]),
    "rt_gather_strips": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "rt_deinterleave_strips": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "rt_deinterleave_strips_host": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "rt_device_selftest": (C.c_int, [_vp, _P(C.c_uint32)]),
    "rt_host_selftest": (C.c_uint32, []),
    "rt_device_math_probe": (C.c_int, [_vp, C.c_uint32, _P(C.c_float), _P(C.c_float)]),
    "rt_measure_copy_bandwidth": (C.c_int, [_vp, C.c_size_t, C.c_int, _P(C.c_double)]),
    "rt_version": (C.c_char_p, []),
}

_lib = None


def lib():
    """Load librt_amd.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU or PyTorch fallback for the HIP path)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib
