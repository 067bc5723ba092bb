"""Host-side mirror of the reference engine's path-tracing surface.

`Scene` keeps the reference's scene vectors and builders (VulkanEngine::
read_obj / read_mtl / cornell_box / prepare_storage_buffers,
src/vk_engine.cpp:638-758, 800-1167) behind the C ABI's scene half.
`Renderer` is the device half: `upload_scene` = the copy_buffer calls
(src/vk_engine.cpp:753-757), `update_*` = update_buffer (:1446-1475),
`run_compute` = run_compute (:1623-1676) with the same frame semantics
(`totalSamples < sampleLimit`, single render = one dispatch of sampleLimit spp,
otherwise raysPerPixel spp per dispatch and frameCount advancing only when
progressive, :1782,1812-1814).

Everything numeric happens in librt_amd.so; this file only moves pointers.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from .devmem import DeviceBuffer, RtError, hip as _hip   # noqa: F401  (engine.RtError and engine._hip are where callers know them)
from ._capi import (BVHNode, PushConstants, RayMaterial, RenderObject, RtAoParams, RtAovBuffers, RtBoxBatch, RtCounters, RtCut, RtDenoiseParams, RtHit, RtIrradianceParams, RtMeshTopology, RtNearest, RtObbBatch, RtOverlap, RtPointBatch, RtPointNormalBatch, RtRadianceParams, RtRayBatch, RtSweep, RtSweepBatch, RtTexel, RtTexelStats, RtTriangleBatch,
                    RtPlacement, RtSampleMapParams, RtSampleMapStats, RtSceneArrays, RtTemporalParams, RtTexture, Sphere, Triangle, TrianglePoint)

ASSET_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


def placement(position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1), samplerIndex=0, frontOnly=False):
    """ImGuiObject's placement fields (src/vk_engine.h:125-132)."""
    p = RtPlacement()
    _capi.lib().rt_placement_default(C.byref(p))
    if np.isscalar(scale):
        scale = (scale,) * 3
    p.position[:] = [float(x) for x in position]
    p.rotation[:] = [float(x) for x in rotation]
    p.scale[:] = [float(x) for x in scale]
    p.samplerIndex = int(samplerIndex)
    p.frontOnly = 1 if frontOnly else 0
    return p


def default_material(**kw):
    m = RayMaterial()
    _capi.lib().rt_material_default(C.byref(m))
    for k, v in kw.items():
        if k in ("albedo", "emissionColor"):
            getattr(m, k)[:] = [float(x) for x in v]
        else:
            setattr(m, k, v)
    return m


def push_constants(width, height, **params):
    """PushConstants with the reference's defaults (src/vk_engine.h:145-171,325).
    Keyword names are the reference's field names; `cameraAngles` (degrees)
    recomputes cameraRotation as run_compute does."""
    pc = PushConstants()
    l = _capi.lib()
    l.rt_push_constants_default(C.byref(pc), width, height)
    for k, v in params.items():
        if k == "cameraAngles":
            ang = (C.c_float * 3)(*[float(x) for x in v])
            l.rt_camera_rotation(ang, pc.camInfo.cameraRotation)
        elif k in ("pos",):
            pc.camInfo.pos[:] = [float(x) for x in v]
        elif k in ("nearPlane", "aspectRatio", "fov"):
            setattr(pc.camInfo, k, float(v))
        elif k in ("horizonColor", "zenithColor", "groundColor", "lightDir"):
            getattr(pc.environment, k)[:] = [float(x) for x in v]
        elif k == "environmentOn":
            pc.environment.lightDir[3] = 1.0 if v else 0.0
        elif k == "frameCount":
            pc.frameCount = int(v)
        elif hasattr(pc.rayTraceParams, k):
            setattr(pc.rayTraceParams, k, int(v))
        else:
            raise KeyError(k)
    return pc


def _points_arg(points):
    """An (n, 8) float32 array (position.xyz, u, normal.xyz, v per point) or a ctypes array of TrianglePoint -> (pointer, n, keep-alive)."""
    if isinstance(points, C.Array) and points._type_ is TrianglePoint:
        return C.cast(points, C.POINTER(TrianglePoint)), len(points), points
    a = np.ascontiguousarray(points, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"points {a.shape}: not an (n, 8) float32 array of TrianglePoint records")
    return C.cast(a.ctypes.data, C.POINTER(TrianglePoint)), a.shape[0], a


class Scene:
    """The reference's CPU-side scene: spheres, rayMaterials, triPoints,
    triangles, objects, bvhNodes (src/vk_engine.h:270-283)."""

    def __init__(self):
        self._l = _capi.lib()
        h = C.c_void_p()
        if self._l.rt_scene_create(C.byref(h)) != 0:
            raise RtError("rt_scene_create failed")
        self._h = h

    def close(self):
        if self._h:
            self._l.rt_scene_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what):
        if rc < 0:
            raise RtError(f"{what}: {self._l.rt_scene_last_error(self._h).decode()}")
        return rc

    # -- builders ---------------------------------------------------------
    def add_material(self, m):
        return self._check(self._l.rt_scene_add_material(self._h, C.byref(m)), "add_material")

    def set_sphere(self, i, position, radius, materialIndex):
        pos = (C.c_float * 3)(*[float(x) for x in position])
        self._check(self._l.rt_scene_set_sphere(self._h, i, pos, float(radius), int(materialIndex)), "set_sphere")

    def read_obj(self, filePath, imGuiObj=None, material=0):
        p = imGuiObj if imGuiObj is not None else placement()
        return self._check(self._l.rt_scene_read_obj(self._h, os.fsencode(filePath), C.byref(p), int(material)),
                           "read_obj")

    def read_mtl(self, filePath):
        return self._check(self._l.rt_scene_read_mtl(self._h, os.fsencode(filePath)), "read_mtl")

    def add_mesh(self, key, positions, normals, imGuiObj=None, material=0, uvs=None):
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 9)
        assert pos.shape == nrm.shape
        fp = C.POINTER(C.c_float)
        uvp = None
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
            uvp = uvs.ctypes.data_as(fp)
        p = imGuiObj if imGuiObj is not None else placement()
        return self._check(self._l.rt_scene_add_mesh(self._h, key.encode(), pos.ctypes.data_as(fp),
                                                     nrm.ctypes.data_as(fp), uvp, pos.shape[0], C.byref(p),
                                                     int(material)), "add_mesh")

    def cornell_box(self, assetDir=ASSET_DIR):
        self._check(self._l.rt_scene_cornell_box(self._h, os.fsencode(assetDir)), "cornell_box")

    def prepare_storage_buffers(self, assetDir=ASSET_DIR):
        self._check(self._l.rt_scene_prepare_default(self._h, os.fsencode(assetDir)), "prepare_storage_buffers")

    def use_device_bvh(self, renderer):
        """Meshes added from now on get their BVH from the GPU builder of `renderer` (rt_bvh_hook):
        the same nodes, numbering and triangle order as the host builder. None switches back."""
        if renderer is None:
            self._check(self._l.rt_scene_set_bvh_hook(self._h, None, None), "rt_scene_set_bvh_hook")
        else:
            fn = C.cast(self._l.rt_bvh_hook, C.c_void_p)
            self._check(self._l.rt_scene_set_bvh_hook(self._h, fn, renderer._h), "rt_scene_set_bvh_hook")
        self._bvh_renderer = renderer  # keep it alive as long as the hook points at it

    def texture_paths(self):
        """Image file of every texture slot the MTL files (or add_texture) claimed, in slot order."""
        n = self._l.rt_scene_texture_count(self._h)
        return [os.fsdecode(self._l.rt_scene_texture_path(self._h, i)) for i in range(n)]

    def add_texture(self, path):
        """Claims the next texture slot for an image file; bind it through a material's albedoIndex."""
        return self._check(self._l.rt_scene_add_texture(self._h, os.fsencode(path)), "add_texture")

    def set_material(self, i, m):
        self._check(self._l.rt_scene_set_material(self._h, int(i), C.byref(m)), "set_material")

    def update_points(self, points, first=0):
        """Replaces triPoints[first, first + n) and refits the BVH boxes of the meshes that use them, topology kept
        (rt_scene_update_points): what Renderer.update_points does to the device tables, on this scene's own arrays. `points`: an
        (n, 8) float32 array (position.xyz, u, normal.xyz, v per point) or a ctypes array of TrianglePoint."""
        p, n, _keep = _points_arg(points)
        self._check(self._l.rt_scene_update_points(self._h, p, int(first), n), "rt_scene_update_points")

    def points(self):
        """triPoints as an (n, 8) float32 array (copied): position.xyz, u, normal.xyz, v."""
        a = self.arrays()
        return self._view(a.triPoints, a.triPointCount, TrianglePoint).copy().view(np.float32).reshape(-1, 8)

    def material(self, i):
        a = self.arrays()
        m = RayMaterial()
        C.memmove(C.byref(m), C.byref(a.materials[i]), C.sizeof(RayMaterial))
        return m

    def find_material(self, key):
        return self._l.rt_scene_find_material(self._h, key.encode())

    def last_bvh_stats(self):
        v = [C.c_uint32() for _ in range(4)]
        self._l.rt_scene_last_bvh_stats(self._h, *[C.byref(x) for x in v])
        return dict(zip(("nodeCount", "maxDepth", "minDepth", "maxTri"), [x.value for x in v]))

    # -- views ------------------------------------------------------------
    def arrays(self):
        a = RtSceneArrays()
        self._check(self._l.rt_scene_get_arrays(self._h, C.byref(a)), "get_arrays")
        return a

    def _view(self, ptr, n, ctype):
        if n == 0:
            return np.zeros((0,), dtype=np.uint8)
        buf = (ctype * n).from_address(C.addressof(ptr.contents))
        return np.frombuffer(buf, dtype=np.uint8).reshape(n, C.sizeof(ctype))

    def numpy(self):
        """Raw byte views (copied) of the six scene arrays, for tests."""
        a = self.arrays()
        return {
            "spheres": self._view(a.spheres, a.sphereCount, Sphere).copy(),
            "materials": self._view(a.materials, a.materialCount, RayMaterial).copy(),
            "triPoints": self._view(a.triPoints, a.triPointCount, TrianglePoint).copy(),
            "triangles": self._view(a.triangles, a.triangleCount, Triangle).copy(),
            "objects": self._view(a.objects, a.objectCount, RenderObject).copy(),
            "bvhNodes": self._view(a.bvhNodes, a.bvhNodeCount, BVHNode).copy(),
        }

    def topology(self):
        """Per object, the statistics of its mesh's topology table and its orientation (rt_scene_topology; DESIGN.md, "Signed point
        queries"; no GPU): a list of dicts with RtMeshTopology's fields."""
        return scene_topology(self.arrays())

    def counts(self):
        a = self.arrays()
        return dict(spheres=a.sphereCount, materials=a.materialCount, triPoints=a.triPointCount,
                    triangles=a.triangleCount, objects=a.objectCount, bvhNodes=a.bvhNodeCount)


class Renderer:
    """One MI355X: device buffers + the wavefront pipeline (rt_ctx)."""

    def __init__(self, device=0):
        self._l = _capi.lib()
        h = C.c_void_p()
        rc = self._l.rt_create(int(device), C.byref(h))
        if rc != 0:
            raise RtError(f"rt_create(device={device}) failed with {rc}: no usable HIP device "
                          "(this path has no CPU fallback)")
        self._h = h
        self.device = device
        self.totalSamples = 0
        self._frameNumber = 0
        self._scene = None
        self._shape = None
        self._aov_shape = None
        self._owned = {}                  # device buffers of this module, by name (_device_buffer)

    def close(self):
        if getattr(self, "_h", None):
            for b in self._owned.values():
                b.free()
            self._owned = {}
            self._l.rt_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise RtError(f"{what} failed ({rc}): {self._l.rt_last_error(self._h).decode()}")

    def set_stream(self, hip_stream_ptr):
        self._check(self._l.rt_set_stream(self._h, C.c_void_p(hip_stream_ptr)), "rt_set_stream")

    def upload_scene(self, scene, dynamic=False):
        """rt_upload_scene; with `dynamic` rt_upload_scene_dynamic, which also keeps on the device what update_points() needs."""
        a = scene.arrays()
        if dynamic:
            self._check(self._l.rt_upload_scene_dynamic(self._h, C.byref(a)), "rt_upload_scene_dynamic")
        else:
            self._check(self._l.rt_upload_scene(self._h, C.byref(a)), "rt_upload_scene")
        self._scene = scene
        self._counts = scene.counts()

    def update_points(self, points, first=0):
        """Deforms the uploaded meshes in place (rt_update_points; DESIGN.md, "Deforming meshes"): replaces triPoints[first, first + n)
        of a scene uploaded with upload_scene(dynamic=True) and refits the BVH boxes on the device, topology kept. Blocks. `points`:
        an (n, 8) float32 array (position.xyz, u, normal.xyz, v per point) or a ctypes array of TrianglePoint. The host scene is not
        touched: Scene.update_points does the same there (InteractiveSession.update_points calls both)."""
        p, n, _keep = _points_arg(points)
        self._check(self._l.rt_update_points(self._h, p, int(first), n), "rt_update_points")

    def upload_textures(self, images):
        """The scene's texture table: a list of uint8 arrays [h, w, 4] in slot order (rt_upload_textures); [] removes it."""
        arr = (RtTexture * max(len(images), 1))()
        keep = []
        for i, im in enumerate(images):
            im = np.ascontiguousarray(im, dtype=np.uint8)
            if im.ndim != 3 or im.shape[2] != 4:
                raise ValueError("textures are [height, width, 4] uint8 (RGBA)")
            keep.append(im)
            arr[i].width, arr[i].height = im.shape[1], im.shape[0]
            arr[i].rgba8 = im.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self._l.rt_upload_textures(self._h, arr, len(images)), "rt_upload_textures")

    def update_materials(self, scene):
        a = scene.arrays()
        self._check(self._l.rt_update_materials(self._h, a.materials, a.materialCount), "rt_update_materials")

    def update_spheres(self, scene):
        a = scene.arrays()
        self._check(self._l.rt_update_spheres(self._h, a.spheres, a.sphereCount), "rt_update_spheres")

    def update_objects(self, scene):
        a = scene.arrays()
        self._check(self._l.rt_update_objects(self._h, a.objects, a.objectCount), "rt_update_objects")

    def fill_counts(self, pc):
        """rayTracerParams.sphereCount/objectCount as run_compute sets them (:1655-1656)."""
        pc.rayTraceParams.sphereCount = self._counts["spheres"]
        pc.rayTraceParams.objectCount = self._counts["objects"]
        return pc

    def render(self, pc, width, height, row0=0, rowStride=1, nRows=None, out_ptr=None, sync=True):
        """One dispatch. Returns an (nRows, width, 4) float32 array unless the
        caller supplied a device pointer."""
        if nRows is None:
            nRows = _tile_rows(height, row0, rowStride)
        self.fill_counts(pc)
        self._check(self._l.rt_render(self._h, C.byref(pc), width, height, row0, rowStride, nRows,
                                      C.c_void_p(out_ptr) if out_ptr else None), "rt_render")
        return self._rendered(nRows, width, out_ptr, sync)

    def _rendered(self, nRows, width, out_ptr, sync):
        """The common end of render / render_frames / render_sampled: the tile's array, or None when the caller did not wait
        (sync=False) or supplied the device pointer."""
        self._shape = (nRows, width, 4)
        if not sync:
            return None
        self.sync()
        return None if out_ptr else self.read_rgba()

    def render_frames(self, pc, width, height, nFrames, row0=0, rowStride=1, nRows=None, out_ptr=None, sync=True):
        """nFrames progressive dispatches starting at pc.frameCount (rt_render_frames): the frames share launches where one
        frame would leave the GPU short of pixels. Same pixels as nFrames render() calls."""
        if nRows is None:
            nRows = _tile_rows(height, row0, rowStride)
        self.fill_counts(pc)
        self._check(self._l.rt_render_frames(self._h, C.byref(pc), width, height, row0, rowStride, nRows, int(nFrames),
                                             C.c_void_p(out_ptr) if out_ptr else None), "rt_render_frames")
        return self._rendered(nRows, width, out_ptr, sync)

    def render_sampled(self, pc, width, height, sample_map, nFrames=1, row0=0, rowStride=1, nRows=None, out_ptr=None, sync=True):
        """render_frames() with a sample count per pixel (rt_render_sampled): pixel p gets min(sample_map[p], S) samples, S being the
        count render() would use, and comes out bit for bit as render_frames() gives it at that count; a pixel with 0 is not written
        and costs nothing. `sample_map`: an (nRows, width) array of counts in the order of the rows rendered, or a device pointer (int)
        to such a plane, as build_sample_map(to_host=False) returns it; None: render_frames()."""
        if nRows is None:
            nRows = _tile_rows(height, row0, rowStride)
        d_map = None
        if sample_map is not None and not isinstance(sample_map, (int, np.integer)):
            m = np.ascontiguousarray(sample_map, np.uint32)
            if m.shape != (nRows, width):
                raise ValueError(f"sample_map {m.shape}: not the ({nRows}, {width}) counts of the rows rendered")
            self.sync()   # (a dispatch still in flight may be reading the buffer this one reuses)
            d_map = self._owned_buffer("sample_map_in", m.nbytes).upload(m, error="render_sampled: the sample map could not be copied to the device").ptr
        elif sample_map is not None:
            d_map = int(sample_map)
        self.fill_counts(pc)
        self._check(self._l.rt_render_sampled(self._h, C.byref(pc), width, height, row0, rowStride, nRows, int(nFrames),
                                              C.c_void_p(d_map) if d_map else None, C.c_void_p(out_ptr) if out_ptr else None),
                    "rt_render_sampled")
        return self._rendered(nRows, width, out_ptr, sync)

    def build_sample_map(self, moments=None, width=None, height=None, to_host=True, **params):
        """Sample counts for render_sampled() from the moments of temporal_accumulate() (rt_build_sample_map; DESIGN.md, "Per-pixel
        sample counts"). `moments`: the (H, W, 4) plane temporal_accumulate(moments=True) returns (through rt_build_sample_map_host),
        or None: the context's own plane of the last temporal_accumulate() of its own frame. `params`: base_samples, min_samples,
        max_samples, target_rel_error, luminance_floor (the library's defaults otherwise). Returns the (H, W) uint32 counts, or with
        to_host=False (context's own moments only) the device pointer of a plane this renderer keeps until the next such call."""
        p = RtSampleMapParams()
        self._l.rt_sample_map_params_default(C.byref(p))
        names = dict(base_samples="baseSamples", min_samples="minSamples", max_samples="maxSamples",
                     target_rel_error="targetRelError", luminance_floor="luminanceFloor")
        for k, v in params.items():
            if k not in names:
                raise TypeError(f"build_sample_map() got an unexpected parameter {k!r}")
            setattr(p, names[k], v)
        if moments is not None:
            mom = np.ascontiguousarray(moments, np.float32)
            H, W = mom.shape[:2]
            if mom.shape != (H, W, 4):
                raise ValueError(f"moments {mom.shape}: not an (H, W, 4) plane")
            out = np.empty((H, W), np.uint32)
            self._check(self._l.rt_build_sample_map_host(self._h, W, H, mom.ctypes.data, C.byref(p), out.ctypes.data), "rt_build_sample_map_host")
            return out
        H, W = (height, width) if width and height else (self._aov_shape or (0, 0))
        self.sync()   # (the plane this call reuses may still be read by a render_sampled() in flight)
        d_map = self._owned_buffer("sample_map_out", max(H * W, 1) * 4)
        self._check(self._l.rt_build_sample_map(self._h, W, H, None, C.byref(p), C.c_void_p(d_map.ptr)), "rt_build_sample_map")
        if not to_host:
            return d_map.ptr
        self.sync()
        return d_map.download((H, W), np.uint32, error="build_sample_map: the map could not be copied back")

    def sample_map_stats(self):
        """Of the last build_sample_map() (rt_sample_map_stats; blocks): samples, the sum of the counts; pixels; unknown, the pixels
        without a variance yet; aboveMin and atMax, the pixels above min_samples and at max_samples."""
        st = RtSampleMapStats()
        self._check(self._l.rt_sample_map_stats(self._h, C.byref(st)), "rt_sample_map_stats")
        return {n: getattr(st, n) for n, _ in RtSampleMapStats._fields_}

    def _device_buffer(self, name, need):
        """Device memory of at least `need` bytes under a name, kept between calls and freed with the renderer: its address."""
        return self._owned_buffer(name, need).ptr

    def _owned_buffer(self, name, need):
        """_device_buffer's DeviceBuffer, for the copies in and out."""
        b = self._owned.get(name)
        if b is None or b.nbytes < need:
            if b is not None:
                self._owned.pop(name).free()
            b = self._owned[name] = DeviceBuffer(need, name)
        return b

    def run_compute(self, pc, width, height, frames=1, **tile):
        """Frame semantics of draw()/run_compute (src/vk_engine.cpp:1782,1812-1814); `tile` = row0 / rowStride / nRows
        of rt_render when the frame is split over several GPUs. `frames` > 1 (progressive accumulation only): that many of
        the frames the loop would dispatch one after the other go in one rt_render_frames call — the same image, sooner."""
        t = pc.rayTraceParams
        if self.totalSamples >= t.sampleLimit:
            return None
        pc.frameCount = self._frameNumber
        n = 1
        if frames > 1 and t.progressive and not t.singleRender and t.raysPerPixel > 0:
            left = (t.sampleLimit - self.totalSamples + t.raysPerPixel - 1) // t.raysPerPixel
            n = max(1, min(int(frames), int(left)))
        img = self.render(pc, width, height, **tile) if n == 1 else self.render_frames(pc, width, height, n, **tile)
        if t.singleRender:
            self.totalSamples = t.sampleLimit
        else:
            self.totalSamples += t.raysPerPixel * n
        if t.progressive:
            self._frameNumber += n
        return img

    def sync(self):
        self._check(self._l.rt_sync(self._h), "rt_sync")

    def clear_framebuffer(self):
        """A new progressive history: the next render into the context's own image starts from zeros."""
        self._check(self._l.rt_clear_framebuffer(self._h), "rt_clear_framebuffer")

    def read_rgba(self):
        out = np.empty(self._shape, dtype=np.float32)
        self._check(self._l.rt_read_rgba_f32(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size),
                    "rt_read_rgba_f32")
        return out

    def read_rgba8_srgb(self):
        out = np.empty(self._shape, dtype=np.uint8)
        self._check(self._l.rt_read_rgba8_srgb(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size),
                    "rt_read_rgba8_srgb")
        return out

    def trace_rays(self, origins, dirs):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        hits = (RtHit * o.shape[0])()
        fp = C.POINTER(C.c_float)
        self._check(self._l.rt_trace_rays(self._h, o.shape[0], o.ctypes.data_as(fp), d.ctypes.data_as(fp), hits),
                    "rt_trace_rays")
        return hits

    def _query(self, what, origins, dirs, tmax, n, out, sync):
        """Both ray queries: numpy arrays through the _host entry points, device memory (objects with data_ptr(), or integer device
        pointers with n=) through the asynchronous ones."""
        rec = C.sizeof(RtHit) if what == "closest" else 1
        if not _on_device(origins, dirs):
            o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
            d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
            if d.shape != o.shape:
                raise ValueError(f"origins {o.shape} and dirs {d.shape}: not one (n, 3) pair")
            t = None if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            if t is not None and t.shape[0] != o.shape[0]:
                raise ValueError(f"tmax has {t.shape[0]} limits for {o.shape[0]} rays")
            if out is not None or not sync:
                raise ValueError("out= and sync=False go with device-pointer inputs")
            batch = RtRayBatch(o.ctypes.data, d.ctypes.data, t.ctypes.data if t is not None else None, o.shape[0])
            res = (RtHit * o.shape[0])() if what == "closest" else np.zeros(o.shape[0], np.uint8)
            fn = getattr(self._l, f"rt_query_{what}_host")
            self._check(fn(self._h, C.byref(batch), C.addressof(res) if what == "closest" else res.ctypes.data), f"rt_query_{what}_host")
            return res if what == "closest" else res.astype(bool)
        n = _device_count(origins, n, out)
        ptrs = [_device_ptr(origins, "origins", 12 * n), _device_ptr(dirs, "dirs", 12 * n),
                None if tmax is None else _device_ptr(tmax, "tmax", 4 * n)]
        batch = RtRayBatch(ptrs[0], ptrs[1], ptrs[2], n)
        fn = getattr(self._l, f"rt_query_{what}")
        self._check(fn(self._h, C.byref(batch), C.c_void_p(_device_ptr(out, "out", rec * n, floats=False))), f"rt_query_{what}")
        if sync:
            self.sync()
        return None

    def query_closest(self, origins, dirs, tmax=None, n=None, out=None, sync=True):
        """The closest hit of each of the caller's rays within its limit (rt_query_closest; DESIGN.md, "Ray queries"). (n, 3) numpy
        arrays and an optional (n,) `tmax` go through rt_query_closest_host and come back as an RtHit array (hits_to_numpy); torch
        tensors on the device (anything with data_ptr(): fp32, contiguous) or integer device pointers with n= go through the
        asynchronous entry point, the RtHit records are written to `out` (device memory, 60 bytes per ray) and sync=False is allowed."""
        return self._query("closest", origins, dirs, tmax, n, out, sync)

    def query_occluded(self, origins, dirs, tmax=None, n=None, out=None, sync=True):
        """Whether each ray hits anything nearer than its limit (rt_query_occluded): a bool array for numpy inputs, one byte per ray
        in `out` for device memory, as query_closest takes it."""
        return self._query("occluded", origins, dirs, tmax, n, out, sync)

    def query_hits(self, origins, dirs, k, tmax=None, n=None, out=None, counts=None, sync=True):
        """Every surface each ray crosses below its limit: the first `k` (0..8) in order, and how many there are (rt_query_hits;
        DESIGN.md, "All-hit ray queries"). (n, 3) numpy arrays and an optional (n,) `tmax` go through rt_query_hits_host and come
        back as (RtHit array of n * k records, ray i's at [i * k, i * k + k); uint32 array of n counts); device memory, as
        query_closest takes it, needs counts= (4 bytes per ray) and, with k > 0, out= (60 bytes per slot), and returns None."""
        k = int(k)
        if not _on_device(origins, dirs):
            o, d, t = _ray_arrays(origins, dirs, tmax)
            if out is not None or counts is not None or not sync:
                raise ValueError("out=, counts= and sync=False go with device-pointer inputs")
            batch = RtRayBatch(o.ctypes.data, d.ctypes.data, t.ctypes.data if t is not None else None, o.shape[0])
            res = (RtHit * max(o.shape[0] * k, 1))()
            cnt = np.zeros(o.shape[0], np.uint32)
            self._check(self._l.rt_query_hits_host(self._h, C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data), "rt_query_hits_host")
            return _hit_rows(res, o.shape[0], k), cnt
        if counts is None:
            raise ValueError("device-pointer inputs need counts=: device memory for the n counts")
        n = _device_count(origins, n, counts)
        if out is None and k > 0:
            raise ValueError("device-pointer inputs need out=: device memory for the n * k records")
        batch = RtRayBatch(_device_ptr(origins, "origins", 12 * n), _device_ptr(dirs, "dirs", 12 * n),
                           None if tmax is None else _device_ptr(tmax, "tmax", 4 * n), n)
        self._check(self._l.rt_query_hits(self._h, C.byref(batch), k, None if out is None else C.c_void_p(_device_ptr(out, "out", C.sizeof(RtHit) * n * k, floats=False)),
                                          C.c_void_p(_device_ptr(counts, "counts", 4 * n, floats=False))), "rt_query_hits")
        if sync:
            self.sync()
        return None

    def upload_topology(self, scene):
        """Builds the topology table of `scene` (the one uploaded) and uploads it: what query_nearest_signed needs (rt_upload_topology).
        upload_scene drops it again; update_points and update_objects keep it."""
        a = scene.arrays()
        self._check(self._l.rt_upload_topology(self._h, C.byref(a)), "rt_upload_topology")

    def query_nearest_signed(self, points, max_dist=None, n=None, out=None, side=None, sync=True):
        """query_nearest, and for each point on which side of the reported surface it lies (rt_query_nearest_signed; DESIGN.md, "Signed
        point queries"): +1 outside, -1 inside, 0 unknown or nothing found. Host arrays come back as (RtNearest array, int8 array);
        device memory (as query_nearest takes it) needs out= and side= (n bytes) and returns None."""
        rec = C.sizeof(RtNearest)
        if not _on_device(points):
            p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
            t = None if max_dist is None else np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
            if t is not None and t.shape[0] != p.shape[0]:
                raise ValueError(f"max_dist has {t.shape[0]} limits for {p.shape[0]} points")
            if out is not None or side is not None or not sync:
                raise ValueError("out=, side= and sync=False go with device-pointer inputs")
            batch = RtPointBatch(p.ctypes.data, t.ctypes.data if t is not None else None, p.shape[0])
            res = (RtNearest * p.shape[0])()
            sd = np.zeros(p.shape[0], np.int8)
            self._check(self._l.rt_query_nearest_signed_host(self._h, C.byref(batch), C.addressof(res), sd.ctypes.data), "rt_query_nearest_signed_host")
            return res, sd
        n = _device_count(points, n, out)
        if side is None:
            raise ValueError("device-pointer inputs need side=: n bytes of device memory")
        batch = RtPointBatch(_device_ptr(points, "points", 12 * n), None if max_dist is None else _device_ptr(max_dist, "max_dist", 4 * n), n)
        self._check(self._l.rt_query_nearest_signed(self._h, C.byref(batch), C.c_void_p(_device_ptr(out, "out", rec * n, floats=False)),
                                                    C.c_void_p(_device_ptr(side, "side", n, floats=False))), "rt_query_nearest_signed")
        if sync:
            self.sync()
        return None

    def query_nearest(self, points, max_dist=None, n=None, out=None, sync=True):
        """The closest surface point of each of the caller's points within its limit (rt_query_nearest; DESIGN.md, "Point queries").
        An (n, 3) numpy array and an optional (n,) `max_dist` go through rt_query_nearest_host and come back as an RtNearest array
        (nearest_to_numpy); a torch tensor on the device (anything with data_ptr(): fp32, contiguous) or an integer device pointer
        with n= goes through the asynchronous entry point, the RtNearest records are written to `out` (device memory, 16-byte
        aligned, 48 bytes per point) and sync=False is allowed."""
        rec = C.sizeof(RtNearest)
        if not _on_device(points):
            p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
            t = None if max_dist is None else np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
            if t is not None and t.shape[0] != p.shape[0]:
                raise ValueError(f"max_dist has {t.shape[0]} limits for {p.shape[0]} points")
            if out is not None or not sync:
                raise ValueError("out= and sync=False go with device-pointer inputs")
            batch = RtPointBatch(p.ctypes.data, t.ctypes.data if t is not None else None, p.shape[0])
            res = (RtNearest * p.shape[0])()
            self._check(self._l.rt_query_nearest_host(self._h, C.byref(batch), C.addressof(res)), "rt_query_nearest_host")
            return res
        n = _device_count(points, n, out)
        batch = RtPointBatch(_device_ptr(points, "points", 12 * n), None if max_dist is None else _device_ptr(max_dist, "max_dist", 4 * n), n)
        self._check(self._l.rt_query_nearest(self._h, C.byref(batch), C.c_void_p(_device_ptr(out, "out", rec * n, floats=False))), "rt_query_nearest")
        if sync:
            self.sync()
        return None

    def query_within(self, points, radius, k, n=None, out=None, counts=None, sync=True):
        """Every surface within `radius` of each point: the first `k` (0..8) nearest first, and how many there are (rt_query_within;
        DESIGN.md, "Radius point queries"). An (n, 3) numpy array and an (n,) `radius` (None: no reach, every surface counts) go
        through rt_query_within_host and come back as (RtNearest array of n * k records, point i's at [i * k, i * k + k);
        uint32 array of n counts); device memory, as query_nearest takes it, needs counts= (4 bytes per point) and, with k > 0,
        out= (48 bytes per slot, 16-byte aligned), and returns None."""
        k = int(k)
        rec = C.sizeof(RtNearest)
        if not _on_device(points):
            p, t = _point_arrays(points, radius, "radius")
            if out is not None or counts is not None or not sync:
                raise ValueError("out=, counts= and sync=False go with device-pointer inputs")
            batch = RtPointBatch(p.ctypes.data, t.ctypes.data if t is not None else None, p.shape[0])
            res = (RtNearest * max(p.shape[0] * k, 1))()
            cnt = np.zeros(p.shape[0], np.uint32)
            self._check(self._l.rt_query_within_host(self._h, C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data), "rt_query_within_host")
            return _nearest_rows(res, p.shape[0], k), cnt
        if counts is None:
            raise ValueError("device-pointer inputs need counts=: device memory for the n counts")
        n = _device_count(points, n, counts)
        if out is None and k > 0:
            raise ValueError("device-pointer inputs need out=: device memory for the n * k records")
        batch = RtPointBatch(_device_ptr(points, "points", 12 * n), None if radius is None else _device_ptr(radius, "radius", 4 * n), n)
        self._check(self._l.rt_query_within(self._h, C.byref(batch), k, None if out is None else C.c_void_p(_device_ptr(out, "out", rec * n * k, floats=False)),
                                            C.c_void_p(_device_ptr(counts, "counts", 4 * n, floats=False))), "rt_query_within")
        if sync:
            self.sync()
        return None


    def query_boxes(self, lo, hi, k, n=None, out=None, counts=None, sync=True):
        """Every surface that touches each closed axis-aligned box [lo, hi]: the first `k` (0..8) in index order (spheres, then
        objects, then triangles), and how many there are (rt_query_boxes; DESIGN.md, "Box queries"). (n, 3) numpy arrays go
        through rt_query_boxes_host and come back as (RtOverlap array of n * k records, box i's at [i * k, i * k + k)
        (overlap_to_numpy); uint32 array of n counts); device memory, as query_within takes it, needs counts= (4 bytes per box)
        and, with k > 0, out= (16 bytes per slot, 16-byte aligned), and returns None."""
        k = int(k)
        rec = C.sizeof(RtOverlap)
        if not _on_device(lo, hi):
            l, h = _box_arrays(lo, hi)
            if out is not None or counts is not None or not sync:
                raise ValueError("out=, counts= and sync=False go with device-pointer inputs")
            batch = RtBoxBatch(l.ctypes.data, h.ctypes.data, l.shape[0])
            res = (RtOverlap * max(l.shape[0] * k, 1))()
            cnt = np.zeros(l.shape[0], np.uint32)
            self._check(self._l.rt_query_boxes_host(self._h, C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data), "rt_query_boxes_host")
            return _overlap_rows(res, l.shape[0], k), cnt
        if counts is None:
            raise ValueError("device-pointer inputs need counts=: device memory for the n counts")
        n = _device_count(lo, n, counts)
        if out is None and k > 0:
            raise ValueError("device-pointer inputs need out=: device memory for the n * k records")
        batch = RtBoxBatch(_device_ptr(lo, "lo", 12 * n), _device_ptr(hi, "hi", 12 * n), n)
        self._check(self._l.rt_query_boxes(self._h, C.byref(batch), k, None if out is None else C.c_void_p(_device_ptr(out, "out", rec * n * k, floats=False)),
                                           C.c_void_p(_device_ptr(counts, "counts", 4 * n, floats=False))), "rt_query_boxes")
        if sync:
            self.sync()
        return None

    def voxelize(self, lo, hi, dims, frame=None):
        """Conservative voxelisation: how many surfaces touch each cell of the grid of dims = (nx, ny, nz) cells over the box
        [lo, hi], as a (nz, ny, nx) uint32 array. It is rt_query_boxes with k = 0 over grid_boxes(lo, hi, dims), no kernel of
        its own. Cells are closed and neighbours share their face bit for bit, so a surface lying in a shared face belongs to
        both cells (and one on a shared edge or corner to every cell around it): no surface inside the grid is lost between
        cells, and the sum of the counts is not the number of surfaces. With `frame` (16 floats, world to grid) the grid lies in
        that frame's coordinates: rt_query_oriented_boxes with sharedFrame = 1 over the same cells, which share the frame and
        their face values bit for bit."""
        nx, ny, nz = (int(d) for d in dims)
        cl, ch = grid_boxes(lo, hi, (nx, ny, nz))
        if frame is None:
            _, counts = self.query_boxes(cl, ch, 0)
        else:
            _, counts = self.query_oriented_boxes(np.asarray(frame, np.float32).reshape(16), cl, ch, 0)
        return counts.reshape(nz, ny, nx)

    def query_oriented_boxes(self, frames, lo, hi, k, n=None, out=None, counts=None, sync=True):
        """Every surface that touches each closed box { p : lo <= F p <= hi } placed by its world-to-box frame F: the first `k`
        (0..8) in index order and how many there are (rt_query_oriented_boxes; DESIGN.md, "Oriented box queries"). `frames`: (n, 16)
        matrices in RenderObject.transformMatrix's layout (obb_frames, object_frames), or one (16,) frame that the whole batch
        shares. numpy arrays go through rt_query_oriented_boxes_host and come back as query_boxes' pair; device memory needs
        counts= and, with k > 0, out=, and n= where lo cannot tell, and returns None; there a tensor of 16 floats is a shared
        frame, and an integer device pointer is taken as n frames."""
        k = int(k)
        rec = C.sizeof(RtOverlap)
        if not _on_device(frames, lo, hi):
            f, shared, l, h = _obb_arrays(frames, lo, hi)
            if out is not None or counts is not None or not sync:
                raise ValueError("out=, counts= and sync=False go with device-pointer inputs")
            batch = RtObbBatch(f.ctypes.data, l.ctypes.data, h.ctypes.data, l.shape[0], shared)
            res = (RtOverlap * max(l.shape[0] * k, 1))()
            cnt = np.zeros(l.shape[0], np.uint32)
            self._check(self._l.rt_query_oriented_boxes_host(self._h, C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data), "rt_query_oriented_boxes_host")
            return _overlap_rows(res, l.shape[0], k), cnt
        if counts is None:
            raise ValueError("device-pointer inputs need counts=: device memory for the n counts")
        n = _device_count(lo, n, counts)
        if out is None and k > 0:
            raise ValueError("device-pointer inputs need out=: device memory for the n * k records")
        # one frame for the batch: an object of 16 floats; an integer pointer is taken as n frames
        shared = 1 if hasattr(frames, "numel") and int(frames.numel()) == 16 and n != 1 else 0
        batch = RtObbBatch(_device_ptr(frames, "frames", 64 if shared else 64 * n), _device_ptr(lo, "lo", 12 * n), _device_ptr(hi, "hi", 12 * n), n, shared)
        self._check(self._l.rt_query_oriented_boxes(self._h, C.byref(batch), k, None if out is None else C.c_void_p(_device_ptr(out, "out", rec * n * k, floats=False)),
                                                    C.c_void_p(_device_ptr(counts, "counts", 4 * n, floats=False))), "rt_query_oriented_boxes")
        if sync:
            self.sync()
        return None

    def query_triangles(self, corners, k=0, n=None, out=None, counts=None, sync=True):
        """Every surface that each closed triangle of `corners` touches: the first `k` (0..8) in index order (spheres, then
        objects, then triangles), and how many there are (rt_query_triangles; DESIGN.md, "Triangle queries"). An (n, 9) or
        (n, 3, 3) numpy array (p, q, r of each triangle) goes through rt_query_triangles_host and comes back as query_boxes'
        pair; device memory, as query_boxes takes it, needs counts= (4 bytes per triangle) and, with k > 0, out= (16 bytes per
        slot, 16-byte aligned), and n= where `corners` cannot tell (numel() // 9), and returns None."""
        k = int(k)
        rec = C.sizeof(RtOverlap)
        if not _on_device(corners):
            c = _triangle_array(corners)
            if out is not None or counts is not None or not sync:
                raise ValueError("out=, counts= and sync=False go with device-pointer inputs")
            batch = RtTriangleBatch(c.ctypes.data, c.shape[0])
            res = (RtOverlap * max(c.shape[0] * k, 1))()
            cnt = np.zeros(c.shape[0], np.uint32)
            self._check(self._l.rt_query_triangles_host(self._h, C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data), "rt_query_triangles_host")
            return _overlap_rows(res, c.shape[0], k), cnt
        if counts is None:
            raise ValueError("device-pointer inputs need counts=: device memory for the n counts")
        if n is None and hasattr(corners, "numel"):
            n = int(corners.numel()) // 9
        n = _device_count(corners, n, counts)
        if out is None and k > 0:
            raise ValueError("device-pointer inputs need out=: device memory for the n * k records")
        batch = RtTriangleBatch(_device_ptr(corners, "corners", 36 * n), n)
        self._check(self._l.rt_query_triangles(self._h, C.byref(batch), k, None if out is None else C.c_void_p(_device_ptr(out, "out", rec * n * k, floats=False)),
                                               C.c_void_p(_device_ptr(counts, "counts", 4 * n, floats=False))), "rt_query_triangles")
        if sync:
            self.sync()
        return None

    def query_mesh(self, points, faces, k=0, matrix=None):
        """query_triangles for the faces of a mesh: `points` (v, 3) float32 and `faces` (f, 3) corner indices; `matrix` (16
        floats, RenderObject.transformMatrix's layout) places the points first, by mesh_corners' float32 restatement of
        rt_xform_point, so that the corners are the ones a placed object of the scene would have. numpy arrays come back as
        query_triangles' pair. Tensors on the device are gathered and placed there and come back as (records, counts): a
        (f, k, 4) and an (f,) int32 tensor holding the RtOverlap words and the counts."""
        c = mesh_corners(points, faces, matrix)
        if not hasattr(c, "data_ptr"):
            return self.query_triangles(c, k)
        import torch
        f = int(c.shape[0])
        cnt = torch.zeros(max(f, 1), dtype=torch.int32, device=c.device)
        rec = torch.zeros((max(f, 1), max(int(k), 1), 4), dtype=torch.int32, device=c.device)
        torch.cuda.synchronize(c.device)   # the gather ran on torch's stream, the query runs on the context's
        self.query_triangles(c, k, n=f, out=rec if int(k) else None, counts=cnt)
        return rec[:f, :int(k)], cnt[:f]

    def query_cuts(self, corners, k=0, n=None, out=None, counts=None, sync=True):
        """The segments along which each closed triangle of `corners` crosses the scene's triangles: the first `k` (0..8) in
        index order (object, then triangle), and how many there are (rt_query_cuts; DESIGN.md, "Triangle cuts"). An (n, 9) or
        (n, 3, 3) numpy array goes through rt_query_cuts_host and comes back as (RtCut array of n * k records, triangle i's at
        [i * k, i * k + k) (cuts_to_numpy); uint32 array of n counts); device memory, as query_triangles takes it, needs counts=
        (4 bytes per triangle) and, with k > 0, out= (48 bytes per slot, 16-byte aligned), and n= where `corners` cannot tell,
        and returns None."""
        k = int(k)
        rec = C.sizeof(RtCut)
        if not _on_device(corners):
            c = _triangle_array(corners)
            if out is not None or counts is not None or not sync:
                raise ValueError("out=, counts= and sync=False go with device-pointer inputs")
            batch = RtTriangleBatch(c.ctypes.data, c.shape[0])
            res = (RtCut * max(c.shape[0] * k, 1))()
            cnt = np.zeros(c.shape[0], np.uint32)
            self._check(self._l.rt_query_cuts_host(self._h, C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data), "rt_query_cuts_host")
            return _cut_rows(res, c.shape[0], k), cnt
        if counts is None:
            raise ValueError("device-pointer inputs need counts=: device memory for the n counts")
        if n is None and hasattr(corners, "numel"):
            n = int(corners.numel()) // 9
        n = _device_count(corners, n, counts)
        if out is None and k > 0:
            raise ValueError("device-pointer inputs need out=: device memory for the n * k records")
        batch = RtTriangleBatch(_device_ptr(corners, "corners", 36 * n), n)
        self._check(self._l.rt_query_cuts(self._h, C.byref(batch), k, None if out is None else C.c_void_p(_device_ptr(out, "out", rec * n * k, floats=False)),
                                          C.c_void_p(_device_ptr(counts, "counts", 4 * n, floats=False))), "rt_query_cuts")
        if sync:
            self.sync()
        return None

    def query_mesh_cuts(self, points, faces, k=0, matrix=None):
        """query_cuts for the faces of a mesh, gathered and placed by mesh_corners as query_mesh gathers them. numpy arrays come
        back as query_cuts' pair. Tensors on the device come back as (records, counts): an (f, k, 12) and an (f,) int32 tensor
        holding the RtCut words (the end points' bits among them) and the counts."""
        c = mesh_corners(points, faces, matrix)
        if not hasattr(c, "data_ptr"):
            return self.query_cuts(c, k)
        import torch
        f = int(c.shape[0])
        cnt = torch.zeros(max(f, 1), dtype=torch.int32, device=c.device)
        rec = torch.zeros((max(f, 1), max(int(k), 1), 12), dtype=torch.int32, device=c.device)
        torch.cuda.synchronize(c.device)   # the gather ran on torch's stream, the query runs on the context's
        self.query_cuts(c, k, n=f, out=rec if int(k) else None, counts=cnt)
        return rec[:f, :int(k)], cnt[:f]

    def query_sweep(self, origins, dirs, radius, tmax=None, n=None, out=None, sync=True):
        """The first contact of a ball of `radius` whose centre moves along each ray (rt_query_sweep; DESIGN.md, "Sphere sweeps"):
        the least t in [0, tmax) at which the centre origins + t dirs is within radius of a surface, and where. (n, 3) numpy
        origins and dirs, an (n,) `radius` and an optional (n,) `tmax` go through rt_query_sweep_host and come back as an RtSweep
        array (sweep_to_numpy); device memory, as query_closest takes it, needs out= (64 bytes per ray, 16-byte aligned), returns
        None, and sync=False is allowed."""
        if not _on_device(origins, dirs):
            o, d, rad, t = _sweep_arrays(origins, dirs, radius, tmax)
            if out is not None or not sync:
                raise ValueError("out= and sync=False go with device-pointer inputs")
            batch = RtSweepBatch(o.ctypes.data, d.ctypes.data, rad.ctypes.data, t.ctypes.data if t is not None else None, o.shape[0])
            res = (RtSweep * max(o.shape[0], 1))()
            self._check(self._l.rt_query_sweep_host(self._h, C.byref(batch), C.addressof(res)), "rt_query_sweep_host")
            return _sweep_rows(res, o.shape[0])
        n = _device_count(origins, n, out)
        batch = RtSweepBatch(_device_ptr(origins, "origins", 12 * n), _device_ptr(dirs, "dirs", 12 * n), _device_ptr(radius, "radius", 4 * n),
                             None if tmax is None else _device_ptr(tmax, "tmax", 4 * n), n)
        self._check(self._l.rt_query_sweep(self._h, C.byref(batch), C.c_void_p(_device_ptr(out, "out", C.sizeof(RtSweep) * n, floats=False))), "rt_query_sweep")
        if sync:
            self.sync()
        return None

    def query_radiance(self, origins, dirs, samples=1, bounces=8, ids=None, progressive=False, frame=0, environment=None, n=None, out=None,
                       sync=True):
        """The path-traced radiance along each of the caller's rays (rt_query_radiance; DESIGN.md, "Radiance queries"): `samples`
        paths of at most `bounces` bounces per ray, the ray's RNG state seeded from ids[i] (or i) and `frame`; `environment`: an
        EnvironmentData (a PushConstants' .environment), None = off. The directions are used as given (unit length is assumed).
        (n, 3) float32 numpy arrays (and (n,) uint32 ids) go through rt_query_radiance_host and come back as an (n, 4) float32
        array; with `progressive`, `out` is the previous result (n, 4) the new one is blended with, and is not modified. Torch
        tensors on the device (anything with data_ptr(): fp32, contiguous; ids uint32 or int32) or integer device pointers with n=
        go through the asynchronous entry point into `out` (device memory, 16 bytes per ray, the previous result when
        `progressive`), and sync=False is allowed. A wrong dtype or shape raises before the library is called."""
        if environment is not None and not isinstance(environment, _capi.EnvironmentData):
            raise TypeError("environment: an EnvironmentData (PushConstants.environment) or None")
        if int(samples) < 0 or int(bounces) < 0 or int(frame) < 0:
            raise ValueError("samples, bounces and frame are unsigned")
        p = RtRadianceParams(int(samples), int(bounces), 1 if progressive else 0, int(frame) & 0xFFFFFFFF)
        env = C.byref(environment) if environment is not None else None
        if not _on_device(origins, dirs):
            o, d = np.asarray(origins), np.asarray(dirs)
            for name, a in (("origins", o), ("dirs", d)):
                if a.dtype != np.float32:
                    raise TypeError(f"{name}: {a.dtype}, not float32")
                if a.ndim != 2 or a.shape[1] != 3:
                    raise ValueError(f"{name}: shape {a.shape}, not (n, 3)")
            if d.shape != o.shape:
                raise ValueError(f"origins {o.shape} and dirs {d.shape}: not one (n, 3) pair")
            count = o.shape[0]
            i = None
            if ids is not None:
                i = np.asarray(ids)
                if i.dtype != np.uint32:
                    raise TypeError(f"ids: {i.dtype}, not uint32")
                if i.shape != (count,):
                    raise ValueError(f"ids: shape {i.shape}, not ({count},)")
                i = np.ascontiguousarray(i)
            if not sync:
                raise ValueError("sync=False goes with device-pointer inputs")
            if out is not None and not progressive:
                raise ValueError("out= with host arrays is the previous result of a progressive query")
            if progressive:
                if out is None:
                    raise ValueError("progressive needs out=: the previous result")
                prev = np.asarray(out)
                if prev.dtype != np.float32:
                    raise TypeError(f"out: {prev.dtype}, not float32")
                if prev.shape != (count, 4):
                    raise ValueError(f"out: shape {prev.shape}, not ({count}, 4)")
                res = np.array(prev, dtype=np.float32, order="C", copy=True)
            else:
                res = np.zeros((count, 4), np.float32)
            o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
            batch = RtRayBatch(o.ctypes.data, d.ctypes.data, None, count)
            self._check(self._l.rt_query_radiance_host(self._h, C.byref(batch), i.ctypes.data if i is not None else None, C.byref(p), env,
                                                       res.ctypes.data), "rt_query_radiance_host")
            return res
        counted = n is None
        n = _device_count(origins, n, out)
        if counted and hasattr(origins, "shape") and (len(origins.shape) != 2 or origins.shape[1] != 3):
            raise ValueError(f"origins: shape {tuple(origins.shape)}, not (n, 3)")
        if hasattr(dirs, "shape") and hasattr(origins, "shape") and tuple(dirs.shape) != tuple(origins.shape):
            raise ValueError(f"origins {tuple(origins.shape)} and dirs {tuple(dirs.shape)}: not one (n, 3) pair")
        if ids is not None and hasattr(ids, "dtype") and not str(ids.dtype).endswith(("uint32", "int32")):
            raise TypeError(f"ids: {ids.dtype}, not uint32 (or int32)")
        batch = RtRayBatch(_device_ptr(origins, "origins", 12 * n), _device_ptr(dirs, "dirs", 12 * n), None, n)
        d_ids = None if ids is None else _device_ptr(ids, "ids", 4 * n, floats=False)
        self._check(self._l.rt_query_radiance(self._h, C.byref(batch), d_ids, C.byref(p), env, C.c_void_p(_device_ptr(out, "out", 16 * n))),
                    "rt_query_radiance")
        if sync:
            self.sync()
        return None

    def query_irradiance(self, points, normals, samples=64, bounces=8, ids=None, progressive=False, frame=0, bias=1e-5, environment=None,
                         n=None, out=None, sync=True):
        """The irradiance at surface points with normals (rt_query_irradiance; DESIGN.md, "Irradiance and SH probes"): E = pi x the
        mean radiance of `samples` cosine-distributed rays per point, each one path of at most `bounces` bounces, the directions
        and the paths seeded from ids[i] (or i) and `frame`; rgb and alpha 1 per point. The normals are used as given (unit
        length is assumed); the rays start at p + n * bias. (n, 3) float32 numpy arrays (and (n,) uint32 ids) go through
        rt_query_irradiance_host and come back as an (n, 4) float32 array; with `progressive`, `out` is the previous result the new
        one is blended with, and is not modified. Torch tensors on the device (anything with data_ptr(): fp32, contiguous; ids
        uint32 or int32) or integer device pointers with n= go through the asynchronous entry point into `out` (device memory, 16
        bytes per point), and sync=False is allowed. A wrong dtype or shape raises before the library is called."""
        return self._query_baked(False, points, normals, samples, bounces, ids, progressive, frame, bias, environment, n, out, sync)

    def query_sh_probes(self, points, samples=64, bounces=8, ids=None, progressive=False, frame=0, environment=None, n=None, out=None,
                        sync=True):
        """The spherical-harmonic coefficients of the radiance around free points (rt_query_sh_probes): c_j = 4 pi x the mean of
        L Y_j over `samples` rays spread on the sphere, for the nine real SH of bands 0..2 in the order 1, y, z, x, xy, yz,
        3z^2 - 1, xz, x^2 - y^2, in world axes: (n, 9, 3) float32, [j][rgb] (device form: 108 bytes per point in `out`). The
        arguments are query_irradiance's without the normals and the bias; sh9_irradiance() turns the result into irradiance."""
        return self._query_baked(True, points, None, samples, bounces, ids, progressive, frame, 0.0, environment, n, out, sync)

    def _query_baked(self, sphere, points, normals, samples, bounces, ids, progressive, frame, bias, environment, n, out, sync):
        what = "rt_query_sh_probes" if sphere else "rt_query_irradiance"
        width = 27 if sphere else 4
        if environment is not None and not isinstance(environment, _capi.EnvironmentData):
            raise TypeError("environment: an EnvironmentData (PushConstants.environment) or None")
        if int(samples) < 0 or int(bounces) < 0 or int(frame) < 0:
            raise ValueError("samples, bounces and frame are unsigned")
        p = RtIrradianceParams(int(samples), int(bounces), 1 if progressive else 0, int(frame) & 0xFFFFFFFF, float(bias))
        env = C.byref(environment) if environment is not None else None
        inputs = [("points", points)] + ([] if sphere else [("normals", normals)])
        if not _on_device(*[a for _, a in inputs]):
            arrays = [(name, np.asarray(a)) for name, a in inputs]
            for name, a in arrays:
                if a.dtype != np.float32:
                    raise TypeError(f"{name}: {a.dtype}, not float32")
                if a.ndim != 2 or a.shape[1] != 3:
                    raise ValueError(f"{name}: shape {a.shape}, not (n, 3)")
            if arrays[-1][1].shape != arrays[0][1].shape:
                raise ValueError(f"points {arrays[0][1].shape} and normals {arrays[-1][1].shape}: not one (n, 3) pair")
            count = arrays[0][1].shape[0]
            i = None
            if ids is not None:
                i = np.asarray(ids)
                if i.dtype != np.uint32:
                    raise TypeError(f"ids: {i.dtype}, not uint32")
                if i.shape != (count,):
                    raise ValueError(f"ids: shape {i.shape}, not ({count},)")
                i = np.ascontiguousarray(i)
            if not sync:
                raise ValueError("sync=False goes with device-pointer inputs")
            if out is not None and not progressive:
                raise ValueError("out= with host arrays is the previous result of a progressive query")
            shape = (count, 9, 3) if sphere else (count, 4)
            if progressive:
                if out is None:
                    raise ValueError("progressive needs out=: the previous result")
                prev = np.asarray(out)
                if prev.dtype != np.float32:
                    raise TypeError(f"out: {prev.dtype}, not float32")
                if prev.shape != shape:
                    raise ValueError(f"out: shape {prev.shape}, not {shape}")
                res = np.array(prev, dtype=np.float32, order="C", copy=True)
            else:
                res = np.zeros(shape, np.float32)
            held = [np.ascontiguousarray(a) for _, a in arrays]
            batch = RtPointNormalBatch(held[0].ctypes.data, None if sphere else held[1].ctypes.data, count)
            self._check(getattr(self._l, what + "_host")(self._h, C.byref(batch), i.ctypes.data if i is not None else None, C.byref(p), env,
                                                         res.ctypes.data), what + "_host")
            return res
        counted = n is None
        n = _device_count(points, n, out)
        if counted and hasattr(points, "shape") and (len(points.shape) != 2 or points.shape[1] != 3):
            raise ValueError(f"points: shape {tuple(points.shape)}, not (n, 3)")
        if not sphere and hasattr(normals, "shape") and hasattr(points, "shape") and tuple(normals.shape) != tuple(points.shape):
            raise ValueError(f"points {tuple(points.shape)} and normals {tuple(normals.shape)}: not one (n, 3) pair")
        if ids is not None and hasattr(ids, "dtype") and not str(ids.dtype).endswith(("uint32", "int32")):
            raise TypeError(f"ids: {ids.dtype}, not uint32 (or int32)")
        batch = RtPointNormalBatch(_device_ptr(points, "points", 12 * n), None if sphere else _device_ptr(normals, "normals", 12 * n), n)
        d_ids = None if ids is None else _device_ptr(ids, "ids", 4 * n, floats=False)
        self._check(getattr(self._l, what)(self._h, C.byref(batch), d_ids, C.byref(p), env, C.c_void_p(_device_ptr(out, "out", 4 * width * n))), what)
        if sync:
            self.sync()
        return None

    def bake_texels(self, object, width, height, out=None, stats=True, sync=True):
        """The surface point and shading normal behind every texel of a width x height map over object `object`'s uv layout
        (rt_bake_texels; DESIGN.md, "Lightmap texels"). Without `out` the records come back through rt_bake_texels_host as
        (RtTexel array of height * width records (texels_to_numpy), statistics dict). With `out` (a torch tensor on the device or
        an integer device pointer: 48 bytes per texel, 16-byte aligned) the asynchronous entry point writes there; the statistics
        dict is returned when `stats` (which waits for them), else None, and sync=False is allowed."""
        object, width, height = int(object), int(width), int(height)
        if object < 0 or width < 0 or height < 0:
            raise ValueError("object, width and height are unsigned")
        st = RtTexelStats()
        if out is None:
            if not sync:
                raise ValueError("sync=False goes with out=: device memory")
            res = (RtTexel * max(width * height, 1))()
            self._check(self._l.rt_bake_texels_host(self._h, object, width, height, C.addressof(res), C.byref(st)), "rt_bake_texels_host")
            return (RtTexel * (width * height)).from_buffer(res), _texel_stats(st)
        ptr = _device_ptr(out, "out", C.sizeof(RtTexel) * width * height, floats=False)
        self._check(self._l.rt_bake_texels(self._h, object, width, height, C.c_void_p(ptr), C.byref(st) if stats else None), "rt_bake_texels")
        if sync:
            self.sync()
        return _texel_stats(st) if stats else None

    def texels_compact(self, texels, n_texels, points, normals, index, count, sync=True):
        """The covered records of `texels` in ascending texel index as packed points, normals and their texel indices, and how
        many (rt_texels_compact): device memory throughout (tensors or integer pointers), n_texels entries' worth per array and
        one word for `count`."""
        n = int(n_texels)
        self._check(self._l.rt_texels_compact(self._h, n, C.c_void_p(_device_ptr(texels, "texels", 48 * n, floats=False)),
                                              C.c_void_p(_device_ptr(points, "points", 12 * n)), C.c_void_p(_device_ptr(normals, "normals", 12 * n)),
                                              C.c_void_p(_device_ptr(index, "index", 4 * n, floats=False)),
                                              C.c_void_p(_device_ptr(count, "count", 4, floats=False))), "rt_texels_compact")
        if sync:
            self.sync()

    def texels_scatter(self, n_texels, n_covered, index, values, rgba, fill, sync=True):
        """values[j] (4 floats) to rgba[index[j]] and fill[index[j]] = 1 for j < n_covered, every other texel 0 (rt_texels_scatter):
        device memory throughout."""
        n, k = int(n_texels), int(n_covered)
        self._check(self._l.rt_texels_scatter(self._h, n, k, C.c_void_p(_device_ptr(index, "index", 4 * k, floats=False)),
                                              C.c_void_p(_device_ptr(values, "values", 16 * k)), C.c_void_p(_device_ptr(rgba, "rgba", 16 * n)),
                                              C.c_void_p(_device_ptr(fill, "fill", n, floats=False))), "rt_texels_scatter")
        if sync:
            self.sync()

    def dilate_texels(self, width, height, passes, rgba, fill, sync=True):
        """`passes` gutter passes over a map and its fill plane in device memory, in place (rt_dilate_texels)."""
        n = int(width) * int(height)
        self._check(self._l.rt_dilate_texels(self._h, int(width), int(height), int(passes), C.c_void_p(_device_ptr(rgba, "rgba", 16 * n)),
                                             C.c_void_p(_device_ptr(fill, "fill", n, floats=False))), "rt_dilate_texels")
        if sync:
            self.sync()

    def bake_lightmap(self, object, width, height, params=None, env=None, dilate=2, out=None, fill=None, sync=True):
        """The lightmap of object `object`: the irradiance at every covered texel of a width x height map over its uv layout and
        `dilate` passes of gutter texels (rt_bake_lightmap: rt_bake_texels, rt_texels_compact, rt_query_irradiance with the texel
        indices as ids, rt_texels_scatter, rt_dilate_texels). `params`: an RtIrradianceParams (None: the defaults), `env`: an
        EnvironmentData or None. Without `out` / `fill`: ((height, width, 4) float32, (height, width) uint8 fill plane,
        statistics dict). With both (torch tensors on the device or integer device pointers, 16 bytes and 1 byte per texel) the
        map is written there and the statistics dict is returned."""
        object, width, height = int(object), int(width), int(height)
        if object < 0 or width < 0 or height < 0 or int(dilate) < 0:
            raise ValueError("object, width, height and dilate are unsigned")
        if env is not None and not isinstance(env, _capi.EnvironmentData):
            raise TypeError("env: an EnvironmentData (PushConstants.environment) or None")
        if params is None:
            params = RtIrradianceParams()
            self._l.rt_irradiance_params_default(C.byref(params))
        if (out is None) != (fill is None):
            raise ValueError("out= and fill= go together")
        st = RtTexelStats()
        n = width * height
        e = C.byref(env) if env is not None else None
        if out is None:
            if not sync:
                raise ValueError("sync=False goes with out= and fill=: device memory")
            with DeviceBuffer(16 * n, "lightmap") as d_rgba, DeviceBuffer(n, "lightmap fill") as d_fill:
                self._check(self._l.rt_bake_lightmap(self._h, object, width, height, C.byref(params), e, int(dilate), C.c_void_p(d_rgba.ptr),
                                                     C.c_void_p(d_fill.ptr), C.byref(st)), "rt_bake_lightmap")
                self.sync()
                return d_rgba.download((height, width, 4), np.float32), d_fill.download((height, width), np.uint8), _texel_stats(st)
        self._check(self._l.rt_bake_lightmap(self._h, object, width, height, C.byref(params), e, int(dilate),
                                             C.c_void_p(_device_ptr(out, "out", 16 * n)), C.c_void_p(_device_ptr(fill, "fill", n, floats=False)),
                                             C.byref(st)), "rt_bake_lightmap")
        if sync:
            self.sync()
        return _texel_stats(st)

    def render_ao(self, aovs=None, samples=4, radius=0.5, seed=0):
        """The ambient-occlusion plane of first-hit planes (rt_render_ao): `samples` cosine-weighted occlusion queries of reach
        `radius` per hit record. Without `aovs`: the context's own planes of the last render_aovs(); else the dict render_aovs()
        returns, uploaded for the call. Returns the (nRows, width) float32 plane: 1 = open, 0 = closed in."""
        p = RtAoParams(int(samples), float(radius), int(seed))
        if aovs is None:
            shape = self._aov_shape or (0, 0)
            n = shape[0] * shape[1]
            self._check(self._l.rt_render_ao(self._h, n, None, C.byref(p), None), "rt_render_ao")
        else:
            planes = numpy_to_aovs(aovs)
            shape = aovs["depth"].shape
            n = int(np.prod(shape))
            self.sync()   # (a pass still in flight may be reading the buffer this one reuses)
            d = self._owned_buffer("ao_planes", max(n, 1) * 16 * 3)
            b = RtAovBuffers()
            for i, k in enumerate(("position", "normalDepth", "ids")):
                d.upload(planes[k], offset=i * n * 16, error="render_ao: the planes could not be copied to the device")
                setattr(b, k, d.ptr + i * n * 16)
            self._check(self._l.rt_render_ao(self._h, n, C.byref(b), C.byref(p), None), "rt_render_ao")
        out = np.empty(shape, np.float32)
        self._check(self._l.rt_read_ao(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "rt_read_ao")
        return out

    def render_aovs(self, pc, width, height, row0=0, rowStride=1, nRows=None, out_ptrs=None, sync=True):
        """First-hit planes of the tile's camera rays (rt_render_aovs), for the rows render() would render. Returns the dict of
        aovs_to_numpy, arrays shaped (nRows, width[, 3]); with `out_ptrs` (device pointers keyed by the RtAovBuffers field names,
        e.g. a torch tensor's data_ptr(); planes left out are not written) the pass writes there and returns None."""
        if nRows is None:
            nRows = _tile_rows(height, row0, rowStride)
        d = None
        if out_ptrs is not None:
            unknown = set(out_ptrs) - set(AOV_PLANES)
            if unknown:
                raise KeyError(f"not an RtAovBuffers field: {sorted(unknown)}")
            d = RtAovBuffers(**{k: v for k, v in out_ptrs.items() if v})
        self.fill_counts(pc)
        self._check(self._l.rt_render_aovs(self._h, C.byref(pc), width, height, row0, rowStride, nRows,
                                           C.byref(d) if d is not None else None), "rt_render_aovs")
        if d is None:
            self._aov_shape = (nRows, width)
        if not sync:
            return None
        self.sync()
        return None if d is not None else self.read_aovs()

    def read_aovs(self):
        """The context's own planes of the last render_aovs() without `out_ptrs` (rt_read_aovs), as aovs_to_numpy gives them."""
        n, w = self._aov_shape or (0, 0)
        planes, b = _empty_planes(n, w)
        self._check(self._l.rt_read_aovs(self._h, C.byref(b), n * w), "rt_read_aovs")
        return aovs_to_numpy(planes)

    def render_guides(self, pc, width, height, max_bounces=4, first_hit=False, row0=0, rowStride=1, nRows=None):
        """Mirror-following guide planes (rt_render_guides; DESIGN.md, "Mirror-following guide planes") for the rows render() would
        render: the dict of aovs_to_numpy for the first surface that is no mirror along each pixel's chain of reflections (`depth` is
        the length of the whole path), plus `bounces`, the mirror segments before it, and `cut`, whether the chain was cut at
        `max_bounces` on a mirror. It goes to denoise() in place of render_aovs()'s. With `first_hit` the call returns
        (guides, first): `first` is what render_aovs() returns for the same tile, from the same traversal (the planes
        temporal_accumulate() takes). The context's own first-hit planes (render_aovs) are left as they are."""
        if nRows is None:
            nRows = _tile_rows(height, row0, rowStride)
        n = nRows * width
        first = None
        if first_hit:
            d_first = self._owned_buffer("first_hit", max(n, 1) * 16 * len(AOV_PLANES))   # what rt_render_guides fills beside the guides
            first = RtAovBuffers(**{k: d_first.ptr + i * n * 16 for i, k in enumerate(AOV_PLANES)})
        self.fill_counts(pc)
        self._check(self._l.rt_render_guides(self._h, C.byref(pc), width, height, row0, rowStride, nRows, int(max_bounces), None,
                                             C.byref(first) if first is not None else None), "rt_render_guides")
        planes, b = _empty_planes(nRows, width)
        self._check(self._l.rt_read_guides(self._h, C.byref(b), n), "rt_read_guides")   # (blocks: the pass is over)
        g = aovs_to_numpy(planes)
        g["bounces"], g["cut"] = (planes["ids"][..., 3] >> 8) & 15, (planes["ids"][..., 3] & 8) != 0
        if first is None:
            return g
        planes, _ = _empty_planes(nRows, width)
        for i, k in enumerate(AOV_PLANES):
            d_first.download(into=planes[k], offset=i * n * 16, error="render_guides: the first-hit planes could not be copied back")
        return g, aovs_to_numpy(planes)

    def denoise(self, frame=None, aovs=None, iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0):
        """The edge-aware a-trous denoiser (rt_denoise; DESIGN.md, "Denoising") of a whole frame: an (H, W, 4) float32 array.
        Without `frame` and `aovs` it filters the context's own frame (the last render() into it) with the context's own planes
        (the last render_aovs() without out_ptrs), both of the whole image. Otherwise `frame` is an (H, W, 4) float32 array and
        `aovs` the dict render_aovs() returns for the same image, and the call goes through rt_denoise_host."""
        p = RtDenoiseParams(int(iterations), float(sigma_luminance), float(sigma_normal), float(sigma_depth))
        if frame is None and aovs is None:
            H, W = self._aov_shape or (0, 0)
            self._check(self._l.rt_denoise(self._h, W, H, None, None, C.byref(p), None), "rt_denoise")
            out = np.empty((H, W, 4), np.float32)
            self._check(self._l.rt_read_denoised_rgba_f32(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size),
                        "rt_read_denoised_rgba_f32")
            return out
        frame, H, W, _planes, b = _frame_with_planes("denoise", frame, aovs)
        out = np.empty_like(frame)
        self._check(self._l.rt_denoise_host(self._h, W, H, frame.ctypes.data, C.byref(b), C.byref(p), out.ctypes.data),
                    "rt_denoise_host")
        return out

    def temporal_accumulate(self, pc_or_cam, frame=None, aovs=None, max_history=32, normal_cos=0.9, depth_tolerance=0.02, moments=False):
        """Temporal accumulation by reprojection (rt_temporal_accumulate; DESIGN.md, "Temporal accumulation") of a whole frame into
        the context's history: returns the accumulated (H, W, 4) float32 frame, to hand to denoise(), and with `moments` also the
        (H, W, 4) plane (m1, m2, variance, history length). `pc_or_cam` is the PushConstants (or its CameraInfo) the frame was
        rendered with. Without `frame` and `aovs` it takes the context's own frame and planes, as denoise() does; otherwise the
        (H, W, 4) array and the dict render_aovs() returns, through rt_temporal_accumulate_host. The history is the same either way."""
        cam = pc_or_cam.camInfo if isinstance(pc_or_cam, PushConstants) else pc_or_cam
        p = RtTemporalParams(int(max_history), float(normal_cos), float(depth_tolerance))
        fp = C.POINTER(C.c_float)
        if frame is None and aovs is None:
            H, W = self._aov_shape or (0, 0)
            self._check(self._l.rt_temporal_accumulate(self._h, W, H, C.byref(cam), None, None, C.byref(p), None, None), "rt_temporal_accumulate")
            out, mom = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
            self._check(self._l.rt_read_temporal_rgba_f32(self._h, out.ctypes.data_as(fp), out.size), "rt_read_temporal_rgba_f32")
            if moments:
                self._check(self._l.rt_read_temporal_moments(self._h, mom.ctypes.data_as(fp), mom.size), "rt_read_temporal_moments")
            return (out, mom) if moments else out
        frame, H, W, _planes, b = _frame_with_planes("temporal_accumulate", frame, aovs)
        out, mom = np.empty_like(frame), np.empty_like(frame)
        self._check(self._l.rt_temporal_accumulate_host(self._h, W, H, C.byref(cam), frame.ctypes.data, C.byref(b), C.byref(p), out.ctypes.data,
                                                        mom.ctypes.data), "rt_temporal_accumulate_host")
        return (out, mom) if moments else out

    def temporal_reset(self):
        """Forgets the temporal history (rt_temporal_reset): after a scene edit, or to start a new sequence."""
        self._check(self._l.rt_temporal_reset(self._h), "rt_temporal_reset")

    def temporal_track_motion(self, on):
        """Lets the temporal history follow objects and spheres that update_objects / update_spheres move between calls
        (rt_temporal_track_motion), so that such edits need no temporal_reset(). Off by default; switching forgets the history."""
        self._check(self._l.rt_temporal_track_motion(self._h, 1 if on else 0), "rt_temporal_track_motion")

    def temporal_motion_state(self):
        """What the last temporal_accumulate() treated as moved or replaced (rt_temporal_motion_state): a dict of movedObjects,
        replacedObjects and movedSpheres; all 0: it ran the static kernel."""
        v = [C.c_uint32() for _ in range(3)]
        self._check(self._l.rt_temporal_motion_state(self._h, *[C.byref(x) for x in v]), "rt_temporal_motion_state")
        return dict(movedObjects=v[0].value, replacedObjects=v[1].value, movedSpheres=v[2].value)

    def pick(self, pc, width, height, x, y):
        """What the camera ray of pixel (x, y) hits: one row of render_aovs(), the record at x (scalars and 3-vectors)."""
        if not (0 <= x < width and 0 <= y < height):
            raise ValueError(f"pixel ({x}, {y}) is outside the {width} x {height} image")
        a = self.render_aovs(pc, width, height, row0=y, rowStride=1, nRows=1)
        return {k: (v[0, x].copy() if v.ndim == 3 else v[0, x].item()) for k, v in a.items()}

    def counters(self):
        c = RtCounters()
        self._check(self._l.rt_get_counters(self._h, C.byref(c)), "rt_get_counters")
        return {n: getattr(c, n) for n, _ in RtCounters._fields_}

    def reset_counters(self):
        self._check(self._l.rt_reset_counters(self._h), "rt_reset_counters")

    def set_profiling(self, on):
        self._check(self._l.rt_set_profiling(self._h, 1 if on else 0), "rt_set_profiling")

    def trace_time_ms(self):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self._l.rt_get_trace_time_ms(self._h, C.byref(ms), C.byref(n)), "rt_get_trace_time_ms")
        return ms.value, n.value

    def trace_busy_ms(self):
        """Time during which at least one traversal launch ran (union of the launches' spans) since set_profiling(True)."""
        ms = C.c_double()
        self._check(self._l.rt_get_trace_busy_ms(self._h, C.byref(ms)), "rt_get_trace_busy_ms")
        return ms.value

    def set_tuning(self, key, value):
        self._check(self._l.rt_set_tuning(self._h, key.encode(), int(value)), "rt_set_tuning")

    def last_kernel(self):
        """Traversal kernel instantiation of the last launch, e.g. 'k_trace_pw<20, false, false, false, false, 144, 5>'."""
        return self._l.rt_last_kernel(self._h).decode()

    def last_parts(self):
        """Parts (streams) the last multi-kernel dispatch ran in."""
        return self._l.rt_last_parts(self._h)

    def last_pipeline(self):
        """0 = multi-kernel wavefront pipeline, 1 = wave-private fused pipeline."""
        return self._l.rt_last_pipeline(self._h)

    def ray_cost(self):
        """Measured box tests per executed ray of the uploaded scene (< 0: not measured yet)."""
        return self._l.rt_ray_cost(self._h)

    def bvh_last_build_ms(self):
        return self._l.rt_bvh_last_build_ms(self._h)

    def selftest(self):
        b = C.c_uint32()
        self._check(self._l.rt_device_selftest(self._h, C.byref(b)), "rt_device_selftest")
        return b.value

    # -- several GPUs, one process each: the final gather over RCCL through the C ABI (rt_comm_*) --------------
    @staticmethod
    def comm_unique_id():
        """On rank 0: the RT_COMM_ID_BYTES every rank passes to comm_init (hand them over by any means)."""
        buf = C.create_string_buffer(128)
        if _capi.lib().rt_comm_unique_id(buf) != 0:
            raise RtError("rt_comm_unique_id failed: RCCL could not be loaded")
        return buf.raw

    def comm_init(self, unique_id, n_ranks, rank):
        self._check(self._l.rt_comm_init(self._h, C.c_char_p(unique_id), int(n_ranks), int(rank)), "rt_comm_init")

    def comm_destroy(self):
        self._check(self._l.rt_comm_destroy(self._h), "rt_comm_destroy")

    def gather_strips(self, strip_ptr, width, height, root=0, frame_ptr=None):
        """This rank's strip (device pointer) -> the whole frame on `root` (device pointer there, None elsewhere)."""
        self._check(self._l.rt_gather_strips(self._h, C.c_void_p(strip_ptr), width, height, int(root),
                                             C.c_void_p(frame_ptr) if frame_ptr else None), "rt_gather_strips")

    def deinterleave_strips(self, strips_ptr, width, height, n_ranks, frame_ptr):
        """Strips of ranks 0..n_ranks-1 stored one after the other (device pointer) -> the frame's rows (device pointer)."""
        self._check(self._l.rt_deinterleave_strips(self._h, C.c_void_p(strips_ptr), width, height, int(n_ranks), C.c_void_p(frame_ptr)),
                    "rt_deinterleave_strips")

    def deinterleave_strips_host(self, strips, n_ranks):
        """[H, W, 4] float32 strips of ranks 0..n_ranks-1 one after the other -> the [H, W, 4] frame (through the device kernel)."""
        strips = np.ascontiguousarray(strips, np.float32)
        out = np.empty_like(strips)
        self._check(self._l.rt_deinterleave_strips_host(self._h, strips.ctypes.data_as(C.c_void_p), strips.shape[1], strips.shape[0], int(n_ranks),
                                                        out.ctypes.data_as(C.c_void_p)), "rt_deinterleave_strips_host")
        return out

    def math_probe(self, inputs):
        """include/rt_probe.h evaluated on the device: [n, 32] float32 -> [n, 64] float32."""
        x = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, 32)
        out = np.zeros((x.shape[0], 64), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self._l.rt_device_math_probe(self._h, x.shape[0], x.ctypes.data_as(fp), out.ctypes.data_as(fp)),
                    "rt_device_math_probe")
        return out

    def copy_bandwidth_gbps(self, nbytes=1 << 30, iters=10):
        g = C.c_double()
        self._check(self._l.rt_measure_copy_bandwidth(self._h, nbytes, iters, C.byref(g)), "copy bandwidth")
        return g.value


AOV_PLANES = ("normalDepth", "position", "albedo", "rayDir", "ids")   # the fields of RtAovBuffers


def _tile_rows(height, row0, rowStride):
    """How many of the rows row0, row0 + rowStride, ... lie in an image of `height` rows: a tile's nRows when the caller names none."""
    return (height - row0 + rowStride - 1) // rowStride


def _plane_buffers(planes):
    return RtAovBuffers(**{k: v.ctypes.data for k, v in planes.items()})


def _empty_planes(n, w):
    """An empty plane set of n rows of w records for the library to fill, and the RtAovBuffers that points into it."""
    planes = {k: np.empty((n, w, 4), np.uint32 if k == "ids" else np.float32) for k in AOV_PLANES}
    return planes, _plane_buffers(planes)


def _frame_with_planes(who, frame, aovs):
    """The host form of denoise() / temporal_accumulate(): one (H, W, 4) frame with the (H, W) planes of render_aovs() ->
    (frame as contiguous float32, H, W, the planes (kept alive by the caller), the RtAovBuffers over them)."""
    if frame is None or aovs is None:
        raise ValueError(f"{who}() takes both a frame and its AOV planes, or neither (the context's own)")
    frame = np.ascontiguousarray(frame, np.float32)
    H, W = frame.shape[:2]
    if frame.shape != (H, W, 4) or aovs["depth"].shape != (H, W):
        raise ValueError(f"frame {frame.shape} and planes {aovs['depth'].shape}: not one (H, W, 4) frame and its (H, W) planes")
    planes = numpy_to_aovs(aovs)
    return frame, H, W, planes, _plane_buffers(planes)


def _on_device(*inputs):
    """Whether a query's inputs are device memory (objects with data_ptr(), or integer device pointers) rather than host arrays."""
    on = [hasattr(x, "data_ptr") or isinstance(x, (int, np.integer)) for x in inputs]
    if any(on) and not all(on):
        raise ValueError("origins and dirs must both be host arrays or both be device memory")
    return on[0]


def _device_count(first, n, out):
    """The rules of a query on device memory: out= is needed, and n= unless the first input can tell (numel() // 3)."""
    if out is None:
        raise ValueError("device-pointer inputs need out=: device memory for the results")
    if n is None:
        if not hasattr(first, "numel"):
            raise ValueError("integer device pointers need n=")
        n = int(first.numel()) // 3
    return int(n)


def _device_ptr(x, name, nbytes, floats=True):
    """The device address behind a tensor-like object (data_ptr(); checked where it says: fp32, contiguous, large enough) or an int."""
    if isinstance(x, (int, np.integer)):
        return int(x)
    if not hasattr(x, "data_ptr"):
        raise TypeError(f"{name}: neither an integer device pointer nor an object with data_ptr()")
    if hasattr(x, "is_contiguous") and not x.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if floats and hasattr(x, "dtype") and not str(x.dtype).endswith("float32"):
        raise ValueError(f"{name}: {x.dtype}, not float32")
    if hasattr(x, "numel") and hasattr(x, "element_size") and x.numel() * x.element_size() < nbytes:
        raise ValueError(f"{name}: {x.numel() * x.element_size()} bytes, {nbytes} needed")
    return int(x.data_ptr())


def ao_rays(aovs, sample, samples=4, radius=0.5, seed=0):
    """The rays render_ao() shoots for sample `sample` of the planes `aovs` (the dict render_aovs() returns), computed on the host
    by the rule the device compiles (rt_ao_rays_host; no GPU): (origins (n, 3), dirs (n, 3), valid (n,) bool) in record order."""
    planes = numpy_to_aovs(aovs)
    n = int(np.prod(aovs["depth"].shape))
    b = RtAovBuffers(**{k: np.ascontiguousarray(planes[k]).ctypes.data for k in ("position", "normalDepth", "ids")})
    p = RtAoParams(int(samples), float(radius), int(seed))
    o, d, v = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    fp = C.POINTER(C.c_float)
    if _capi.lib().rt_ao_rays_host(n, C.byref(b), C.byref(p), int(sample), o.ctypes.data_as(fp), d.ctypes.data_as(fp),
                                   v.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise RtError("rt_ao_rays_host refused its arguments (samples 1..64, radius finite and > 0, sample < samples, at least one pixel)")
    return o, d, v.astype(bool)


def _baked_batch(points, normals, ids, samples, frame, bias, progressive=False):
    """The host structs of the baked-light rule's host forms; normals None: the probe form. Returns (batch, ids, params, held)."""
    pts = np.ascontiguousarray(points, np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points: shape {pts.shape}, not (n, 3)")
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32)
        if nrm.shape != pts.shape:
            raise ValueError(f"points {pts.shape} and normals {nrm.shape}: not one (n, 3) pair")
    i = None
    if ids is not None:
        i = np.ascontiguousarray(ids, np.uint32)
        if i.shape != (len(pts),):
            raise ValueError(f"ids: shape {i.shape}, not ({len(pts)},)")
    batch = RtPointNormalBatch(pts.ctypes.data, None if nrm is None else nrm.ctypes.data, len(pts))
    params = RtIrradianceParams(int(samples), 0, 1 if progressive else 0, int(frame) & 0xFFFFFFFF, float(bias))
    return batch, i, params, (pts, nrm)


def irradiance_rays(points, normals=None, samples=64, ids=None, frame=0, bias=1e-5, first=0, count=None):
    """The rays query_irradiance() (normals given) or query_sh_probes() (normals None) shoots for points [first, first + count) of
    the batch, computed on the host by the rule the device compiles (rt_irradiance_rays_host; no GPU): (origins (count * samples,
    3), dirs likewise, rayIds (count * samples,) uint32), ray (i - first) * samples + s being sample s of point i."""
    batch, i, params, held = _baked_batch(points, normals, ids, samples, frame, bias)
    count = batch.n - int(first) if count is None else int(count)
    rays = max(count, 0) * int(samples)
    o, d, r = np.zeros((rays, 3), np.float32), np.zeros((rays, 3), np.float32), np.zeros(rays, np.uint32)
    if _capi.lib().rt_irradiance_rays_host(C.byref(batch), None if i is None else i.ctypes.data, C.byref(params), 0 if normals is not None else 1,
                                           int(first), count, o.ctypes.data, d.ctypes.data, r.ctypes.data) != 0:
        raise RtError("rt_irradiance_rays_host refused its arguments (samples 1 .. 2^24 - 1, bias finite and >= 0, first + count <= n)")
    return o, d, r


def irradiance_gather(radiance, n, samples=64, ids=None, frame=0, sphere=False, progressive=False, out=None):
    """What the device makes of the radiance records of a batch's rays ((n * samples, 4) float32, as query_radiance() returns them
    for irradiance_rays()' rays), by the rule's weights and summation order on the host (rt_irradiance_gather_host; no GPU):
    (n, 4) irradiance, or with `sphere` (n, 9, 3) SH coefficients; with `progressive` blended with the previous result `out`
    (not modified) at weight 1 / (frame + 1)."""
    n = int(n)
    rad = np.ascontiguousarray(radiance, np.float32)
    if rad.shape != (n * int(samples), 4):
        raise ValueError(f"radiance: shape {rad.shape}, not ({n * int(samples)}, 4)")
    shape = (n, 9, 3) if sphere else (n, 4)
    if progressive:
        if out is None or np.asarray(out).shape != shape:
            raise ValueError(f"progressive needs out=: the previous result {shape}")
        res = np.array(out, dtype=np.float32, order="C", copy=True)
    else:
        res = np.zeros(shape, np.float32)
    i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    if i is not None and i.shape != (n,):
        raise ValueError(f"ids: shape {i.shape}, not ({n},)")
    batch = RtPointNormalBatch(None, None, n)
    params = RtIrradianceParams(int(samples), 0, 1 if progressive else 0, int(frame) & 0xFFFFFFFF, 0.0)
    if _capi.lib().rt_irradiance_gather_host(C.byref(batch), None if i is None else i.ctypes.data, C.byref(params), 1 if sphere else 0,
                                             rad.ctypes.data, res.ctypes.data) != 0:
        raise RtError("rt_irradiance_gather_host refused its arguments (samples 1 .. 2^24 - 1)")
    return res


def sh9_irradiance(coeffs, normals):
    """The irradiance on a surface of normal `normals` ((n, 3), or (3,) for all) under the radiance whose SH coefficients are
    `coeffs` ((n, 9, 3), query_sh_probes' order): the convolution with the clamped cosine lobe, band weights pi, 2 pi / 3, pi / 4.
    numpy, float64: (n, 3)."""
    c = np.asarray(coeffs, np.float64)
    if c.ndim != 3 or c.shape[1:] != (9, 3):
        raise ValueError(f"coeffs: shape {c.shape}, not (n, 9, 3)")
    nn = np.broadcast_to(np.asarray(normals, np.float64), (c.shape[0], 3))
    x, y, z = nn[:, 0], nn[:, 1], nn[:, 2]
    basis = np.stack([0.282095 * np.ones_like(x), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                      0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], axis=1)
    band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return np.einsum("nj,njc->nc", basis * band, c)


def _texel_stats(st):
    return dict(covered=int(st.covered), overlapped=int(st.overlapped), skippedTriangles=int(st.skippedTriangles),
                degenerateTexels=int(st.degenerateTexels))


def texels_to_numpy(recs, width=None, height=None):
    """RtTexel array (or an (n, 12) uint32 array of record words) -> dict of numpy arrays; with width and height shaped (height, width[, k])."""
    if isinstance(recs, np.ndarray):
        u = np.ascontiguousarray(recs).view(np.uint32).reshape(-1, 12)
        f = u.view(np.float32)
    else:
        f, u = _record_words(recs, RtTexel)
    d = dict(point=f[:, 0:3].copy(), state=u[:, 3].copy(), normal=f[:, 4:7].copy(), triIndex=u[:, 7].copy(), uv=f[:, 8:10].copy(), pad=u[:, 10:12].copy())
    if width is not None and height is not None:
        d = {k: v.reshape((int(height), int(width)) + v.shape[1:]) for k, v in d.items()}
    return d


def texels_exhaustive(scene_arrays, object, width, height):
    """The rule of the texel bake in plain loops over the host arrays (rt_texels_exhaustive_host; no GPU): `scene_arrays` is
    Scene.arrays(); returns (RtTexel array of height * width records (texels_to_numpy), statistics dict)."""
    width, height = int(width), int(height)
    res = (RtTexel * max(width * height, 1))()
    st = RtTexelStats()
    if _capi.lib().rt_texels_exhaustive_host(C.byref(scene_arrays), int(object), width, height, C.addressof(res), C.byref(st)) != 0:
        raise RtError("rt_texels_exhaustive_host refused its arguments (an object, a size or indices out of range, or a mesh whose triangles are not one range)")
    return (RtTexel * (width * height)).from_buffer(res), _texel_stats(st)


def dilate_texels(rgba, fill, passes):
    """`passes` gutter passes over an (H, W, 4) float32 map and its (H, W) uint8 fill plane on the host, by the rule the device
    compiles (rt_dilate_texels_host; no GPU): new arrays, the inputs are not modified."""
    out = np.array(rgba, dtype=np.float32, order="C", copy=True)
    f = np.array(fill, dtype=np.uint8, order="C", copy=True)
    if out.ndim != 3 or out.shape[2] != 4 or f.shape != out.shape[:2]:
        raise ValueError(f"rgba {out.shape} and fill {f.shape}: not one (H, W, 4) map and its (H, W) plane")
    if _capi.lib().rt_dilate_texels_host(out.shape[1], out.shape[0], int(passes), out.ctypes.data, f.ctypes.data) != 0:
        raise RtError("rt_dilate_texels_host refused its arguments (a size outside 1 .. 8192, passes > 254)")
    return out, f


def aovs_to_numpy(planes):
    """The five (nRows, width, 4) planes of rt_render_aovs (float32, ids uint32) -> named arrays shaped (nRows, width[, 3])."""
    nd, ids = planes["normalDepth"], planes["ids"]
    return dict(depth=nd[..., 3].copy(), normal=nd[..., :3].copy(), position=planes["position"][..., :3].copy(),
                albedo=planes["albedo"][..., :3].copy(), ray_dir=planes["rayDir"][..., :3].copy(), object=ids[..., 0].copy(),
                triangle=ids[..., 1].copy(), material=ids[..., 2].copy(), hit=(ids[..., 3] & 1) != 0,
                sphere=(ids[..., 3] & 2) != 0, front_face=(ids[..., 3] & 4) != 0)


def numpy_to_aovs(a):
    """The inverse of aovs_to_numpy: the named arrays of render_aovs() -> the five (H, W, 4) planes of RtAovBuffers."""
    shape = a["depth"].shape + (4,)
    planes = {k: np.zeros(shape, np.uint32 if k == "ids" else np.float32) for k in AOV_PLANES}
    planes["normalDepth"][..., :3], planes["normalDepth"][..., 3] = a["normal"], a["depth"]
    planes["position"][..., :3], planes["position"][..., 3] = a["position"], a["hit"]
    planes["albedo"][..., :3], planes["albedo"][..., 3] = a["albedo"], a["hit"]
    planes["rayDir"][..., :3] = a["ray_dir"]
    ids = planes["ids"]
    ids[..., 0], ids[..., 1], ids[..., 2] = a["object"], a["triangle"], a["material"]
    ids[..., 3] = a["hit"].astype(np.uint32) | (a["sphere"].astype(np.uint32) << 1) | (a["front_face"].astype(np.uint32) << 2)
    return planes


def _record_words(recs, ctype):
    """A ctypes array of records -> its 32-bit words, one row per record, as (float32 view, uint32 view)."""
    raw = np.frombuffer(recs, dtype=np.uint8).reshape(len(recs), C.sizeof(ctype))
    return raw.view(np.float32).reshape(len(recs), -1), raw.view(np.uint32).reshape(len(recs), -1)


def hits_to_numpy(hits):
    """RtHit array -> dict of numpy arrays."""
    f, u = _record_words(hits, RtHit)
    return dict(dst=f[:, 0].copy(), didHit=u[:, 1].copy(), isSphere=u[:, 2].copy(), objectHitIndex=u[:, 3].copy(),
                triHitIndex=u[:, 4].copy(), materialIndex=u[:, 5].copy(), frontFace=u[:, 6].copy(),
                hitPoint=f[:, 7:10].copy(), normal=f[:, 10:13].copy(), boxTests=u[:, 13].copy(),
                triTests=u[:, 14].copy())


def _ray_arrays(origins, dirs, tmax):
    """Host rays as the entry points take them: (n, 3) float32 origins and dirs and (n,) limits or None."""
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    if d.shape != o.shape:
        raise ValueError(f"origins {o.shape} and dirs {d.shape}: not one (n, 3) pair")
    t = None if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
    if t is not None and t.shape[0] != o.shape[0]:
        raise ValueError(f"tmax has {t.shape[0]} limits for {o.shape[0]} rays")
    return o, d, t


def _hit_rows(res, n, k):
    """The n * k records of an all-hit query out of the (never empty) ctypes array they were written to."""
    return (RtHit * (n * k)).from_buffer(res) if n * k else (RtHit * 0)()


def hits_walk(scene_arrays, origins, dirs, k, tmax=None, textures=None, spheres=None, objects=None):
    """The definition of the all-hit ray queries as a plain loop over the host arrays (rt_hits_walk_host; no GPU): `scene_arrays`
    is Scene.arrays(), `textures` a list of uint8 [h, w, 4] arrays in slot order as upload_textures takes them (None: no maps);
    `spheres` / `objects`: how many of the arrays' entries take part (None: all). Returns (RtHit array of n * k records, uint32
    counts), as Renderer.query_hits does for numpy inputs."""
    o, d, t = _ray_arrays(origins, dirs, tmax)
    k = int(k)
    images = [np.ascontiguousarray(im, dtype=np.uint8) for im in (textures or [])]
    tex = (RtTexture * max(len(images), 1))()
    for i, im in enumerate(images):
        if im.ndim != 3 or im.shape[2] != 4:
            raise ValueError("textures are [height, width, 4] uint8 (RGBA)")
        tex[i].width, tex[i].height = im.shape[1], im.shape[0]
        tex[i].rgba8 = im.ctypes.data_as(C.POINTER(C.c_uint8))
    batch = RtRayBatch(o.ctypes.data, d.ctypes.data, t.ctypes.data if t is not None else None, o.shape[0])
    res = (RtHit * max(o.shape[0] * k, 1))()
    cnt = np.zeros(o.shape[0], np.uint32)
    rc = _capi.lib().rt_hits_walk_host(C.byref(scene_arrays), scene_arrays.sphereCount if spheres is None else int(spheres),
                                       scene_arrays.objectCount if objects is None else int(objects), tex if images else None, len(images),
                                       C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data)
    if rc != 0:
        raise RtError("rt_hits_walk_host refused its arguments (k > 8, n >= 2^30, or arrays that index out of range)")
    return _hit_rows(res, o.shape[0], k), cnt


def nearest_to_numpy(recs):
    """RtNearest array -> dict of numpy arrays."""
    f, u = _record_words(recs, RtNearest)
    return dict(dst=f[:, 0].copy(), found=u[:, 1].copy(), isSphere=u[:, 2].copy(), objectIndex=u[:, 3].copy(), triIndex=u[:, 4].copy(),
                uv=f[:, 5:7].copy(), point=f[:, 7:10].copy())


def nearest_exhaustive(scene_arrays, points, max_dist=None):
    """The rule of the point queries in a plain loop over the host arrays (rt_nearest_exhaustive_host; no GPU, no pruning):
    `scene_arrays` is Scene.arrays(); returns an RtNearest array (nearest_to_numpy)."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    t = None if max_dist is None else np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
    if t is not None and t.shape[0] != p.shape[0]:
        raise ValueError(f"max_dist has {t.shape[0]} limits for {p.shape[0]} points")
    batch = RtPointBatch(p.ctypes.data, t.ctypes.data if t is not None else None, p.shape[0])
    res = (RtNearest * max(p.shape[0], 1))()
    if _capi.lib().rt_nearest_exhaustive_host(C.byref(scene_arrays), C.byref(batch), C.addressof(res)) != 0:
        raise RtError("rt_nearest_exhaustive_host refused its arguments (NULL arrays, n >= 2^30, or indices out of range)")
    return (RtNearest * p.shape[0]).from_buffer(res) if p.shape[0] else (RtNearest * 0)()


def _point_arrays(points, limits, name):
    """Host points as the entry points take them: (n, 3) float32 points and (n,) limits or None."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    t = None if limits is None else np.ascontiguousarray(limits, dtype=np.float32).reshape(-1)
    if t is not None and t.shape[0] != p.shape[0]:
        raise ValueError(f"{name} has {t.shape[0]} limits for {p.shape[0]} points")
    return p, t


def _nearest_rows(res, n, k):
    """The n * k records of a radius query out of the (never empty) ctypes array they were written to."""
    return (RtNearest * (n * k)).from_buffer(res) if n * k else (RtNearest * 0)()


def within_exhaustive(scene_arrays, points, radius, k):
    """The definition of the radius point queries as a plain loop over the host arrays (rt_within_exhaustive_host; no GPU, no
    pruning): `scene_arrays` is Scene.arrays(), `radius` an (n,) array or None (no reach). Returns (RtNearest array of n * k
    records (nearest_to_numpy), uint32 counts), as Renderer.query_within does for numpy inputs."""
    p, t = _point_arrays(points, radius, "radius")
    k = int(k)
    batch = RtPointBatch(p.ctypes.data, t.ctypes.data if t is not None else None, p.shape[0])
    res = (RtNearest * max(p.shape[0] * k, 1))()
    cnt = np.zeros(p.shape[0], np.uint32)
    if _capi.lib().rt_within_exhaustive_host(C.byref(scene_arrays), C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data) != 0:
        raise RtError("rt_within_exhaustive_host refused its arguments (k > 8, NULL arrays, n >= 2^30, or indices out of range)")
    return _nearest_rows(res, p.shape[0], k), cnt


def _box_arrays(lo, hi):
    """Host boxes as the entry points take them: two (n, 3) float32 arrays."""
    l = np.ascontiguousarray(lo, dtype=np.float32).reshape(-1, 3)
    h = np.ascontiguousarray(hi, dtype=np.float32).reshape(-1, 3)
    if l.shape[0] != h.shape[0]:
        raise ValueError(f"hi has {h.shape[0]} corners for {l.shape[0]} boxes")
    return l, h


def _overlap_rows(res, n, k):
    """The n * k records of a box query out of the (never empty) ctypes array they were written to."""
    return (RtOverlap * (n * k)).from_buffer(res) if n * k else (RtOverlap * 0)()


def overlap_to_numpy(recs):
    """RtOverlap array -> dict of numpy arrays."""
    u = np.frombuffer(recs, dtype=np.uint32).reshape(-1, 4) if len(recs) else np.zeros((0, 4), np.uint32)
    return dict(found=u[:, 0].copy(), isSphere=u[:, 1].copy(), objectIndex=u[:, 2].copy(), triIndex=u[:, 3].copy())


def boxes_exhaustive(scene_arrays, lo, hi, k):
    """The definition of the box queries as a plain loop over the host arrays (rt_boxes_exhaustive_host; no GPU, no pruning):
    `scene_arrays` is Scene.arrays(). Returns (RtOverlap array of n * k records (overlap_to_numpy), uint32 counts), as
    Renderer.query_boxes does for numpy inputs."""
    l, h = _box_arrays(lo, hi)
    k = int(k)
    batch = RtBoxBatch(l.ctypes.data, h.ctypes.data, l.shape[0])
    res = (RtOverlap * max(l.shape[0] * k, 1))()
    cnt = np.zeros(l.shape[0], np.uint32)
    if _capi.lib().rt_boxes_exhaustive_host(C.byref(scene_arrays), C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data) != 0:
        raise RtError("rt_boxes_exhaustive_host refused its arguments (k > 8, NULL arrays, n >= 2^30, or indices out of range)")
    return _overlap_rows(res, l.shape[0], k), cnt


def _triangle_array(corners):
    """Host triangles as the entry points take them: an (n, 9) float32 array, p, q, r of each."""
    c = np.ascontiguousarray(corners, dtype=np.float32)
    if c.size % 9:
        raise ValueError(f"corners: {c.size} numbers are not whole triangles of nine")
    return c.reshape(-1, 9)


def tris_exhaustive(scene_arrays, corners, k):
    """The definition of the triangle queries as a plain loop over the host arrays (rt_tris_exhaustive_host; no GPU, no
    pruning): `scene_arrays` is Scene.arrays(), `corners` (n, 9). Returns what boxes_exhaustive returns."""
    c = _triangle_array(corners)
    k = int(k)
    batch = RtTriangleBatch(c.ctypes.data, c.shape[0])
    res = (RtOverlap * max(c.shape[0] * k, 1))()
    cnt = np.zeros(c.shape[0], np.uint32)
    if _capi.lib().rt_tris_exhaustive_host(C.byref(scene_arrays), C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data) != 0:
        raise RtError("rt_tris_exhaustive_host refused its arguments (k > 8, NULL arrays, n >= 2^30, or indices out of range)")
    return _overlap_rows(res, c.shape[0], k), cnt


def _cut_rows(res, n, k):
    """The n * k records of a cut query out of the (never empty) ctypes array they were written to."""
    return (RtCut * (n * k)).from_buffer(res) if n * k else (RtCut * 0)()


CUT_DTYPE = np.dtype([("a", np.float32, 3), ("featA", np.uint32), ("b", np.float32, 3), ("featB", np.uint32),
                      ("found", np.uint32), ("objectIndex", np.uint32), ("triIndex", np.uint32), ("reserved", np.uint32)])


def cuts_to_numpy(recs):
    """RtCut array (or its bytes) -> a structured numpy view of CUT_DTYPE: a, featA, b, featB, found, objectIndex, triIndex,
    reserved. A view: the end points keep their bits."""
    return np.frombuffer(recs, dtype=CUT_DTYPE) if len(recs) else np.zeros(0, CUT_DTYPE)


def cuts_exhaustive(scene_arrays, corners, k):
    """The definition of the cut queries as a plain loop over the host arrays (rt_cuts_exhaustive_host; no GPU, no pruning):
    `scene_arrays` is Scene.arrays(), `corners` (n, 9). Returns what Renderer.query_cuts returns for numpy inputs."""
    c = _triangle_array(corners)
    k = int(k)
    batch = RtTriangleBatch(c.ctypes.data, c.shape[0])
    res = (RtCut * max(c.shape[0] * k, 1))()
    cnt = np.zeros(c.shape[0], np.uint32)
    if _capi.lib().rt_cuts_exhaustive_host(C.byref(scene_arrays), C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data) != 0:
        raise RtError("rt_cuts_exhaustive_host refused its arguments (k > 8, NULL arrays, n >= 2^30, or indices out of range)")
    return _cut_rows(res, c.shape[0], k), cnt


def chain_cuts(recs):
    """Joins the cuts of ONE query (cuts_to_numpy records; those with found == 0 are left out) into polylines by end points that
    are equal bit for bit, which is what the rule promises along the scene's edges. Returns (loops, chains): lists of lists of
    record indices in walking order; a loop came back to where it started, a chain has two loose ends. A cut of length zero
    is a chain of its own unless its point is an end of another cut, which it then hangs on. An end point shared by more than
    two cuts (a scene corner in the query's plane) is joined pairwise in index order."""
    r = np.asarray(recs)
    idx = [int(i) for i in np.flatnonzero(r["found"] != 0)]
    key = lambda i, end: np.ascontiguousarray(r[end][i]).view(np.uint32).tobytes()
    ends = {}
    for i in idx:
        for end in ("a", "b"):
            ends.setdefault(key(i, end), []).append((i, end))
    link = {}   # (cut, end) -> (cut, end) across a shared point
    for at in ends.values():
        at = [e for e in at if not (key(e[0], "a") == key(e[0], "b") and e[1] == "b")]   # a point cut offers one end
        for x, y in zip(at[0::2], at[1::2]):
            if x[0] != y[0]:
                link[x], link[y] = y, x
    other = {"a": "b", "b": "a"}
    seen, loops, chains = set(), [], []

    def walk(i, end):
        """from cut i, leaving through `end`: the cuts met, and whether the walk came back to i"""
        path = []
        while (i, end) in link:
            i, arrive = link[(i, end)]
            if i in seen:
                return path, True
            seen.add(i)
            path.append(i)
            end = other[arrive]
        return path, False

    for i in idx:
        if i in seen:
            continue
        seen.add(i)
        fwd, closed = walk(i, "b")
        if closed:
            loops.append([i] + fwd)
            continue
        back, _ = walk(i, "a")
        chains.append(back[::-1] + [i] + fwd)
    return loops, chains


def mesh_corners(points, faces, matrix=None):
    """The (f, 9) float32 batch of a mesh's faces: points[faces], each point first taken through `matrix` (16 floats,
    column-major) when given, as rt_xform_point takes it: ((m0 x + m4 y) + m8 z) + m12 in float32, one rounding an operation.
    numpy arrays give a numpy array; torch tensors are gathered where they live, by the same expressions."""
    if hasattr(points, "data_ptr"):
        pts, idx = points.float().reshape(-1, 3), faces.long().reshape(-1, 3)
    else:
        pts, idx = np.ascontiguousarray(points, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    if matrix is not None:
        m = [float(v) for v in np.asarray(matrix.cpu() if hasattr(matrix, "cpu") else matrix, np.float32).reshape(16)]
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        cols = [((x * m[r] + y * m[4 + r]) + z * m[8 + r]) + m[12 + r] for r in range(3)]
        pts = cols[0].new_empty((pts.shape[0], 3)) if hasattr(pts, "data_ptr") else np.empty((pts.shape[0], 3), np.float32)
        for r in range(3):
            pts[:, r] = cols[r]
    c = pts[idx].reshape(-1, 9)
    return c.contiguous() if hasattr(c, "contiguous") else np.ascontiguousarray(c, np.float32)


def _obb_arrays(frames, lo, hi):
    """Host oriented boxes as the entry points take them: (n, 16) float32 frames, or (16,) with shared = 1, and _box_arrays' two."""
    l, h = _box_arrays(lo, hi)
    f = np.ascontiguousarray(frames, dtype=np.float32)
    shared = 1 if f.ndim == 1 and f.size == 16 else 0
    f = f.reshape(-1, 16)
    if not shared and f.shape[0] != l.shape[0]:
        raise ValueError(f"{f.shape[0]} frames for {l.shape[0]} boxes")
    return f, shared, l, h


def obbs_exhaustive(scene_arrays, frames, lo, hi, k):
    """The definition of the oriented box queries as a plain loop over the host arrays (rt_obbs_exhaustive_host; no GPU, no
    pruning): `scene_arrays` is Scene.arrays(), `frames` (n, 16) or one shared (16,). Returns what boxes_exhaustive returns."""
    f, shared, l, h = _obb_arrays(frames, lo, hi)
    k = int(k)
    batch = RtObbBatch(f.ctypes.data, l.ctypes.data, h.ctypes.data, l.shape[0], shared)
    res = (RtOverlap * max(l.shape[0] * k, 1))()
    cnt = np.zeros(l.shape[0], np.uint32)
    if _capi.lib().rt_obbs_exhaustive_host(C.byref(scene_arrays), C.byref(batch), k, C.addressof(res) if k else None, cnt.ctypes.data) != 0:
        raise RtError("rt_obbs_exhaustive_host refused its arguments (k > 8, NULL arrays, sharedFrame > 1, n >= 2^30, or indices out of range)")
    return _overlap_rows(res, l.shape[0], k), cnt


def obb_frames(centres, rotations, scale=1.0):
    """The world-to-box frames, (n, 16) float32 in RenderObject.transformMatrix's layout, of boxes whose axes are the columns of
    `rotations` (n, 3, 3) about `centres` (n, 3): F p = scale R^T (p - centre), computed in float64 and rounded once. `scale`
    (a number or n of them) is local units per world unit: a box [-h, h] under it has the world half-extents h / scale."""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    R = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    if R.shape[0] != c.shape[0]:
        raise ValueError(f"{R.shape[0]} rotations for {c.shape[0]} centres")
    s = np.broadcast_to(np.asarray(scale, np.float64), (c.shape[0],))
    A = s[:, None, None] * np.transpose(R, (0, 2, 1))                  # rows of A: the box's axes
    t = -np.einsum("nij,nj->ni", A, c)
    f = np.zeros((c.shape[0], 4, 4))                                   # f[n, column, row]
    f[:, :3, :3] = np.transpose(A, (0, 2, 1))
    f[:, 3, :3] = t
    f[:, 3, 3] = 1.0
    return np.ascontiguousarray(f.reshape(-1, 16).astype(np.float32))


def object_frames(scene_arrays, objects):
    """Each listed object's inverse matrix by rt_mat4_inverse, (n, 16) float32: under it lo and hi are in that object's own
    coordinates (rt_object_frames_host)."""
    idx = np.ascontiguousarray(objects, dtype=np.uint32).reshape(-1)
    f = np.zeros((len(idx), 16), np.float32)
    if _capi.lib().rt_object_frames_host(C.byref(scene_arrays), idx.ctypes.data, len(idx), f.ctypes.data) != 0:
        raise RtError("rt_object_frames_host refused its arguments (an object index out of range)")
    return f


def frame_is_similarity(frames, tol=1e-5):
    """Per frame: whether its linear part A is a rotation or reflection times a uniform scale within `tol`: every entry of
    A^T A / s^2 - I is at most tol in size, s^2 = trace(A^T A) / 3 > 0. For those frames rt_obb_sphere is the geometry of the
    shell; for the others it is its formula."""
    f = np.asarray(frames, np.float64).reshape(-1, 4, 4)
    A = np.transpose(f[:, :3, :3], (0, 2, 1))
    G = np.einsum("nki,nkj->nij", A, A)
    s2 = np.trace(G, axis1=1, axis2=2) / 3.0
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.abs(G / s2[:, None, None] - np.eye(3)).max(axis=(1, 2))
    return (s2 > 0) & np.isfinite(off) & (off <= tol)


def grid_boxes(lo, hi, dims):
    """The cells of a grid of dims = (nx, ny, nz) over the box [lo, hi], as two (nx ny nz, 3) float32 arrays (lo, hi), x fastest.
    Per axis the N + 1 edges are computed once, e_i = float32(L + i (H - L) / N) in float64 with e_0 = L and e_N = H as float32,
    and cell i is [e_i, e_{i+1}]: neighbours share their face bit for bit."""
    L = np.asarray(lo, dtype=np.float32).reshape(3)
    H = np.asarray(hi, dtype=np.float32).reshape(3)
    n = [int(d) for d in dims]
    if len(n) != 3 or min(n) < 1:
        raise ValueError("dims is (nx, ny, nz), each at least 1")
    edges = []
    for a in range(3):
        e = (float(L[a]) + np.arange(n[a] + 1, dtype=np.float64) * (float(H[a]) - float(L[a])) / n[a]).astype(np.float32)
        e[0], e[-1] = L[a], H[a]
        edges.append(e)
    z, y, x = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    cl = np.stack([edges[0][x], edges[1][y], edges[2][z]], axis=1).astype(np.float32)
    ch = np.stack([edges[0][x + 1], edges[1][y + 1], edges[2][z + 1]], axis=1).astype(np.float32)
    return np.ascontiguousarray(cl), np.ascontiguousarray(ch)


def _sweep_arrays(origins, dirs, radius, tmax):
    """Host sweeps as the entry points take them: _ray_arrays' three and the (n,) radii."""
    o, d, t = _ray_arrays(origins, dirs, tmax)
    if radius is None:
        raise ValueError("a sweep needs its radii")
    rad = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
    if rad.shape[0] != o.shape[0]:
        raise ValueError(f"radius has {rad.shape[0]} entries for {o.shape[0]} rays")
    return o, d, rad, t


def _sweep_rows(res, n):
    """The n records of a sweep out of the (never empty) ctypes array they were written to."""
    return (RtSweep * n).from_buffer(res) if n else (RtSweep * 0)()


def sweep_to_numpy(recs):
    """RtSweep array -> dict of numpy arrays."""
    f, u = _record_words(recs, RtSweep)
    return dict(t=f[:, 0].copy(), found=u[:, 1].copy(), isSphere=u[:, 2].copy(), objectIndex=u[:, 3].copy(), triIndex=u[:, 4].copy(),
                uv=f[:, 5:7].copy(), gap=f[:, 7].copy(), point=f[:, 8:11].copy(), startsInContact=u[:, 11].copy(), normal=f[:, 12:15].copy())


def sweep_exhaustive(scene_arrays, origins, dirs, radius, tmax=None):
    """The definition of the sphere sweeps as a plain loop over the host arrays (rt_sweep_exhaustive_host; no GPU, no pruning):
    `scene_arrays` is Scene.arrays(). Returns an RtSweep array (sweep_to_numpy), as Renderer.query_sweep does for numpy inputs."""
    o, d, rad, t = _sweep_arrays(origins, dirs, radius, tmax)
    batch = RtSweepBatch(o.ctypes.data, d.ctypes.data, rad.ctypes.data, t.ctypes.data if t is not None else None, o.shape[0])
    res = (RtSweep * max(o.shape[0], 1))()
    if _capi.lib().rt_sweep_exhaustive_host(C.byref(scene_arrays), C.byref(batch), C.addressof(res)) != 0:
        raise RtError("rt_sweep_exhaustive_host refused its arguments (NULL arrays, n >= 2^30, or indices out of range)")
    return _sweep_rows(res, o.shape[0])


def scene_topology(scene_arrays):
    """rt_scene_topology on Scene.arrays() (or an edited copy of them): one dict of RtMeshTopology's fields per object."""
    n = scene_arrays.objectCount
    st = (RtMeshTopology * max(n, 1))()
    if _capi.lib().rt_scene_topology(C.byref(scene_arrays), st, n) != 0:
        raise RtError("rt_scene_topology refused its arguments (2^30 triangles or more, or indices out of range)")
    return [{k: getattr(st[i], k) for k, _ in RtMeshTopology._fields_} for i in range(n)]


def nearest_side_host(scene_arrays, points, records, features=False):
    """The side rule of the signed point queries applied to given records in a plain loop (rt_nearest_side_host; no GPU): `records`
    is an RtNearest array (query_nearest's, query_nearest_signed's or nearest_exhaustive's) for `points`; returns an int8 array.
    With `features` (rt_nearest_side_features_host): (side, feature uint8, fan uint16), the region code each point's rule met
    (255: none) and the triangles it walked around a vertex."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    if len(records) != p.shape[0]:
        raise ValueError(f"{len(records)} records for {p.shape[0]} points")
    batch = RtPointBatch(p.ctypes.data, None, p.shape[0])
    side, feat, fan = np.zeros(p.shape[0], np.int8), np.full(p.shape[0], 255, np.uint8), np.zeros(p.shape[0], np.uint16)
    if p.shape[0] and _capi.lib().rt_nearest_side_features_host(C.byref(scene_arrays), C.byref(batch), C.addressof(records), side.ctypes.data,
                                                                 feat.ctypes.data if features else None, fan.ctypes.data if features else None) != 0:
        raise RtError("rt_nearest_side_host refused its arguments (n >= 2^30, or records or arrays that index out of range)")
    return (side, feat, fan) if features else side


def signed_distance(records, side):
    """dst x side where side != 0; NaN where something was found and side == 0; RT_MISS_DST where nothing was found. `records`: an
    RtNearest array or nearest_to_numpy's dict."""
    r = records if isinstance(records, dict) else nearest_to_numpy(records)
    s = np.asarray(side, np.int8)
    d = r["dst"].astype(np.float32) * s.astype(np.float32)
    d = np.where(s == 0, np.float32(np.nan), d)
    return np.where(r["found"] == 0, np.float32(99999999.0), d).astype(np.float32)


def load_textures(scene):
    """Decodes the scene's texture files to RGBA8 the way the reference does (stbi_load(..., STBI_rgb_alpha),
    src/vk_textures.cpp:103-113: 4 channels, rows top to bottom), with PIL. A missing file raises (the reference exits)."""
    from PIL import Image
    out = []
    for path in scene.texture_paths():
        with Image.open(path) as im:
            out.append(np.asarray(im.convert("RGBA"), dtype=np.uint8))
    return out
