"""Shared helpers for the parity tests."""
import contextlib

import numpy as np

from ray_tracer_amd import devmem, engine, scenes


def cornell_scene(spheres=True):
    s, _ = scenes.cornell(spheres)
    return s


def model_scene(obj, material=0, scale=0.7, position=(0.0, 0.53, 0.0), spheres=False):
    """Default Cornell box + one of the small OBJ assets that ship in assets/."""
    import os
    s = engine.Scene()
    s.prepare_storage_buffers()
    s.read_obj(os.path.join(engine.ASSET_DIR, obj), engine.placement(position=position, scale=scale, samplerIndex=1), material)
    if spheres:
        s.set_sphere(0, (0.55, 0.2, -0.5), 0.25, 5)
    return s


def seeded_rays(n, seed, box=1.2):
    """Rays that start inside/around the Cornell box and point everywhere."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-box, box, size=(n, 3)).astype(np.float32)
    o[:, 1] -= 0.5
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # a few axis-aligned and zero-component directions (inf in invDir)
    d[0] = (0, 0, 1); d[1] = (1, 0, 0); d[2] = (0, -1, 0); d[3] = (0, 1, 0)
    o[4] = (0, -0.5, -3.5); d[4] = (0, 0, 1)
    return o, d.astype(np.float32)


def bits(a):
    """An array as uint32 words: what bit-for-bit comparisons are taken on (NaNs and signed zeros compare by their bits)."""
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """Whether two arrays (of any dtype) have one dtype, one shape and the same bytes."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_bits(a, b, what="arrays"):
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"
    if not same_bits(a, b):
        x, y = (bits(a), bits(b)) if a.dtype == np.float32 else (a, b)
        raise AssertionError(f"{what} differs at {np.argwhere(x != y)[:5].tolist()}")


def assert_hits_equal(a, b):
    """Two RtHit dict-of-arrays must agree bit for bit."""
    for k in a:
        assert_same_bits(a[k], b[k], f"field {k}")


def code_object():
    """tools/code_object.py (what the library's gfx950 code object says about its kernels) as a module."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "code_object.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def kernel_instantiations(names):
    """The instantiations in the library of the kernel templates `names` (a regular expression), read from its symbol table."""
    import re
    import subprocess
    from ray_tracer_amd import _capi
    out = subprocess.run(["nm", "-C", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return set(re.findall(rf"__device_stub__({names}<[^>]*>)", out))


class EditedScene:
    """A Scene whose materials / spheres / objects arrays have been edited in place, the way the reference's ImGui panels
    edit the host vectors before "Update Buffer" (src/vk_engine.cpp:1536-1618): ctypes copies of the three arrays that the
    test mutates, handed to rt_update_* and, as the same RtSceneArrays, to the oracle."""

    def __init__(self, scene):
        import ctypes as C
        from ray_tracer_amd._capi import RayMaterial, RenderObject, Sphere
        self.scene = scene
        a = scene.arrays()
        self.materials = (RayMaterial * max(a.materialCount, 1))()
        self.objects = (RenderObject * max(a.objectCount, 1))()
        self.spheres = (Sphere * max(a.sphereCount, 1))()
        C.memmove(self.materials, a.materials, C.sizeof(RayMaterial) * a.materialCount)
        C.memmove(self.objects, a.objects, C.sizeof(RenderObject) * a.objectCount)
        C.memmove(self.spheres, a.spheres, C.sizeof(Sphere) * a.sphereCount)
        self.nMaterials, self.nObjects, self.nSpheres = a.materialCount, a.objectCount, a.sphereCount

    def arrays(self):
        import ctypes as C
        from ray_tracer_amd._capi import RayMaterial, RenderObject, Sphere
        a = self.scene.arrays()
        a.materials = C.cast(self.materials, C.POINTER(RayMaterial))
        a.objects = C.cast(self.objects, C.POINTER(RenderObject))
        a.spheres = C.cast(self.spheres, C.POINTER(Sphere))
        return a

    def counts(self):
        return self.scene.counts()

    def set_transform(self, i, placement):
        """objects[i].transformMatrix = T*Rx*Ry*Rz*S of the placement (src/vk_engine.cpp:1597-1601)."""
        import ctypes as C
        from ray_tracer_amd import _capi
        _capi.lib().rt_transform_matrix(C.byref(placement), self.objects[i].transformMatrix)

    def push(self, renderer, what):
        """update_buffer for one of the arrays (src/vk_engine.cpp:1545,1572,1603)."""
        l, h = renderer._l, renderer._h
        if what == "materials":
            renderer._check(l.rt_update_materials(h, self.materials, self.nMaterials), "rt_update_materials")
        elif what == "objects":
            renderer._check(l.rt_update_objects(h, self.objects, self.nObjects), "rt_update_objects")
        elif what == "spheres":
            renderer._check(l.rt_update_spheres(h, self.spheres, self.nSpheres), "rt_update_spheres")
        else:
            raise KeyError(what)


def random_emitter_scene(seed):
    """The bare Cornell box plus random small meshes and spheres, several of them emissive, under random placements: the
    stress scenes of the light queries (emitters in front of, behind and inside other things, emissive spheres, more than one
    emissive mesh). Returns (scene, push constants, width, height)."""
    rng = np.random.default_rng(4000 + seed)
    s = cornell_scene(False)
    mats = [0, 1, 2, 4, 5]
    for _ in range(2):
        mats.append(s.add_material(engine.default_material(albedo=tuple(rng.random(3)), emissionColor=tuple(rng.random(3)),
                                                            emissionStrength=float(rng.random() * 3 + 0.1))))
    for k in range(int(rng.integers(2, 6))):
        n = int(rng.integers(1, 9))
        tri = rng.uniform(-0.8, 0.8, (n, 3, 3)).astype(np.float32)
        tri[:, :, 1] -= 0.5
        tri[:, 1:, :] = tri[:, :1, :] + rng.uniform(-0.35, 0.35, (n, 2, 3)).astype(np.float32)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)
        pl = engine.placement(rotation=tuple(rng.uniform(-40, 40, 3)), scale=tuple(rng.uniform(0.6, 1.2, 3))) if rng.random() < 0.5 else engine.placement()
        s.add_mesh(f"e{seed}_{k}", tri, np.repeat(nrm[:, None, :], 3, axis=1).astype(np.float32), pl, int(rng.choice(mats)))
    for i in range(int(rng.integers(0, 5))):
        s.set_sphere(i, tuple(rng.uniform(-0.7, 0.7, 3)), float(rng.uniform(0.05, 0.3)), int(rng.choice(mats)))
    W, H = 80, 60
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=int(rng.integers(2, 9)), environmentOn=bool(seed % 2))
    return s, pc, W, H


def _mesh_triangles(scene, obj):
    """The point indices (n, 3) of the triangles of the mesh of object `obj`."""
    a = scene.numpy()
    nodes = a["bvhNodes"].view(np.uint32).reshape(-1, 8)
    tri = a["triangles"].view(np.uint32).reshape(-1, 12)[:, :3]
    root = int(a["objects"].view(np.uint32).reshape(-1, 20)[obj, 17])
    stack, used = [root], []
    while stack:
        n = stack.pop()
        index, count = int(nodes[n, 6]), int(nodes[n, 7])
        if count:
            used.append(tri[index:index + count])
        else:
            stack += [index, index + 1]
    return np.concatenate(used)


def _mesh_points(scene, obj):
    """The point indices the mesh of object `obj` uses, as a range [lo, hi)."""
    used = _mesh_triangles(scene, obj)
    return int(used.min()), int(used.max()) + 1


def _smooth(points, seed, amp):
    """A seeded smooth displacement of positions (and a tilt of the normals and a shift of the uvs)."""
    rng = np.random.default_rng(seed)
    k, ph = rng.uniform(2.0, 7.0, (3, 3)), rng.uniform(0, 6.28, 3)
    p = points.copy()
    p[:, :3] += (amp * np.sin(points[:, :3].astype(np.float64) @ k.T + ph)).astype(np.float32)
    p[:, 4:7] += (0.2 * np.cos(points[:, :3].astype(np.float64) @ k + ph)).astype(np.float32)
    p[:, 3] += np.float32(0.01)
    return p


# ---------------------------------------------------------------------------------------------------------------- float64
def _deformed_bunny():
    s = model_scene("bunny.obj")
    lo, hi = _mesh_points(s, s.counts()["objects"] - 1)
    return s, _smooth(s.points()[lo:hi], 31, 0.06), lo


def emitters_scene():
    """Cornell with an emissive sphere, glass right under the ceiling light and a second light coplanar with the ceiling (also the
    "emitters" case of tests/test_paths_float64.py)."""
    s = cornell_scene(True)
    glow = s.add_material(engine.default_material(albedo=(0.1, 0.1, 0.1), emissionColor=(0.3, 0.6, 1.0), emissionStrength=1.2))
    s.set_sphere(3, (-0.6, -0.9, 0.4), 0.2, glow)
    s.set_sphere(4, (0.1, -1.3, 0.0), 0.25, 5)       # glass right under the ceiling light
    quad = np.array([[[-0.2, -1.5, 0.5], [0.2, -1.5, 0.5], [0.2, -1.5, 0.8]], [[-0.2, -1.5, 0.5], [0.2, -1.5, 0.8], [-0.2, -1.5, 0.8]]], np.float32)
    nq = np.zeros_like(quad); nq[..., 1] = 1
    s.add_mesh("coplanar_light", quad, nq, engine.placement(), glow)   # in the plane of the ceiling: equal distances
    return s


@contextlib.contextmanager
def device_buffers(names, nbytes, fill=None):
    """name -> a devmem.DeviceBuffer of `nbytes` the test owns, every byte set to `fill` first (so that what the library did not
    write shows) and that fill waited for; freed when the block ends."""
    bufs = {}
    try:
        for k in names:
            bufs[k] = devmem.DeviceBuffer(nbytes)
            if fill is not None:
                bufs[k].fill(fill)
        devmem.synchronize()
        yield bufs
    finally:
        for b in bufs.values():
            b.free()


def to_device(renderer, name, a):
    """The array in a named device buffer of the renderer's own (Renderer._device_buffer: kept and freed with it): its address.
    renderer._owned[name] is the buffer, for reading it back."""
    a = np.ascontiguousarray(a)
    p = renderer._device_buffer(name, max(a.nbytes, 1))
    renderer._owned[name].upload(a)
    return p


def progressive_frames(renderer, s, W, H, after_frame=None):
    """Three progressive frames after a render_aovs() of the same image, with `after_frame(pc)` (a post pass, or nothing) run
    behind each: the frames, the counters each one added, and the state of the launch policy at the end. A pass that leaves
    rendering alone gives the same three with and without it."""
    renderer.upload_scene(s)
    renderer.clear_framebuffer()
    pc = engine.push_constants(W, H, progressive=1, raysPerPixel=2)
    renderer.render_aovs(pc, W, H)
    frames, deltas = [], []
    for k in range(3):
        pc.frameCount = k
        before = renderer.counters()
        frames.append(renderer.render(pc, W, H))
        after = renderer.counters()
        deltas.append({n: after[n] - before[n] for n in after})
        if after_frame:
            after_frame(pc)
    renderer.sync()
    return frames, deltas, (renderer.ray_cost(), renderer.last_pipeline(), renderer.last_parts(), renderer.last_kernel())


def frames_between_passes(renderer, s, W, H, passes=None):
    """Three progressive frames with `passes(other, W + 24, H + 16)` run before each: side passes of another camera over a bigger
    image, so that the path state grows. Returns what progressive_frames returns, without the kernel's name."""
    renderer.upload_scene(s)
    renderer.clear_framebuffer()
    pc = engine.push_constants(W, H, progressive=1, raysPerPixel=2)
    other = engine.push_constants(W + 24, H + 16, cameraAngles=(15.0, 40.0, 0.0), pos=(0.2, -0.6, -2.5))
    frames, deltas = [], []
    for k in range(3):
        if passes:
            passes(other, W + 24, H + 16)
        pc.frameCount = k
        before = renderer.counters()
        frames.append(renderer.render(pc, W, H))
        after = renderer.counters()
        deltas.append({n: after[n] - before[n] for n in after})
    renderer.sync()
    return frames, deltas, (renderer.ray_cost(), renderer.last_pipeline(), renderer.last_parts())
