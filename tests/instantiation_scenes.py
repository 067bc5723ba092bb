"""The scenes that reach every traversal kernel instantiation (tests/test_instantiations.py), shared with the tests that render them again."""
import numpy as np

from ray_tracer_amd import engine


def _normals(tri):
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    return np.repeat(n[:, None, :], 3, axis=1).astype(np.float32)


def soup(n, seed, size=0.02):
    """n small triangles scattered in the Cornell volume: a balanced BVH of depth ~ log2 n."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.6, 0.6, (n, 1, 3)).astype(np.float32)
    c[:, :, 1] -= 0.4
    tri = c + rng.uniform(-size, size, (n, 3, 3)).astype(np.float32)
    return tri, _normals(tri)


def skewed(n, p, seed):
    """Centroids u**p: the binned builder keeps cutting a sparse tail off a dense corner, which gives a deep, lopsided tree."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (n, 1, 3))
    c = (u ** p * 0.6).astype(np.float32)
    c[:, :, 1] -= 0.5
    tri = c + rng.uniform(-1e-4, 1e-4, (n, 3, 3)).astype(np.float32) * c.max(axis=2, keepdims=True).clip(1e-3)
    tri = tri.astype(np.float32)
    return tri, _normals(tri)


def build_scene(mesh, placed):
    """The mesh under an identity placement, lit by the environment and a small emitter at the NEE rectangle; `placed`: two more
    small meshes under general transforms, which is what makes the library pick its CULL kernels (rt_update_objects)."""
    s = engine.Scene()
    glow = s.add_material(engine.default_material(albedo=(0, 0, 0), emissionColor=(1, 0.9, 0.8), emissionStrength=3.0))
    grey = s.add_material(engine.default_material(albedo=(0.7, 0.7, 0.75)))
    mirror = s.add_material(engine.default_material(albedo=(1, 1, 1), reflectance=1.0))
    tri, nrm = mesh()
    s.add_mesh("main", tri, nrm, engine.placement(), grey)
    depth = s.last_bvh_stats()["maxDepth"]
    quad = np.array([[[-0.3, -1.5, -0.3], [0.3, -1.5, -0.3], [0.3, -1.5, 0.3]], [[-0.3, -1.5, -0.3], [0.3, -1.5, 0.3], [-0.3, -1.5, 0.3]]], np.float32)
    s.add_mesh("light", quad, np.tile(np.array([0, 1, 0], np.float32), (2, 3, 1)), engine.placement(), glow)
    floor = quad.copy() * 4
    floor[:, :, 1] = 0.5
    s.add_mesh("floor", floor, np.tile(np.array([0, -1, 0], np.float32), (2, 3, 1)), engine.placement(), grey)
    if placed:
        t2, n2 = soup(40, 77, 0.1)
        s.add_mesh("placed_a", t2, n2, engine.placement(position=(0.5, 0.1, 0.2), rotation=(20, 35, 10), scale=(0.4, 0.5, 0.4)), mirror)
        s.add_mesh("placed_b", t2, n2, engine.placement(position=(-0.5, 0.0, -0.1), rotation=(-15, 70, 5), scale=(0.5, 0.4, 0.6)), grey)
    s.grey = grey
    return s, depth


def _same(img, cnt, ref, rc, what):
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{what}: pixels differ from the oracle's"
    for k in ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests"):
        assert cnt[k] == rc[k], f"{what}: counter {k}: gpu {cnt[k]} oracle {rc[k]}"
    assert rc["lightQueryMismatch"] == 0
