"""The scenes and point sets of the point-query tests (tests/test_point_queries_host.py on the CPU, tests/test_point_queries.py on
the GPU), made once per session, each with the answer of the float64 brute force (tests/nearest_float64.py).

Scenes: the Cornell box with its spheres; spheres only; Cornell + the 908-triangle bunny; four bunny instances (a rotation with a
uniform scale, the non-uniform scale (1, 0.4, 2.5), a shear, a rotation with a translation); 150 placed small objects (what the
world-box skip is for); and one mesh that is a chain of thin triangles under a comb-shaped BVH (CombScene), whose deepest leaf lies below the 24 entries of
the shallow instantiation of k_nearest_points.
Point sets, at most 4096 points a scene: uniform in twice the scene's box; points on surfaces (barycentric samples, dst ~ 0); mesh
vertices exactly (sphere poles where there is no mesh); points at distance ~1e3."""
import ctypes as C
import os

import numpy as np

from ray_tracer_amd import engine
from ray_tracer_amd._capi import BVHNode, RayMaterial, RenderObject, Sphere, Triangle, TrianglePoint

import nearest_float64 as nf
from util import EditedScene, cornell_scene, model_scene

SCENES = ("cornell", "spheres", "cornell_bunny", "instances", "placed150", "deep")
SETS = (("uniform", 768), ("surface", 384), ("vertices", 384), ("far", 128))
DEEP_MIN_DEPTH = 25

_cases = {}


def arrays_to_numpy(a):
    """Scene.numpy() for any RtSceneArrays (an EditedScene's too)."""
    def view(ptr, n, ctype):
        if n == 0:
            return np.zeros((0, C.sizeof(ctype)), dtype=np.uint8)
        buf = (ctype * n).from_address(C.addressof(ptr.contents))
        return np.frombuffer(buf, dtype=np.uint8).reshape(n, C.sizeof(ctype)).copy()
    return {"spheres": view(a.spheres, a.sphereCount, Sphere), "materials": view(a.materials, a.materialCount, RayMaterial),
            "triPoints": view(a.triPoints, a.triPointCount, TrianglePoint), "triangles": view(a.triangles, a.triangleCount, Triangle),
            "objects": view(a.objects, a.objectCount, RenderObject), "bvhNodes": view(a.bvhNodes, a.bvhNodeCount, BVHNode)}


def _flat_normals(tri):
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    return np.repeat(n[:, None, :], 3, axis=1).astype(np.float32)


def chain_mesh(n=30):
    """A strip of n thin triangles along x, each a tenth as high as it is long."""
    tri = np.zeros((n, 3, 3), np.float32)
    for k in range(n):
        tri[k] = [[0.1 * k - 1.5, -0.5, 0.0], [0.1 * k - 1.4, -0.5, 0.0], [0.1 * k - 1.45, -0.49, 0.02 * (k % 3)]]
    return tri, _flat_normals(tri)


class CombScene:
    """A one-mesh Scene whose BVH is replaced by a comb: every interior node's left child is a leaf of one triangle, its right child
    the rest of the chain, so the last leaves lie n - 1 levels down (the builder would balance a mesh this small). The boxes are
    the exact boxes of the triangles below each node, the children of a node adjacent, as the builder lays them out."""

    def __init__(self, scene):
        self.scene = scene
        a = scene.arrays()
        assert a.objectCount == 1 and a.objects[0].bvhIndex == 0
        n = a.triangleCount
        pos = np.array([[list(a.triPoints[v].position)[:3] for v in (a.triangles[t].v0, a.triangles[t].v1, a.triangles[t].v2)] for t in range(n)], np.float32)
        self.nodes = (BVHNode * (2 * n - 1))()

        def put(node, tris, index, count):
            p = pos[tris].reshape(-1, 3)
            lo, hi = p.min(axis=0), p.max(axis=0)
            node.boundsX[0], node.boundsX[1] = float(lo[0]), float(hi[0])
            node.boundsY[0], node.boundsY[1] = float(lo[1]), float(hi[1])
            node.boundsZ[0], node.boundsZ[1] = float(lo[2]), float(hi[2])
            node.index, node.triCount = index, count

        at = 0                                     # the node that holds triangles [k, n)
        for k in range(n - 1):
            put(self.nodes[at], slice(k, n), 2 * k + 1, 0)
            put(self.nodes[2 * k + 1], slice(k, k + 1), k, 1)
            at = 2 * k + 2
        put(self.nodes[at], slice(n - 1, n), n - 1, 1)
        self.depth = n - 1

    def arrays(self):
        a = self.scene.arrays()
        a.bvhNodes = C.cast(self.nodes, C.POINTER(BVHNode))
        a.bvhNodeCount = len(self.nodes)
        return a

    def counts(self):
        c = self.scene.counts()
        c["bvhNodes"] = len(self.nodes)
        return c


def _bare_scene():
    s = engine.Scene()
    s.add_material(engine.default_material(albedo=(0.7, 0.7, 0.7)))
    return s


def build_scene(name):
    """What upload_scene takes (a Scene or an EditedScene: both have arrays() and counts())."""
    if name == "cornell":
        return cornell_scene(True)
    if name == "spheres":
        s = _bare_scene()
        s.set_sphere(0, (0.3, -0.4, 0.2), 0.35, 0)
        s.set_sphere(1, (-0.5, -0.7, -0.1), 0.2, 0)
        s.set_sphere(3, (0.0, 0.4, 0.9), 0.6, 0)      # (slot 2 stays zeroed: no surface)
        return s
    if name == "cornell_bunny":
        return model_scene("bunny.obj")
    if name == "instances":
        s = _bare_scene()
        bunny = os.path.join(engine.ASSET_DIR, "bunny.obj")
        for pl in (engine.placement(position=(-0.8, 0.2, 0.1), rotation=(20, 35, 10), scale=(0.6, 0.6, 0.6)),
                   engine.placement(position=(0.7, 0.1, -0.3), scale=(1.0, 0.4, 2.5)),
                   engine.placement(position=(0.0, -0.9, 0.6)),
                   engine.placement(position=(0.1, 0.9, -0.8), rotation=(-75, 10, 130))):
            s.read_obj(bunny, pl, 0)
        e = EditedScene(s)
        m = e.objects[2].transformMatrix      # a shear: x += 0.7 y, z += -0.4 x, on top of the translation
        m[4] = 0.7
        m[2] = -0.4
        return e
    if name == "placed150":
        s = _bare_scene()
        rng = np.random.default_rng(150)
        v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32) * 0.1
        faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
        tri = np.array([[v[i], v[j], v[k]] for i, j, k in faces], np.float32)       # an octahedron: eight well-shaped faces
        for k in range(150):
            pos = ((k % 6) * 0.7 - 1.75, ((k // 6) % 5) * 0.7 - 1.4, (k // 30) * 0.7 - 1.4)
            s.add_mesh(f"small{k}", tri, _flat_normals(tri),
                       engine.placement(position=pos, rotation=tuple(rng.uniform(-90, 90, 3)), scale=tuple(rng.uniform(0.5, 1.5, 3))), 0)
        return s
    if name == "deep":
        s = _bare_scene()
        tri, nrm = chain_mesh()
        s.add_mesh("chain", tri, nrm, engine.placement(), 0)
        comb = CombScene(s)
        assert comb.depth >= DEEP_MIN_DEPTH
        return comb
    raise KeyError(name)


def point_sets(ns, seed):
    """name -> (n, 3) float32, from the float64 scene alone; and the float64 answer of the uniform set."""
    rng = np.random.default_rng(seed)
    lo, hi = ns.box()
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    out = {}
    n = dict(SETS)
    # uniform in twice the box, less the points so near a surface that a limit of 0.999 or 1.001 x their distance would lie within
    # the float32 bound of it (the limits run on this set; the surface and vertex sets are the ones with dst ~ 0): candidates are
    # dropped on the float64 answer alone, 1e-3 dst < 4 bound, and the first n kept
    cand = (mid + rng.uniform(-2, 2, (2 * n["uniform"], 3)) * half).astype(np.float32)
    ref = nf.nearest(ns, cand)
    keep = np.flatnonzero(1e-3 * ref["dst"] >= 4 * ref["bound"])[:n["uniform"]]
    assert len(keep) == n["uniform"], f"only {len(keep)} of {len(cand)} candidates keep clear of the surfaces"
    out["uniform"] = cand[keep]
    uniform_ref = {k: v[keep] for k, v in ref.items()}
    if len(ns.W):
        t = rng.integers(0, len(ns.W), n["surface"])
        b = rng.dirichlet((1, 1, 1), n["surface"])
        out["surface"] = np.einsum("pk,pkd->pd", b, ns.W[t]).astype(np.float32)
        out["vertices"] = ns.W[rng.integers(0, len(ns.W), n["vertices"]), rng.integers(0, 3, n["vertices"])].astype(np.float32)
    else:
        d = rng.normal(size=(n["surface"], 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        k = rng.integers(0, len(ns.sph_c), n["surface"])
        out["surface"] = (ns.sph_c[k] + ns.sph_r[k, None] * d).astype(np.float32)
        k = rng.integers(0, len(ns.sph_c), n["vertices"])
        pole = np.eye(3)[rng.integers(0, 3, n["vertices"])] * rng.choice([-1.0, 1.0], (n["vertices"], 1))
        out["vertices"] = (ns.sph_c[k] + ns.sph_r[k, None] * pole).astype(np.float32)
    d = rng.normal(size=(n["far"], 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out["far"] = (mid + d * rng.uniform(800, 1200, (n["far"], 1))).astype(np.float32)
    return out, uniform_ref


def case(name):
    """dict(scene, arrays (numpy), ns (NearestScene), sets: name -> points, ref: name -> nearest_float64.nearest())."""
    if name not in _cases:
        scene = build_scene(name)
        arrays = arrays_to_numpy(scene.arrays())
        ns = nf.NearestScene.from_numpy(arrays)
        sets, uniform_ref = point_sets(ns, 7000 + SCENES.index(name))
        ref = {k: (uniform_ref if k == "uniform" else nf.nearest(ns, p)) for k, p in sets.items()}
        _cases[name] = dict(scene=scene, arrays=arrays, ns=ns, sets=sets, ref=ref)
    return _cases[name]


def check_records(c, points, rec, ref, what):
    """The float64 rules for `rec` (nearest_to_numpy of records that all found something) against ref = nearest() of the same
    points; returns the largest |dst - ref| / bound(C = 1)."""
    ns = c["ns"]
    q = points.astype(np.float64)
    assert rec["found"].all(), f"{what}: {int((rec['found'] == 0).sum())} points found nothing"
    err = np.abs(rec["dst"].astype(np.float64) - ref["dst"])
    assert (err <= ref["bound"]).all(), f"{what}: |dst - ref| up to {float((err / ref['bound']).max()):.3g} bounds"
    p = rec["point"].astype(np.float64)
    gap = np.abs(np.linalg.norm(p - q, axis=1) - rec["dst"])
    assert (gap <= ref["bound"]).all(), f"{what}: | |point - q| - dst | up to {float((gap / ref['bound']).max()):.3g} bounds"
    u, v = rec["uv"][:, 0].astype(np.float64), rec["uv"][:, 1].astype(np.float64)
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1 + 4 * nf.U32).all(), f"{what}: barycentrics outside the triangle"
    sph = rec["isSphere"].astype(bool)
    assert (rec["uv"][sph] == 0).all() and (rec["triIndex"][sph] == 0).all()
    d_own, b_own, W = nf.distance_to_reported(ns, points, sph, rec["objectIndex"], rec["triIndex"])
    assert (d_own - b_own <= ref["upper"]).all(), f"{what}: a reported primitive is not within the bound of the minimum"
    rebuilt = (1 - u - v)[:, None] * W[:, 0] + u[:, None] * W[:, 1] + v[:, None] * W[:, 2]
    off = np.linalg.norm(rebuilt - p, axis=1)[~sph]
    assert (off <= b_own[~sph]).all(), f"{what}: point is not w a + u b + v c of the reported triangle"
    return float((err / ref["unit"]).max())
