"""The scenes, rays and comparison rules of the float64 closest-hit tests (tests/test_closest_hit_float64.py), shared with the tests that hold other entry points to the same reference."""
import itertools
import os

import numpy as np

from ray_tracer_amd import engine, scenes

import brute_force as bf
from util import cornell_scene, seeded_rays


MAX_EXCLUDED = 0.02
MIN_MESH_HITS = 500
COARSE = 1e-3
ON_SURFACE = 1e-3     # world distance

SCENES = ("cornell", "meshes", "surface", "blob70k", "instances", "front_only")


def _aimed_rays(bs, objects, n, rng):
    """Rays from random origins in and around the Cornell box at random points of random triangles of `objects`; a third of
    them with directions of length 0.2 - 5."""
    obj = rng.choice(np.asarray(objects), size=n)
    o = rng.uniform(-1.2, 1.2, size=(n, 3))
    o[:, 1] -= 0.5
    target = np.zeros((n, 3))
    for j in np.unique(obj):
        rows = np.flatnonzero(obj == j)
        mesh, M = bs.meshes[bs.objects[j][0]], bs.objects[j][1]
        k = rng.integers(0, len(mesh.P), size=len(rows))
        w = rng.dirichlet((1.0, 1.0, 1.0), size=len(rows))
        p = np.einsum("ij,ijk->ik", w, mesh.P[k])
        target[rows] = p @ M[:3, :3].T + M[:3, 3]
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::3] *= rng.uniform(0.2, 5.0, size=(len(d[::3]), 1))
    return o.astype(np.float32), d.astype(np.float32)


def _check_placement(scene, obj, **placement):
    """The helper's own T Rx Ry Rz S against the object's matrix (rt_transform_matrix): a few float32 ulp of the largest entry."""
    ob = scene.numpy()["objects"]
    M32 = ob.view(np.float32).reshape(len(ob), -1)[obj, :16].astype(np.float64).reshape(4, 4).T
    M = bf.placement_matrix(**placement)
    assert np.abs(M32 - M).max() <= 8 * bf.U32 * max(1.0, np.abs(M).max()), (obj, np.abs(M32 - M).max())


def _obj(name):
    return os.path.join(engine.ASSET_DIR, name)


BUNNY = dict(position=(-0.45, 0.45, 0.3), rotation=(10.0, 40.0, -15.0), scale=(0.5, 0.65, 0.4))
KLEIN = dict(position=(0.35, -0.5, -0.25), rotation=(25.0, -30.0, 60.0), scale=(0.45, 0.25, 0.4))
CLOSED = dict(position=(0.45, -0.9, -0.4), rotation=(15.0, 50.0, -20.0), scale=(0.3, 0.45, 0.25))


def _meshes_scene():
    s = engine.Scene()
    s.prepare_storage_buffers()
    s.read_obj(_obj("bunny.obj"), engine.placement(samplerIndex=1, **BUNNY), 0)
    s.read_obj(_obj("klein_bottle.obj"), engine.placement(samplerIndex=1, **KLEIN), 4)
    s.set_sphere(0, (0.55, 0.2, -0.5), 0.25, 5)
    bs = bf.BruteScene.from_numpy(s.numpy())
    _check_placement(s, 9, **BUNNY)
    _check_placement(s, 10, **KLEIN)
    return s, bs


def _build(name, renderer=None):
    """(scene, brute-force scene, origins, dirs, the objects whose triangles count as mesh triangles)."""
    rng = np.random.default_rng({"cornell": 11, "meshes": 12, "surface": 13, "blob70k": 14, "instances": 15, "front_only": 16}[name])
    if name == "cornell":
        # axis-aligned and zero-component directions, origins outside the box (seeded_rays); its meshes are the two cubes
        s = cornell_scene(True)
        bs = bf.BruteScene.from_numpy(s.numpy())
        o, d = seeded_rays(4096, seed=101)
        o2, d2 = _aimed_rays(bs, [0, 1], 1500, rng)
        return s, bs, np.concatenate([o, o2]), np.concatenate([d, d2]), [0, 1]
    if name == "meshes":
        s, bs = _meshes_scene()
        o, d = _aimed_rays(bs, [9, 10], 4400, rng)
        return s, bs, o, d, [9, 10]
    if name == "surface":
        # rays that start on a surface and leave it, as shading rays do: o = hit + 1e-3 n
        s, bs = _meshes_scene()
        o, d = _aimed_rays(bs, [9, 10], 3000, rng)
        first = bs.closest_hit(o, d)
        ok = first["didHit"] & ~first["ill"]
        n = first["normal"][ok]
        v = rng.normal(size=n.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v *= np.where(np.einsum("ij,ij->i", v, n) < 0, -1.0, 1.0)[:, None]
        return s, bs, (first["hitPoint"][ok] + 1e-3 * n).astype(np.float32), v.astype(np.float32), [9, 10]
    if name == "blob70k":
        # a deep tree; on the GPU its BVH comes from the device builder. Baked in place under an identity matrix (T = 0: the
        # triangle test's own roundings alone); placed meshes are the "meshes", "instances" and "front_only" sets' business
        s = engine.Scene()
        s.prepare_storage_buffers()
        if renderer is not None:
            s.use_device_bvh(renderer)
        pos, nrm = scenes.blob(70000, seed=5, radius=0.8, center=(0.0, -0.5, 0.0))
        s.add_mesh("blob70k", pos, nrm, engine.placement(), 0)
        bs = bf.BruteScene.from_numpy(s.numpy())
        bs.replace_mesh(9, pos, nrm, False)
        _check_placement(s, 9)
        o, d = _aimed_rays(bs, [9], 1400, rng)
        return s, bs, o, d, [9]
    if name == "instances":
        # 34 identity objects, then 40 placed copies of one small mesh: the object hierarchy and the object-mask window
        s = engine.Scene()
        s.prepare_storage_buffers()
        own = {}
        for k in range(34):
            where = (-0.8 + 0.27 * (k % 7), 0.4 - 0.12 * (k // 7), -0.8 + 0.2 * (k % 5))
            pos, nrm = scenes.blob(48 + 4 * k, seed=70 + k, radius=0.06, center=where)
            own[s.counts()["objects"]] = (pos, nrm, {})
            s.add_mesh(f"i{k}", pos, nrm, engine.placement(), k % 3)
        pos, nrm = scenes.blob(120, seed=33, radius=1.0)
        placed = []
        for k in range(40):
            pl = dict(position=(-0.75 + 0.3 * (k % 6), -1.3 + 0.22 * (k // 6), -0.6 + 0.3 * (k % 4)),
                      scale=(0.08, 0.1, 0.07), rotation=(12.0 * k, 31.0 * k, 7.0 * k))
            placed.append(s.counts()["objects"])
            own[placed[-1]] = (pos, nrm, pl)
            s.add_mesh("copy", pos, nrm, engine.placement(**pl), [0, 1, 2, 4, 5][k % 5])
        assert s.counts()["objects"] == 9 + 34 + 40
        bs = bf.BruteScene.from_numpy(s.numpy())
        for j, (p, nr, pl) in own.items():
            bs.replace_mesh(j, p, nr, False)
            _check_placement(s, j, **pl)
        o, d = _aimed_rays(bs, placed, 2000, rng)
        o2, d2 = _aimed_rays(bs, sorted(set(own) - set(placed)), 600, rng)
        return s, bs, np.concatenate([o, o2]), np.concatenate([d, d2]), sorted(own)
    if name == "front_only":
        # two closed frontOnly meshes (one baked in place under an identity matrix, one placed), origins inside and outside;
        # origins on the identity mesh's bounding-box corners and faces exactly (tNear = 0), and rays that run in the plane
        # y = (a vertex's y) with d.y = 0: every node box bounded by that vertex gets (lo - o) * (1 / 0) = 0 * inf there
        s = cornell_scene(False)
        centre = np.array((-0.3, -0.4, 0.2))
        pos, nrm = scenes.blob(2000, seed=8, radius=0.4, center=tuple(centre))
        a = s.counts()["objects"]
        s.add_mesh("closed", pos, nrm, engine.placement(frontOnly=True), 1)
        pos2, nrm2 = scenes.blob(1500, seed=9, radius=1.0)
        s.add_mesh("closed2", pos2, nrm2, engine.placement(frontOnly=True, **CLOSED), 2)
        bs = bf.BruteScene.from_numpy(s.numpy())
        bs.replace_mesh(a, pos, nrm, True)
        bs.replace_mesh(a + 1, pos2, nrm2, True)
        _check_placement(s, a + 1, **CLOSED)
        flat = pos.reshape(-1, 3)
        lo, hi = flat.min(axis=0), flat.max(axis=0)                       # float32, exactly the vertices' extremes
        O, D = [], []
        o, d = _aimed_rays(bs, [a, a + 1], 1200, rng)                     # from outside (mostly)
        O.append(o); D.append(d)
        inside = np.concatenate([centre + rng.uniform(-0.12, 0.12, (500, 3)),
                                 np.asarray(CLOSED["position"]) + rng.uniform(-0.06, 0.06, (300, 3))]).astype(np.float32)
        v = rng.normal(size=inside.shape)
        O.append(inside); D.append((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
        corners = np.array(list(itertools.product(*zip(lo, hi))), np.float32)                 # 8 corners
        for c in corners:
            t = centre + rng.uniform(-0.2, 0.2, (12, 3))
            O.append(np.repeat(c[None], 12, 0)); D.append((t - c).astype(np.float32))
        for axis in range(3):                                              # on a face: that coordinate exact, the others inside
            for side in (lo, hi):
                p = rng.uniform(lo + 0.05, hi - 0.05, (40, 3)).astype(np.float32)
                p[:, axis] = side[axis]
                t = centre + rng.uniform(-0.2, 0.2, (40, 3))
                O.append(p); D.append((t - p).astype(np.float32))
        ys = flat[rng.integers(0, len(flat), 300), 1]                     # d.y = 0 at a vertex's height
        ang = rng.uniform(0, 2 * np.pi, 300)
        p = np.stack([centre[0] + 0.9 * np.cos(ang), ys, centre[2] + 0.9 * np.sin(ang)], 1).astype(np.float32)
        p[:, 1] = ys
        t = np.stack([centre[0] + rng.uniform(-0.15, 0.15, 300), ys, centre[2] + rng.uniform(-0.15, 0.15, 300)], 1)
        dd = (t - p).astype(np.float32)
        dd[:, 1] = 0.0
        O.append(p); D.append(dd)
        p = np.stack([centre[0] + rng.uniform(-0.1, 0.1, 200), ys[:200], centre[2] + rng.uniform(-0.1, 0.1, 200)], 1).astype(np.float32)
        p[:, 1] = ys[:200]                                                 # the same from inside the mesh: back faces, rejected
        dd = rng.normal(size=(200, 3)).astype(np.float32)
        dd[:, 1] = 0.0
        O.append(p); D.append(dd)
        return s, bs, np.concatenate(O), np.concatenate(D), [a, a + 1]
    raise KeyError(name)


_cases = {}


def _case(name, renderer=None):
    """The scene, its rays and their float64 answers, computed once per session (the rays do not depend on the renderer)."""
    key = (name, renderer is not None)
    if key not in _cases:
        s, bs, o, d, mesh_objects = _build(name, renderer)
        ref = bs.closest_hit(o, d)
        # A random origin now and then lands on a surface (t of a few 1e-6). Such a ray is ill-conditioned by rule (a), and the
        # coarse relative check cannot be asked of it either: float32 leaves |dt| of 1e-7 there whatever the code does. Rays that
        # start next to a surface are the "surface" set's business, which starts them 1e-3 off it; here they are dropped, by the
        # reference's own t, before any code under test has seen them, and counted as excluded under the 2 % cap.
        keep = ~(ref["didHit"] & (ref["dst"] * np.linalg.norm(d.astype(np.float64), axis=1) < ON_SURFACE))
        o, d, ref = o[keep], d[keep], {k: v[keep] for k, v in ref.items()}
        _cases[key] = (s, bs, o, d, mesh_objects, ref, int((~keep).sum()))
    return _cases[key]


def _corners_of(scene):
    a = scene.numpy()
    tp = a["triPoints"].view(np.float32).reshape(-1, 8)[:, :3].astype(np.float64)
    tr = a["triangles"].view(np.uint32).reshape(len(a["triangles"]), -1)[:, :3].astype(np.int64)
    return lambda obj, tri: tp[tr[tri.astype(np.int64)]]


def _conditions(name, ref, mesh_objects, dropped=0):
    """The cap on exclusions and the floor on mesh hits: conditions on the ray set, not on the code under test. `dropped` rays
    (origin on the surface it hits, see _case) are part of the set and of its excluded share."""
    n = len(ref["ill"]) + dropped
    good = ~ref["ill"]
    excluded = (int(ref["ill"].sum()) + dropped) / n
    mesh = good & ref["didHit"] & ~ref["isSphere"] & np.isin(ref["objectHitIndex"], mesh_objects)
    print(f"[{name}] rays {n}  well-conditioned mesh hits {int(mesh.sum())}  excluded {excluded:.4%}  "
          f"(of them {dropped} with the origin within {ON_SURFACE} of the surface hit)")
    assert excluded <= MAX_EXCLUDED, (name, excluded)
    assert mesh.sum() >= MIN_MESH_HITS, (name, int(mesh.sum()))
    return good, int(mesh.sum()), float(excluded)


def _compare(name, what, ref, got, corners_of, good):
    """All the assertions of one hit-record set against the reference. Returns the largest |dt| / bound(c = 1) on triangle hits."""
    fail, dt = bf.hits_agree(ref, got, corners_of)
    both = ref["didHit"] & got["didHit"].astype(bool)
    tri = both & good & ~ref["isSphere"]
    ratio = float((dt[tri] / ref["dst_bound_c1"][tri]).max()) if tri.any() else 0.0
    sph = both & good & ref["isSphere"]
    sratio = float((dt[sph] / ref["dst_bound"][sph]).max()) if sph.any() else 0.0
    dn = np.linalg.norm(got["normal"].astype(np.float64) - ref["normal"], axis=1)
    dp = np.linalg.norm(got["hitPoint"].astype(np.float64) - ref["hitPoint"], axis=1)
    bg = both & good
    print(f"[{name}] {what}: |dt|/bound(c=1) triangles {ratio:.3f}  spheres (full bound) {sratio:.3f}  "
          f"|dp|/bound {float((dp[bg] / ref['point_bound'][bg]).max()) if bg.any() else 0:.3f}  "
          f"|dn|/bound {float((dn[bg] / ref['normal_bound'][bg]).max()) if bg.any() else 0:.3f}  max |dn| {float(dn[bg].max()) if bg.any() else 0:.2e}")
    for k, m in fail.items():
        bad = np.flatnonzero(m & good)
        assert len(bad) == 0, f"{name} / {what}: {k} differs from the float64 reference on {len(bad)} well-conditioned rays, first {bad[:5].tolist()}"
    rel = dt[both] / ref["dst"][both]
    assert np.all(rel < COARSE), f"{name} / {what}: a ray jumped to another surface: |dt|/t up to {rel.max():.3e} at {np.flatnonzero(both)[np.argmax(rel)]}"
    return ratio


# ---------------------------------------------------------------------------------------------------------------- GPU half
KNOBS = [dict(trace_variant=v, lds_stack=l, hot_pairs=h) for v in (0, 1) for l in (8, 24) for h in (0, 2)]
DEFAULTS = dict(trace_variant=1, lds_stack=24, hot_pairs=2, object_tree_min=48)
