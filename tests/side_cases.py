"""The scenes and point sets of the signed point-query tests (tests/test_signed_queries_host.py on the CPU,
tests/test_signed_queries.py on the GPU), made once per session, each with the float64 answers of tests/nearest_float64.py and the
components of tests/side_float64.py.

Scenes: `cubes`, cube.obj three times: rotated, under the non-uniform scale (1, 0.4, 2.5), mirrored (scale x = -1, det < 0);
`torus`, a 24 x 12 torus (576 triangles) under the shear x += 0.7 y, z += -0.4 x; `torus_flipped`, the same with a seeded third of
its triangles stored reversed (same points, same answers); `spikes`, an octahedron with every face raised to a sharp apex (24
triangles: at its vertices and edges a face normal alone gives the wrong sign, asserted below); `mixed`, the Cornell box (open
quads), the 908-triangle bunny (not manifold) and spheres; `klein`, klein_bottle.obj (closed, not orientable); `spheres`, the
spheres-only scene of tests/point_query_cases.py with a point at a centre and points exactly on poles.
Point sets, at most 1024 points each: `uniform` in 1.5 x the scene's box; `features`, mesh vertices and edge midpoints pushed
+- 0.02 x the box diagonal along the float64 pseudo-normal (the vertex and edge branches are rare in a uniform set); `inside`,
points the reference keeps as inside."""
import os

import numpy as np

from ray_tracer_amd import engine

import nearest_float64 as nf
import side_float64 as sf
from point_query_cases import _bare_scene, _flat_normals, arrays_to_numpy
from util import EditedScene, model_scene

SCENES = ("cubes", "torus", "torus_flipped", "spikes", "mixed", "klein", "spheres")
N_UNIFORM, N_FEATURES, N_INSIDE = 768, 512, 256
FLIP_SEED = 11

_cases = {}


def torus_mesh(nu=24, nv=12, R=1.0, r=0.4, radial=None):
    """[nu * nv * 2, 3, 3] float32, outward. `radial`: a function of the ring angles (u, v) that scales the tube's radius (the
    deformation of the update test: coincident points move alike because it is a function of the grid node)."""
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    U, V = np.meshgrid(u, v, indexing="ij")
    rr = r * (radial(U, V) if radial is not None else 1.0)
    P = np.stack([(R + rr * np.cos(V)) * np.cos(U), (R + rr * np.cos(V)) * np.sin(U), rr * np.sin(V)], axis=-1).astype(np.float32)
    tri = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = P[i, j], P[(i + 1) % nu, j], P[(i + 1) % nu, (j + 1) % nv], P[i, (j + 1) % nv]
            tri += [[a, b, c], [a, c, d]]
    return np.array(tri, np.float32)


def flipped(tri, seed=FLIP_SEED):
    """A seeded third of the triangles stored with corners 1 and 2 swapped; returns (mesh, which)."""
    which = np.random.default_rng(seed).random(len(tri)) < 1 / 3
    out = tri.copy()
    out[which] = tri[which][:, [0, 2, 1]]
    return out, which


def spikes_mesh(apex=1.3):
    tri = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                X, Y, Z, A = (sx, 0, 0), (0, sy, 0), (0, 0, sz), (apex * sx, apex * sy, apex * sz)
                face = (X, Y, Z) if sx * sy * sz > 0 else (X, Z, Y)
                for k in range(3):
                    tri.append([face[k], face[(k + 1) % 3], A])
    return np.array(tri, np.float32)


def _sheared(scene, index=0):
    e = EditedScene(scene)
    m = e.objects[index].transformMatrix      # x += 0.7 y, z += -0.4 x
    m[4] = 0.7
    m[2] = -0.4
    return e


def build_scene(name, torus=None):
    if name == "cubes":
        s = _bare_scene()
        cube = os.path.join(engine.ASSET_DIR, "cube.obj")
        for pl in (engine.placement(position=(-3.0, 0.2, 0.1), rotation=(20, 35, 10)),
                   engine.placement(position=(0.0, 0.0, 0.0), scale=(1.0, 0.4, 2.5)),
                   engine.placement(position=(3.0, -0.1, 0.3), rotation=(0, 15, 0), scale=(-1.0, 1.0, 1.0))):
            s.read_obj(cube, pl, 0)
        return s
    if name in ("torus", "torus_flipped"):
        s = _bare_scene()
        tri = torus_mesh() if torus is None else torus
        if name == "torus_flipped":
            tri, _ = flipped(tri)
        s.add_mesh(name, tri, _flat_normals(tri), engine.placement(), 0)
        return _sheared(s)
    if name == "spikes":
        s = _bare_scene()
        tri = spikes_mesh()
        s.add_mesh("spikes", tri, _flat_normals(tri), engine.placement(rotation=(12, -25, 40), scale=(0.8, 0.8, 0.8)), 0)
        return s
    if name == "mixed":
        return model_scene("bunny.obj", spheres=True)
    if name == "klein":
        s = _bare_scene()
        s.read_obj(os.path.join(engine.ASSET_DIR, "klein_bottle.obj"), engine.placement(rotation=(10, 20, 30)), 0)
        return s
    if name == "spheres":
        s = _bare_scene()
        s.set_sphere(0, (0.3, -0.4, 0.2), 0.35, 0)
        s.set_sphere(1, (-0.5, -0.7, -0.1), 0.2, 0)
        s.set_sphere(3, (0.0, 0.4, 0.9), 0.6, 0)      # (slot 2 stays zeroed: no surface)
        return s
    raise KeyError(name)


def ref_records(ns, ref):
    """The float64 minimiser of every point as a record (what truth() takes)."""
    tri = ~ref["sphere"]
    idx = ref["index"]
    return dict(found=np.ones(len(idx), np.uint32), isSphere=ref["sphere"].astype(np.uint32),
                objectIndex=np.where(tri, ns.obj[np.where(tri, idx, 0)] if len(ns.obj) else 0, ns.sph_index[np.where(tri, 0, idx)] if len(ns.sph_index) else 0).astype(np.uint32),
                triIndex=(np.where(tri, ns.tri[np.where(tri, idx, 0)], 0) if len(ns.tri) else np.zeros(len(idx))).astype(np.uint32))


def _nearest(ns, points):
    return nf.nearest(ns, points, chunk=32 if len(ns.W) > 5000 else 256)


def point_sets(name, ns, ss, arrays, seed):
    rng = np.random.default_rng(seed)
    lo, hi = ns.box()
    mid, half, diag = (lo + hi) / 2, (hi - lo) / 2, float(np.linalg.norm(hi - lo))
    big = len(ns.W) > 5000                                    # klein: the float64 brute force is 36 000 triangles a point
    out = {"uniform": (mid + rng.uniform(-1.5, 1.5, (64 if big else N_UNIFORM, 3)) * half).astype(np.float32)}
    if name == "spheres":
        poles = np.concatenate([ns.sph_c + ns.sph_r[:, None] * np.eye(3)[k] * s for k in range(3) for s in (1.0, -1.0)])
        out["features"] = np.concatenate([ns.sph_c, poles]).astype(np.float32)     # a point at every centre, points exactly on poles
    elif not big:
        n, vn, W = ss.unit_normals(), ss.vertex_normals(), ns.W
        live = np.flatnonzero(ss.component_of >= 0)
        t = rng.choice(live, N_FEATURES // 4)
        k = rng.integers(0, 3, len(t))
        corner, normal = W[t, k], vn[ss.weld[t, k]]
        mids, en = [], []
        for ti, ki in zip(rng.choice(live, N_FEATURES // 4), rng.integers(0, 3, N_FEATURES // 4)):
            others = ss.neighbours.get((int(ti), int(ki)), [])
            mids.append((W[ti, ki] + W[ti, (ki + 1) % 3]) / 2)
            en.append(n[ti] + (n[others[0][0]] if others else 0.0))
        base, N = np.concatenate([corner, np.array(mids)]), np.concatenate([normal, np.array(en)])
        N = N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-12)
        out["features"] = np.concatenate([base + 0.02 * diag * N, base - 0.02 * diag * N]).astype(np.float32)
    if not big:
        cand = (mid + rng.uniform(-1.0, 1.0, (4096, 3)) * half).astype(np.float32)
        ref = _nearest(ns, cand)
        rec = ref_records(ns, ref)
        t = ss.truth(cand, rec, ref)
        inside = t["kept"] & (t["expected"] == -1)
        if len(ns.sph_c):
            side, sph = sf.sphere_sides(arrays, cand, rec)
            inside |= sph & (side == -1)
        if inside.any():
            out["inside"] = cand[inside][:N_INSIDE]
    return out


def case(name):
    """dict(scene, arrays (numpy), ns (NearestScene), ss (SideScene), sets: name -> points, ref: name -> nearest_float64.nearest())."""
    if name not in _cases:
        scene = build_scene(name)
        arrays = arrays_to_numpy(scene.arrays())
        ns = nf.NearestScene.from_numpy(arrays)
        ss = sf.SideScene(arrays, ns)
        if name == "torus_flipped":                            # the unflipped scene's points: every side has to equal its
            sets = case("torus")["sets"]
        else:
            sets = point_sets(name, ns, ss, arrays, 9100 + SCENES.index(name))
        ref = {k: _nearest(ns, p) for k, p in sets.items()}
        _cases[name] = dict(scene=scene, arrays=arrays, ns=ns, ss=ss, sets=sets, ref=ref)
        if name == "spikes":
            _spikes_earn_their_place(_cases[name])
    return _cases[name]


def _spikes_earn_their_place(c):
    """The float64 face-normal rule (the sign of (q - p) . n of the nearest triangle alone) is wrong on at least one kept point."""
    wrong = 0
    n = c["ss"].unit_normals()
    for k, points in c["sets"].items():
        ref = c["ref"][k]
        t = c["ss"].truth(points, ref_records(c["ns"], ref), ref)
        d = points.astype(np.float64) - ref["point"]
        face = np.where(np.einsum("pk,pk->p", d, n[ref["index"]]) > 0, 1, -1)
        wrong += int((t["kept"] & t["signable"] & (face != t["expected"])).sum())
    assert wrong > 0, "spikes: the face normal alone is right everywhere: the scene does not test the pseudo-normal"
    c["face_normal_wrong"] = wrong


def check_sides(c, points, rec, side, ref, what):
    """The float64 rules for `side` (int8) beside `rec` (nearest_to_numpy): every kept point's side is the winding number's where
    the reported triangle's component is signable and 0 where it is not; spheres exactly; nothing found: 0; at most CAP of the
    points excluded. Returns the truth dict with `excluded`."""
    t = c["ss"].truth(points, rec, ref)
    side = np.asarray(side).astype(np.int64)
    tri = (rec["found"] != 0) & (rec["isSphere"] == 0)
    excluded = tri & ~t["kept"]
    assert excluded.mean() <= sf.CAP, f"{what}: {excluded.mean():.2%} of the points are excluded, above the cap"
    bad = np.flatnonzero(t["kept"] & (side != t["expected"]))
    assert len(bad) == 0, (f"{what}: {len(bad)} kept points on the wrong side, first {bad[:5].tolist()}: side {side[bad[:5]].tolist()}, "
                           f"expected {t['expected'][bad[:5]].tolist()}, w {t['w'][bad[:5]].tolist()}, |cos| {t['cosine'][bad[:5]].tolist()}")
    want, sph = sf.sphere_sides(c["arrays"], points, rec)
    assert np.array_equal(side[sph], want[sph].astype(np.int64)), f"{what}: a sphere's side differs from the float32 rule"
    assert not side[rec["found"] == 0].any(), f"{what}: a point that found nothing has a side"
    t["excluded"] = excluded
    return t
