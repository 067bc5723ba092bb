"""Deforming meshes in place on the GPU (rt_upload_scene_dynamic, rt_update_points; DESIGN.md, "Deforming meshes").

Context A is upload_scene(dynamic=True) followed by update_points; context B a fresh upload_scene of the host scene after
Scene.update_points; the oracle runs on B's arrays. All three must agree bit for bit: trace_rays (per-ray boxTests / triTests
included), render in both pipelines with hot_pairs 0 and 2 (and equal RtCounters), render_aovs. On the bunny A is also held to
brute_force.BruteScene built from the deformed points, exactly as test_closest_hit_float64.py holds the static scene. No-op
updates, the refusals through the ABI, and the temporal pass (the refit mesh's objects are "replaced") follow."""
import os

import numpy as np
import pytest

from ray_tracer_amd import engine, scenes
from oracle import pyoracle
import brute_force as bf
from closest_hit_cases import ON_SURFACE, _aimed_rays, _compare, _conditions, _corners_of
from util import _deformed_bunny, _mesh_points, _mesh_triangles, _smooth, assert_hits_equal, cornell_scene, model_scene, same_bits, seeded_rays

pytestmark = pytest.mark.gpu

W, H = 64, 48
SCENES = ("cornell", "cube", "bunny", "instances", "emissive", "blob")
DEFORMATIONS = ("smooth_all", "sub_range", "grow", "twice")
COUNTERS = ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests")


def _obj(name):
    return os.path.join(engine.ASSET_DIR, name)


def _scene(name):
    """(scene, tuning the scene is uploaded and rendered with)."""
    if name == "cornell":        # its meshes are root leaves of 2 triangles, the light among them
        return cornell_scene(True), {}
    if name == "cube":
        s = cornell_scene(False)
        s.read_obj(_obj("cube.obj"), engine.placement(position=(0.1, 0.3, 0.1), rotation=(20.0, 35.0, -10.0), scale=(0.3, 0.45, 0.25)), 1)
        return s, {}
    if name == "bunny":
        return model_scene("bunny.obj"), {}
    if name == "instances":      # one mesh, two objects: one identity, one rotated and scaled; the object hierarchy from one object on
        s = cornell_scene(False)
        s.read_obj(_obj("bunny.obj"), engine.placement(), 0)
        s.read_obj(_obj("bunny.obj"), engine.placement(position=(0.35, 0.5, -0.2), rotation=(15.0, 60.0, -25.0), scale=(0.5, 0.7, 0.4)), 2)
        return s, dict(object_tree_min=1)
    if name == "emissive":       # an emissive mesh of the emitter list, and a leaf of 100 triangles (one centroid: the builder cannot split it)
        s = cornell_scene(False)
        m = s.add_material(engine.default_material(albedo=(0, 0, 0), emissionColor=(1.0, 0.8, 0.6), emissionStrength=3.0))
        quad = np.array([[(-0.3, -0.2, 0.1), (0.1, -0.2, 0.1), (0.1, 0.1, 0.3)], [(-0.3, -0.2, 0.1), (0.1, 0.1, 0.3), (-0.3, 0.1, 0.3)]], np.float32)
        nq = np.cross(quad[:, 1] - quad[:, 0], quad[:, 2] - quad[:, 0])
        nq /= np.linalg.norm(nq, axis=1, keepdims=True)
        s.add_mesh("glow", quad, np.repeat(nq[:, None], 3, 1).astype(np.float32), engine.placement(rotation=(0.0, 20.0, 0.0)), m)
        # every triangle of the fan has the centroid c, exactly: corners c + a, c + b, c - a - b on a grid of 1 / 64
        ang = np.linspace(0.0, np.pi, 100, endpoint=False)
        c = np.array((0.25, -0.625, -0.25))
        a = np.round(16 * np.stack([np.cos(ang), np.sin(ang), 0.3 * np.cos(3 * ang)], 1)) / 64
        b = np.round(16 * np.stack([-np.sin(ang), 0.5 * np.cos(ang), 0.6 + 0.3 * np.sin(2 * ang)], 1)) / 64
        fan = np.stack([c + a, c + b, c - a - b], 1).astype(np.float32)
        nf = np.cross(fan[:, 1] - fan[:, 0], fan[:, 2] - fan[:, 0])
        nf /= np.linalg.norm(nf, axis=1, keepdims=True)
        s.add_mesh("fan", fan, np.repeat(nf[:, None], 3, 1).astype(np.float32), engine.placement(), 1)
        return s, {}
    if name == "blob":           # 6000 triangles: levels of more than 256 interior nodes, which take one launch each
        s = cornell_scene(False)
        pos, nrm = scenes.blob(6000, seed=21, radius=0.45, center=(0.0, 0.0, 0.0))
        s.add_mesh("blob6k", pos, nrm, engine.placement(position=(0.05, -0.45, 0.1), rotation=(0.0, 30.0, 10.0), scale=(1.0, 0.8, 1.1)), 2)
        return s, {}
    raise KeyError(name)


def _widest_level(scene, obj):
    """The largest number of interior nodes at one depth of the mesh of object `obj`."""
    a = scene.numpy()
    nodes = a["bvhNodes"].view(np.uint32).reshape(-1, 8)
    level, widest = [int(a["objects"].view(np.uint32).reshape(-1, 20)[obj, 17])], 0
    while level:
        interior = [n for n in level if nodes[n, 7] == 0]
        widest = max(widest, len(interior))
        level = [c for n in interior for c in (int(nodes[n, 6]), int(nodes[n, 6]) + 1)]
    return widest


def _updates(scene, deformation, seed):
    """The (points, first) updates of a deformation, and the object whose mesh it grows (or None)."""
    pts = scene.points()
    last = scene.counts()["objects"] - 1
    lo, hi = _mesh_points(scene, last)
    sub = lambda base, s: (_smooth(base[lo + (hi - lo) // 3:lo + (hi - lo) // 3 + max(1, (hi - lo) // 3)], s, 0.05), lo + (hi - lo) // 3)   # noqa: E731
    if deformation == "smooth_all":
        return [(_smooth(pts, seed, 0.04), 0)], None
    if deformation == "sub_range":
        return [sub(pts, seed)], None
    if deformation == "grow":     # the last object's mesh, 2.5 times as big about its centre and moved: well outside its old root box
        p = pts[lo:hi].copy()
        c = p[:, :3].mean(axis=0)
        p[:, :3] = ((p[:, :3] - c) * np.float32(2.5) + c + np.array((0.35, 0.1, -0.2), np.float32)).astype(np.float32)
        return [(p, lo)], last
    if deformation == "twice":
        first = _smooth(pts, seed, 0.04)
        return [(first, 0), sub(first, seed + 1)], None
    raise KeyError(deformation)


def _rays(scene, grown):
    o, d = seeded_rays(2048, seed=7)
    if grown is None:
        return o, d
    tri = _mesh_triangles(scene, grown)           # rays aimed at points of the grown mesh's triangles, through its object's matrix
    M = scene.numpy()["objects"].view(np.float32).reshape(-1, 20)[grown, :16].reshape(4, 4).T.astype(np.float64)
    rng = np.random.default_rng(8)
    corners = scene.points()[tri[rng.integers(0, len(tri), 512)], :3].astype(np.float64)
    t = np.einsum("ij,ijk->ik", rng.dirichlet((1.0, 1.0, 1.0), 512), corners) @ M[:3, :3].T + M[:3, 3]
    o2 = rng.uniform(-1.0, 1.0, (512, 3))
    o2[:, 1] -= 0.5
    d2 = t - o2
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    return np.concatenate([o, o2.astype(np.float32)]), np.concatenate([d, d2.astype(np.float32)])


def _pc():
    return engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=4)


CONFIGS = [dict(pipeline=p, hot_pairs=h) for p in (0, 1) for h in (0, 2)]
DEFAULTS = dict(pipeline=-1, hot_pairs=2, object_tree_min=48)


def _everything(r, o, d):
    """What the entry points give for the tables now on the device."""
    out = dict(hits=engine.hits_to_numpy(r.trace_rays(o, d)), frames=[], counters=[])
    for cfg in CONFIGS:
        for k, v in cfg.items():
            r.set_tuning(k, v)
        r.reset_counters()
        out["frames"].append(r.render(_pc(), W, H))
        out["counters"].append(r.counters())
    for k in ("pipeline", "hot_pairs"):
        r.set_tuning(k, DEFAULTS[k])
    out["aovs"] = r.render_aovs(_pc(), W, H)
    return out


@pytest.mark.parametrize("deformation", DEFORMATIONS)
@pytest.mark.parametrize("name", SCENES)
def test_refit_tables_equal_a_fresh_upload_and_the_oracle(renderer, name, deformation):
    scene, tuning = _scene(name)
    updates, grown = _updates(scene, deformation, seed=100 + SCENES.index(name))
    if name == "blob":
        assert _widest_level(scene, scene.counts()["objects"] - 1) > 256, "no level of the mesh is wider than the single-block launch takes"
    if name == "emissive":
        assert (scene.numpy()["bvhNodes"].view(np.uint32).reshape(-1, 8)[:, 7] > 7).any(), "the scene has no leaf of more than 7 triangles"
    try:
        for k, v in tuning.items():
            renderer.set_tuning(k, v)
        renderer.upload_scene(scene, dynamic=True)                  # context A: the old shape, then the refit
        for p, first in updates:
            renderer.update_points(p, first)
        for p, first in updates:
            scene.update_points(p, first)
        o, d = _rays(scene, grown)
        A = _everything(renderer, o, d)
        renderer.upload_scene(scene)                                # context B: a fresh upload of the refit host scene
        B = _everything(renderer, o, d)
    finally:
        for k, v in DEFAULTS.items():
            renderer.set_tuning(k, v)
    ref_hits = engine.hits_to_numpy(pyoracle.trace_rays(scene, o, d))
    if grown is not None:
        aimed = ref_hits["objectHitIndex"][2048:][ref_hits["didHit"][2048:].astype(bool) & (ref_hits["isSphere"][2048:] == 0)]
        assert (aimed == grown).sum() > 50, "the aimed rays do not reach the grown mesh"
    assert_hits_equal(A["hits"], B["hits"])
    assert_hits_equal(A["hits"], ref_hits)
    ref_img, ref_cnt = pyoracle.render(scene, _pc(), W, H)
    for cfg, fa, fb, ca, cb in zip(CONFIGS, A["frames"], B["frames"], A["counters"], B["counters"]):
        assert same_bits(fa, fb), f"{cfg}: the frame after update_points differs from a fresh upload's"
        assert same_bits(fa, ref_img), f"{cfg}: the frame after update_points differs from the oracle's"
        assert ca == cb, f"{cfg}: counters {ca} against a fresh upload's {cb}"
        for k in COUNTERS:
            assert ca[k] == ref_cnt[k], f"{cfg}: counter {k}: {ca[k]}, oracle {ref_cnt[k]}"
    for k in A["aovs"]:
        assert same_bits(A["aovs"][k], B["aovs"][k]), f"render_aovs plane {k}"


def _float64_case(scene):
    """The rays and the float64 answers for the deformed bunny (object 9), as test_closest_hit_float64._case makes them."""
    bs = bf.BruteScene.from_numpy(scene.numpy())
    o, d = _aimed_rays(bs, [9], 2600, np.random.default_rng(41))
    ref = bs.closest_hit(o, d)
    keep = ~(ref["didHit"] & (ref["dst"] * np.linalg.norm(d.astype(np.float64), axis=1) < ON_SURFACE))
    return o[keep], d[keep], {k: v[keep] for k, v in ref.items()}, int((~keep).sum())


def test_deformed_bunny_against_float64(renderer):
    """Context A against brute force in float64 over the deformed points: the margin, the 2 % cap on excluded rays and the floor of
    500 well-conditioned mesh hits of test_closest_hit_float64.py (its own _conditions and _compare)."""
    scene, p, first = _deformed_bunny()
    renderer.upload_scene(scene, dynamic=True)
    renderer.update_points(p, first)
    scene.update_points(p, first)
    o, d, ref, dropped = _float64_case(scene)
    good, _, _ = _conditions("deformed bunny", ref, [9], dropped)
    corners = _corners_of(scene)
    _compare("deformed bunny", "oracle", ref, engine.hits_to_numpy(pyoracle.trace_rays(scene, o, d)), corners, good)
    _compare("deformed bunny", "gpu after update_points", ref, engine.hits_to_numpy(renderer.trace_rays(o, d)), corners, good)


# ---------------------------------------------------------------------------------------------------------------- no-ops, refusals
def _frame(r):
    r.reset_counters()
    img = r.render(_pc(), W, H)
    c = r.counters()
    return img, (c["boxTests"], c["triTests"], c["raysTraced"])


def test_noop_updates_leave_frames_bit_equal(renderer):
    scene = model_scene("bunny.obj", spheres=True)
    renderer.upload_scene(scene, dynamic=True)
    img0, cnt0 = _frame(renderer)
    renderer.update_points(scene.points(), 0)                        # the original points again: every box refit to what it was
    img1, cnt1 = _frame(renderer)
    assert same_bits(img0, img1) and cnt0 == cnt1
    renderer.update_points(np.zeros((0, 8), np.float32), 5)          # count = 0
    renderer._check(renderer._l.rt_update_points(renderer._h, None, 0, 0), "rt_update_points")
    img2, cnt2 = _frame(renderer)
    assert same_bits(img0, img2) and cnt0 == cnt2


def test_refusals_through_the_abi(renderer):
    scene = model_scene("bunny.obj")
    n = scene.counts()["triPoints"]
    pts = scene.points()
    renderer.upload_scene(scene)
    with pytest.raises(engine.RtError, match="was not uploaded with rt_upload_scene_dynamic"):
        renderer.update_points(pts[:4], 0)
    renderer.upload_scene(scene, dynamic=True)
    img0, cnt0 = _frame(renderer)
    with pytest.raises(engine.RtError, match="run past the scene's"):
        renderer.update_points(pts[:4], n - 3)
    with pytest.raises(engine.RtError, match="points is null"):
        renderer._check(renderer._l.rt_update_points(renderer._h, None, 0, 4), "rt_update_points")
    bad = _smooth(pts, 3, 0.1)
    bad[n // 2, 1] = np.nan
    with pytest.raises(engine.RtError, match=f"the position of point {n // 2} is not finite"):
        renderer.update_points(bad, 0)
    img1, cnt1 = _frame(renderer)
    assert same_bits(img0, img1) and cnt0 == cnt1, "a refused update changed the next frame"
    with pytest.raises(engine.RtError, match="is not finite"):
        scene.update_points(bad, 0)
    renderer.upload_scene(scene)                                     # a plain upload drops what the dynamic one kept
    with pytest.raises(engine.RtError, match="was not uploaded with rt_upload_scene_dynamic"):
        renderer.update_points(pts[:4], 0)


class _WithSharedNodes:
    """A scene's arrays with one more object, whose mesh is the first child of the last object's root: two meshes that share nodes."""

    def __init__(self, scene):
        import ctypes as C
        from ray_tracer_amd import _capi
        self._scene, self._a = scene, scene.arrays()
        n = self._a.objectCount
        self._objects = (_capi.RenderObject * (n + 1))()
        C.memmove(self._objects, self._a.objects, C.sizeof(_capi.RenderObject) * n)
        C.memmove(C.byref(self._objects[n]), C.byref(self._objects[n - 1]), C.sizeof(_capi.RenderObject))
        root = self._a.bvhNodes[self._objects[n - 1].bvhIndex]
        assert root.triCount == 0
        self._objects[n].bvhIndex = root.index
        self._a.objects, self._a.objectCount = C.cast(self._objects, C.POINTER(_capi.RenderObject)), n + 1

    def arrays(self):
        return self._a

    def counts(self):
        return dict(self._scene.counts(), objects=self._a.objectCount)


def test_a_refused_dynamic_upload_leaves_the_context_as_it_was(renderer):
    scene = model_scene("bunny.obj")
    renderer.upload_scene(scene, dynamic=True)
    img0, cnt0 = _frame(renderer)
    shared = _WithSharedNodes(scene)
    with pytest.raises(engine.RtError, match="rt_upload_scene_dynamic: a mesh shares BVH nodes with another mesh"):
        renderer.upload_scene(shared, dynamic=True)
    renderer._counts = scene.counts()
    img1, cnt1 = _frame(renderer)
    assert same_bits(img0, img1) and cnt0 == cnt1
    renderer.update_points(scene.points(), 0)                        # and it is still the dynamic scene it was
    img2, cnt2 = _frame(renderer)
    assert same_bits(img0, img2) and cnt0 == cnt2


# ---------------------------------------------------------------------------------------------------------------- temporal
def test_temporal_pass_restarts_the_refit_objects_only(renderer):
    scene = model_scene("bunny.obj")
    bunny = scene.counts()["objects"] - 1
    lo, hi = _mesh_points(scene, bunny)
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=1, bounceLimit=2)

    def step():
        renderer.render(pc, W, H)
        aovs = renderer.render_aovs(pc, W, H)
        _, mom = renderer.temporal_accumulate(pc, moments=True)
        return aovs, mom[..., 3]

    try:
        renderer.temporal_track_motion(True)
        renderer.upload_scene(scene, dynamic=True)
        step()
        before, n2 = step()
        assert renderer.temporal_motion_state() == dict(movedObjects=0, replacedObjects=0, movedSpheres=0)
        renderer.update_points(_smooth(scene.points()[lo:hi], 5, 0.02), lo)
        after, n3 = step()
        assert renderer.temporal_motion_state() == dict(movedObjects=0, replacedObjects=1, movedSpheres=0)
        on_bunny = after["hit"] & ~after["sphere"] & (after["object"] == bunny) & (n3 > 0)
        assert on_bunny.sum() > 50 and np.all(n3[on_bunny] == 1), "the refit object's pixels kept a history"
        walls = after["hit"] & before["hit"] & (after["object"] != bunny) & (before["object"] == after["object"]) & (n2 == 2)
        assert walls.sum() > 500 and np.all(n3[walls] == 3), "pixels of objects that were not refit lost their history"
        _, n4 = step()                                               # the snapshot has the true meshes again
        assert renderer.temporal_motion_state() == dict(movedObjects=0, replacedObjects=0, movedSpheres=0)
        assert np.all(n4[on_bunny & (n4 > 0)] >= 1) and (n4[on_bunny] == 2).sum() > 50
    finally:
        renderer.temporal_track_motion(False)


# ---------------------------------------------------------------------------------------------------------------- session
def test_session_update_points_keeps_scene_and_device_in_step(renderer):
    from ray_tracer_amd.session import InteractiveSession
    scene = model_scene("bunny.obj")
    lo, hi = _mesh_points(scene, scene.counts()["objects"] - 1)
    o, d = seeded_rays(1024, seed=9)
    plain = InteractiveSession(renderer, scene, W, H)
    with pytest.raises(engine.RtError, match="dynamic=True"):
        plain.update_points(scene.points()[lo:hi], lo)
    s = InteractiveSession(renderer, scene, W, H, dynamic=True)
    before = engine.hits_to_numpy(renderer.trace_rays(o, d))
    s.update_points(_smooth(scene.points()[lo:hi], 17, 0.08), lo)
    after = engine.hits_to_numpy(renderer.trace_rays(o, d))
    assert not np.array_equal(before["dst"], after["dst"])
    assert_hits_equal(after, engine.hits_to_numpy(pyoracle.trace_rays(s.scene, o, d)))
    bad = scene.points()[lo:lo + 2]
    bad[1, 2] = np.inf
    with pytest.raises(engine.RtError, match="is not finite"):
        s.update_points(bad, lo)
    assert_hits_equal(after, engine.hits_to_numpy(renderer.trace_rays(o, d)))
    assert_hits_equal(after, engine.hits_to_numpy(pyoracle.trace_rays(s.scene, o, d)))
