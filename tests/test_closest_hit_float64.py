"""The closest-hit query against tests/brute_force.py: every triangle and sphere tested in float64, no BVH, nothing shared with
the oracle or the kernels. The CPU half holds oracle/raytrace_oracle.cpp to it, the GPU half rt_trace_rays (both traversal
kernels, LDS stack 8 and 24, hot pairs 0 and 2), rt_render_aovs and pick().

On the well-conditioned rays (brute_force's verdict, margin 1e-4; at most 2 % of a scene's rays may be excluded and at least 500
well-conditioned rays must end on a mesh triangle, both asserted) didHit, isSphere, objectHitIndex, frontFace, materialIndex and
the triangle (by its three corner positions) are equal and dst, hitPoint, normal are within the bounds brute_force derives from the
rounding count (c = 11 for dst). On all rays, where both hit, |dt| / t < 1e-3: an ill-conditioned ray may take the neighbouring
triangle, not another surface.

Every case prints its figures (rays, well-conditioned mesh hits, excluded share, largest |dt| / bound(c = 1)); c = 11 is asserted to
be at least twice each ratio of the oracle. The figures as measured are in brute_force's docstring, next to the rounding count.
"""
import numpy as np
import pytest

from ray_tracer_amd import engine
from oracle import pyoracle
import brute_force as bf
from closest_hit_cases import _case, _compare, _conditions, _corners_of, _meshes_scene, DEFAULTS, KNOBS, SCENES


# ---------------------------------------------------------------------------------------------------------------- CPU half
def test_reference_pieces():
    """The helper against closed forms: a sphere from outside and inside, one triangle's barycentric pairing and forward-matrix
    normal, a frontOnly back face, the tie going to the first object, the inverse's error estimate on a diagonal matrix."""
    b = bf.BruteScene()
    b.set_spheres([(0, 0, 5)], [1.0], [3])
    P = np.array([[(0, 0, 2), (1, 0, 2), (0, 1, 2)]], np.float64)
    N = np.array([[(1, 0, 0), (0, 1, 0), (0, 0, 1)]], np.float64)      # n0, n1, n2 tell the corners apart
    M = np.diag([2.0, 1.0, 1.0, 1.0])
    b.add_object(P, N, M, front_only=True, material=7)
    b.add_object(P, N, M, front_only=False, material=8)
    o = np.array([(0.5, 0.25, 0), (0.5, 0.25, 4), (0, 0, 5), (5, 5, 0)], np.float32)
    d = np.array([(0, 0, 2), (0, 0, -1), (0, 0, 1), (0, 0, 1)], np.float32)
    r = b.closest_hit(o, d)
    # ray 0: object-space x = 0.25, y = 0.25: u = 0.25 (towards v1), v = 0.25, w = 0.5; e1 x e2 = +z, -d.n < 0: a back face: the
    # frontOnly copy rejects it, the second copy takes it with the normal flipped; t = 2 / 2 (the direction has length 2)
    assert r["didHit"][0] and r["objectHitIndex"][0] == 1 and r["materialIndex"][0] == 8 and not r["frontFace"][0]
    assert abs(r["dst"][0] - 1.0) < 1e-15
    n = -(M[:3, :3] @ (0.5 * N[0, 0] + 0.25 * N[0, 1] + 0.25 * N[0, 2]))
    assert np.allclose(r["normal"][0], n / np.linalg.norm(n), atol=1e-15)
    # ray 1: from behind: a front face, both copies accept at the same t: the first wins, and the tie makes the ray ill-conditioned
    assert r["objectHitIndex"][1] == 0 and r["frontFace"][1] and abs(r["dst"][1] - 2.0) < 1e-15 and r["ill"][1]
    # ray 2: from the sphere's centre: the far root, the inside, the normal towards the origin
    assert r["isSphere"][2] and not r["frontFace"][2] and abs(r["dst"][2] - 1.0) < 1e-15 and np.allclose(r["normal"][2], (0, 0, -1))
    assert not r["didHit"][3]
    r = b.closest_hit(np.array([(0, 0, 2.5)], np.float32), np.array([(0, 0, 1)], np.float32))
    assert r["isSphere"][0] and r["frontFace"][0] and abs(r["dst"][0] - 1.5) < 1e-15 and np.allclose(r["normal"][0], (0, 0, -1))
    E = bf.inverse_error_unit(np.diag([2.0, 4.0, 8.0, 1.0]))
    assert np.allclose(np.diag(E), 3 * np.array([0.5, 0.25, 0.125, 1.0])) and E[0, 1] == 0


@pytest.mark.parametrize("name", SCENES)
def test_oracle_against_float64(name):
    s, bs, o, d, mesh_objects, ref, dropped = _case(name)
    good, mesh_hits, excluded = _conditions(name, ref, mesh_objects, dropped)
    got = engine.hits_to_numpy(pyoracle.trace_rays(s, o, d))
    ratio = _compare(name, "oracle", ref, got, _corners_of(s), good)
    assert bf.DST_C >= 2 * ratio, f"{name}: c = {bf.DST_C} is less than twice the worst ratio {ratio:.2f}: the count has lost a term"


def _camera_case(dirs32, pos):
    """The meshes scene seen by camera rays: the reference's answer for them."""
    s, bs = _meshes_scene()
    d = np.asarray(dirs32, np.float32).reshape(-1, 3)
    o = np.repeat(np.asarray(pos, np.float32)[None], len(d), 0)
    return s, bs, o, d, bs.closest_hit(o, d)


CAMERA = dict(W=80, H=60, kw=dict(pos=(0.15, -0.45, -2.6), cameraAngles=(3.0, -4.0, 0.0), fov=50.0))


def test_oracle_camera_rays_against_float64():
    """The rays render_aovs() shoots (here from the float64 camera, rounded), through the oracle."""
    W, H = CAMERA["W"], CAMERA["H"]
    pc = engine.push_constants(W, H, **CAMERA["kw"])
    s, bs, o, d, ref = _camera_case(bf.camera_dirs(pc, W, H).astype(np.float32), list(pc.camInfo.pos))
    good, _, _ = _conditions("camera", ref, [9, 10])
    _compare("camera", "oracle", ref, engine.hits_to_numpy(pyoracle.trace_rays(s, o, d)), _corners_of(s), good)


def _gpu_trace(renderer, name, tree_mins=(48,)):
    s, bs, o, d, mesh_objects, ref, dropped = _case(name, renderer)
    good, _, _ = _conditions(name, ref, mesh_objects, dropped)
    corners = _corners_of(s)
    worst = 0.0
    try:
        renderer.upload_scene(s)
        for tree_min in tree_mins:
            renderer.set_tuning("object_tree_min", tree_min)
            for knobs in KNOBS:
                for k, v in knobs.items():
                    renderer.set_tuning(k, v)
                got = engine.hits_to_numpy(renderer.trace_rays(o, d))
                worst = max(worst, _compare(name, f"gpu tree_min={tree_min} {knobs}", ref, got, corners, good))
    finally:
        for k, v in DEFAULTS.items():
            renderer.set_tuning(k, v)
    print(f"[{name}] gpu worst |dt|/bound(c=1) {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SCENES if n != "instances"])
def test_trace_rays_against_float64(renderer, name):
    _gpu_trace(renderer, name)


@pytest.mark.gpu
def test_trace_rays_against_float64_over_many_placed_objects(renderer):
    """The object hierarchy (off, from 2 objects on, default) and the object-mask window, which exist only on the GPU."""
    _gpu_trace(renderer, "instances", tree_mins=(0, 2, 48))


@pytest.mark.gpu
def test_aovs_and_pick_against_float64(renderer):
    """render_aovs(): its own ray_dir plane and the camera position are the reference's rays; depth, normal, position and the id
    planes against the answer. pick() on a handful of those pixels."""
    W, H = CAMERA["W"], CAMERA["H"]
    pc = engine.push_constants(W, H, **CAMERA["kw"])
    s, _ = _meshes_scene()
    renderer.upload_scene(s)
    a = renderer.render_aovs(pc, W, H)
    s, bs, o, d, ref = _camera_case(a["ray_dir"], list(pc.camInfo.pos))
    good, _, _ = _conditions("aovs", ref, [9, 10])
    h = a["hit"].reshape(-1)
    z = lambda x: np.where(h, x.reshape(-1), 0).astype(np.uint32)   # noqa: E731
    got = dict(dst=a["depth"].reshape(-1), didHit=h.astype(np.uint32), isSphere=a["sphere"].reshape(-1).astype(np.uint32),
               objectHitIndex=z(a["object"]), triHitIndex=z(a["triangle"]), materialIndex=z(a["material"]),
               frontFace=a["front_face"].reshape(-1).astype(np.uint32), hitPoint=a["position"].reshape(-1, 3),
               normal=a["normal"].reshape(-1, 3))
    corners = _corners_of(s)
    _compare("aovs", "render_aovs", ref, got, corners, good)
    rng = np.random.default_rng(77)
    mesh = np.flatnonzero(good & ref["didHit"] & ~ref["isSphere"] & np.isin(ref["objectHitIndex"], [9, 10]))
    other = np.flatnonzero(good & ~np.isin(np.arange(W * H), mesh))
    for i in list(rng.choice(mesh, 4, replace=False)) + list(rng.choice(other, 3, replace=False)):
        y, x = divmod(int(i), W)
        p = renderer.pick(pc, W, H, x, y)
        one = {k: v[i:i + 1] for k, v in ref.items()}
        hit = bool(p["hit"])
        rec = dict(dst=np.array([p["depth"]], np.float32), didHit=np.array([hit], np.uint32), isSphere=np.array([p["sphere"]], np.uint32),
                   objectHitIndex=np.array([p["object"] if hit else 0], np.uint32), triHitIndex=np.array([p["triangle"] if hit else 0], np.uint32),
                   materialIndex=np.array([p["material"] if hit else 0], np.uint32), frontFace=np.array([p["front_face"]], np.uint32),
                   hitPoint=np.asarray(p["position"], np.float32)[None], normal=np.asarray(p["normal"], np.float32)[None])
        assert np.array_equal(np.asarray(p["ray_dir"], np.float32), a["ray_dir"][y, x])
        _compare("aovs", f"pick({x}, {y})", one, rec, corners, np.array([True]))
