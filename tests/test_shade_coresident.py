"""k_shade at the 80 registers that let one of its waves sit beside six waves of k_trace_pw_wide on a SIMD
(tests/test_coresidency_budget.py), against the oracle, bit for bit: pixels and all eight counters.

What the squeeze moved in shade_path is the order of its stores, the spot where `total` is compared with what was loaded, and where
the pending MIS's scalars are made, so every scene holds the branches that reach those spots: Cornell with its spheres and the
ceiling light (diffuse bounces whose two light queries fly, are answered by their creator, or one of each), a mirror mesh next to
a glass one (the specular branches and the sign of the refracted ray's origin), a camera that sees the sky over an open floor
(misses, samples that end, the kept camera hit of the samples after the first) and a mesh under a rotation and an uneven scale
(the matrix path of reconstruct_hit). 64 x 48 pixels, 4 spp, eight bounces, one and three frames per dispatch, with the three
parts and the wide kernel, which only big dispatches take by default, switched on for every size ("lanes_min_kslots" 1,
"wide_min_kslots" 0), so k_shade runs beside the other parts' traversal.

The plan gives the wide kernel only to a scene whose kernel would be k_trace_pw<20, .., 144, 5> (launch_plan.cpp:
trace_kernel_key): a BVH in the 20-entry bucket and fewer than two general-transform objects. The four scenes above are not such
scenes — the Cornell box alone is five placed objects on an 8-entry stack — and run their own k_trace_pw instantiations in three
parts. The Sponza stand-in is, so it is the fifth scene: the pair of kernels the register arithmetic is about, k_shade beside
k_trace_pw_wide<20, 192, 768>."""
import os

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine, scenes

from instantiation_scenes import _same
from util import cornell_scene, model_scene

pytestmark = pytest.mark.gpu

WIDE = "k_trace_pw_wide<20, 192, 768>"
W, H, SPP, BOUNCES = 64, 48, 4, 8
FRAMES = (1, 3)
DEFAULTS = (("pipeline", -1), ("wide_min_kslots", 1024), ("lanes_min_kslots", 1024))
KEYS = ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests")


def _cornell():
    return cornell_scene(True), {}


def _mirror_and_glass():
    s = model_scene("klein_bottle.obj", material=4, scale=0.5, position=(-0.35, -0.2, 0.0))
    s.read_obj(os.path.join(engine.ASSET_DIR, "bunny.obj"), engine.placement(position=(0.45, 0.53, -0.3), scale=0.5, samplerIndex=1), 5)
    return s, {}


def _open_floor():
    """No box: a floor, a diffuse, a mirror and a glass blob over it and the sky behind them."""
    s = engine.Scene()
    for i in range(10):
        s.set_sphere(i, (0, 0, 0), 0.0, 0)
    for m in (engine.default_material(), engine.default_material(albedo=(1, 0, 0)), engine.default_material(albedo=(0, 1, 0)),
              engine.default_material(albedo=(0, 0, 0), emissionColor=(1, 1, 1), emissionStrength=2.4),
              engine.default_material(reflectance=1.0), engine.default_material(ior=2.0)):
        s.add_material(m)
    fpos, fnrm = scenes.grid_patch((-2.0, 1.0, -2.0), (4.0, 0, 0), (0, 0, 4.0), 8, 8)
    s.add_mesh("floor", fpos, fnrm, engine.placement(), 0)
    for k, mat in enumerate((1, 4, 5)):
        pos, nrm = scenes.blob(60 + 8 * k, seed=170 + k, radius=0.35, center=(-0.8 + 0.8 * k, 0.5, -0.2 + 0.2 * k))
        s.add_mesh(f"blob{k}", pos, nrm, engine.placement(), mat)
    return s, dict(environmentOn=True, cameraAngles=(25.0, 0.0, 0.0))


def _placed_mesh():
    s = cornell_scene(False)
    s.read_obj(os.path.join(engine.ASSET_DIR, "bunny.obj"),
               engine.placement(position=(0.1, 0.5, 0.0), rotation=(20.0, 35.0, 10.0), scale=(0.5, 0.7, 0.6), samplerIndex=1), 0)
    return s, {}


def _sponza():
    return scenes.CONFIGS["sponza"]()[0], None


SCENES = {"cornell": _cornell, "mirror-and-glass": _mirror_and_glass, "sky": _open_floor, "placed-mesh": _placed_mesh, "sponza": _sponza}
TAKES_WIDE = ("sponza",)


@pytest.fixture(scope="module", params=list(SCENES))
def case(request):
    """(name, scene, push constants, {frames: the oracle's (last frame, summed counters)}): made once per scene, left unchanged."""
    s, kw = SCENES[request.param]()
    if kw is None:
        pc = scenes.sponza_camera(W, H, raysPerPixel=SPP, progressive=1, bounceLimit=BOUNCES)
    else:
        pc = engine.push_constants(W, H, raysPerPixel=SPP, progressive=1, bounceLimit=BOUNCES, **kw)
    refs, prev, tot = {}, None, {k: 0 for k in KEYS}
    tot["lightQueryMismatch"] = 0
    for f in range(max(FRAMES)):
        pc.frameCount = f
        prev, rc = pyoracle.render(s, pc, W, H, prev=prev)
        for k in tot:
            tot[k] += rc[k]
        if f + 1 in FRAMES:
            refs[f + 1] = (prev.copy(), dict(tot))
    pc.frameCount = 0
    return request.param, s, pc, refs


def _bounces(rc):
    """From the counters of one frame (camReuse on): diffuse bounces (each adds three calculateIntersections to its segment's one),
    light queries that were traced, and light queries their creator answered. A segment consumes one main-ray hit, traced unless
    it is the first of a pixel's later samples (the kept camera hit); what raysTraced holds beyond those are light queries."""
    diffuse = (rc["raysReference"] - rc["segments"]) // 3
    main_traced = rc["segments"] - (rc["paths"] - W * H)
    flown = rc["raysTraced"] - main_traced
    return diffuse, flown, 2 * diffuse - flown


def test_the_scenes_reach_the_branches(case):
    """The oracle's own counters and hits say that each scene holds what it is there for."""
    name, s, pc, refs = case
    rc = refs[1][1]
    diffuse, flown, answered = _bounces(rc)
    assert (rc["raysReference"] - rc["segments"]) % 3 == 0 and diffuse > 0, f"{name}: no diffuse bounce"
    assert rc["paths"] == W * H * SPP
    if name == "cornell":
        # light queries that fly and light queries answered from the emitter list, thousands of each; the ceiling light is small,
        # so most bounces have one of each (the NEE ray aims at it, the cosine probe rarely does), and bounces next to the light
        # or behind a sphere have two of a kind: a count of the mixed ones alone is not in the counters
        assert rc["emitterTests"] > 0 and flown > 1000 and answered > 1000, f"{name}: {flown} light queries traced, {answered} answered"
        assert flown + answered == 2 * diffuse
    if name == "mirror-and-glass":
        # every segment but a sample's last goes on, after a diffuse or a specular bounce; diffuse bounces count even where the path
        # ends with them, so what goes on beyond their number bounced off the mirror or through the glass
        specular_at_least = (rc["segments"] - rc["paths"]) - diffuse
        assert specular_at_least > 1000, f"{name}: at least {specular_at_least} specular bounces"
        _meets(s, pc, "klein bottle (mirror)", s.counts()["objects"] - 2, (-0.35, -0.2, 0.0))
        _meets(s, pc, "bunny (glass)", s.counts()["objects"] - 1, (0.45, 0.3, -0.3))
    if name == "sky":
        assert rc["raysHit"] < rc["raysTraced"] and rc["segments"] > rc["paths"], f"{name}: {rc}"
    if name == "placed-mesh":
        _meets(s, pc, "placed bunny", s.counts()["objects"] - 1, (0.1, 0.3, 0.0))


def _meets(s, pc, what, obj, around):
    """Rays from the camera towards a 7 x 7 patch around a point: some of them have object `obj` as their closest hit."""
    o = np.array(list(pc.camInfo.pos)[:3], np.float32)
    g = np.linspace(-0.3, 0.3, 7, dtype=np.float32)
    targets = np.array([[around[0] + dx, around[1] + dy, around[2]] for dx in g for dy in g], np.float32)
    d = targets - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    hits = pyoracle.trace_rays(s, np.tile(o, (len(d), 1)), d)
    n = sum(1 for h in hits if h.didHit and not h.isSphere and h.objectHitIndex == obj)
    assert n > 0, f"no ray from the camera meets the {what}"


@pytest.mark.parametrize("frames", FRAMES)
def test_shading_beside_the_wide_traversal_matches_the_oracle(renderer, case, frames):
    name, s, pc, refs = case
    r = renderer
    try:
        r.set_tuning("pipeline", 0)
        r.set_tuning("wide_min_kslots", 0)
        r.set_tuning("lanes_min_kslots", 1)
        r.upload_scene(s)
        r.clear_framebuffer(); r.reset_counters()
        pc.frameCount = 0
        img = r.render_frames(pc, W, H, frames)
        assert r.last_pipeline() == 0 and r.last_parts() == 3, f"{name}: pipeline {r.last_pipeline()}, {r.last_parts()} parts"
        assert (r.last_kernel() == WIDE) == (name in TAKES_WIDE), f"{name}: {r.last_kernel()}"
        _same(img, r.counters(), *refs[frames], what=f"{name}, {frames} frame(s) per dispatch")
    finally:
        pc.frameCount = 0
        for k, v in DEFAULTS:
            r.set_tuning(k, v)
