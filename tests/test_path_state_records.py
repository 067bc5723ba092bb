"""The records a path leaves between k_shade and k_trace_pw, and the ones it no longer leaves: a main ray whose seed says nothing
has no seed record (its queue entry is RAY_MAIN_BLANK), a sample's first segment reads the kept camera hit where it is, the
unfinished MIS of a diffuse bounce waits in two records (pendAlbedo, pendMis) while the directions of its two light queries are
written only for the queries that are traced, and `total` is stored only when it changed. None of this may show: pixels and all
eight counters against the oracle, in the three pipeline modes, the multi-kernel one forced into three parts.

Every scene here holds both sides of a branch in one image, so that a condition the wrong way round reads a record nobody wrote
(a stale one from an earlier bounce or another kind of ray) and the pixels or the counters differ."""
import os

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine, scenes

from util import cornell_scene, model_scene, random_emitter_scene

pytestmark = pytest.mark.gpu
KEYS = ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests")


@pytest.fixture(params=[(0, 0), (1, 64), (1, 8)], ids=["multikernel-3-parts", "fused", "fused-refill"])
def r(request, renderer):
    """The three pipeline modes of tests/test_gpu_parity.py; the multi-kernel one in three parts as tests/test_lanes.py forces it."""
    renderer.set_tuning("pipeline", request.param[0])
    renderer.set_tuning("pixel_refill", request.param[1])
    renderer.set_tuning("lanes_min_kslots", 1)
    renderer.set_tuning("lanes", 3)
    renderer.multi = request.param[0] == 0
    yield renderer
    for k, v in (("pipeline", -1), ("pixel_refill", 0), ("lanes_min_kslots", 1024), ("lanes", 0)):
        renderer.set_tuning(k, v)


def _same(r, scene, pc, W, H, what):
    ref, rc = pyoracle.render(scene, pc, W, H)
    r.upload_scene(scene)
    r.reset_counters()
    img = r.render(pc, W, H)
    if r.multi:
        assert r.last_pipeline() == 0 and r.last_parts() == 3
    diff = img.view(np.uint32) != ref.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.any(axis=-1).sum())} pixels differ"
    c = r.counters()
    for k in KEYS:
        assert c[k] == rc[k], f"{what}: counter {k}: gpu {c[k]} oracle {rc[k]}"
    assert rc["lightQueryMismatch"] == 0
    return ref


def _materials(s):
    """The materials of scenes.cornell() on a scene without the box: 0 white, 1 red, 2 green, 3 light, 4 mirror, 5 glass."""
    for i in range(10):
        s.set_sphere(i, (0, 0, 0), 0.0, 0)
    for m in (engine.default_material(), engine.default_material(albedo=(1, 0, 0)), engine.default_material(albedo=(0, 1, 0)),
              engine.default_material(albedo=(0, 0, 0), emissionColor=(1, 1, 1), emissionStrength=2.4),
              engine.default_material(reflectance=1.0), engine.default_material(ior=2.0)):
        s.add_material(m)


def _placed_objects_scene():
    """Identity-transform blobs and placed (general-transform) ones over a floor: the rays' seeds carry an object mask that rules
    some of the placed objects out (a record that has to be stored) next to rays that can reach all of them (no record)."""
    s = engine.Scene()
    _materials(s)
    fpos, fnrm = scenes.grid_patch((-1.0, 1.0, -1.0), (2.0, 0, 0), (0, 0, 2.0), 6, 6)
    s.add_mesh("floor", fpos, fnrm, engine.placement(), 0)
    for k in range(3):
        pos, nrm = scenes.blob(60 + 8 * k, seed=170 + k, radius=0.12, center=(-0.6 + 0.6 * k, 0.7, -0.3 + 0.3 * k))
        s.add_mesh(f"i{k}", pos, nrm, engine.placement(), [0, 1, 4][k])
    for k in range(7):
        where = (-0.75 + 0.25 * k, -0.6 + 0.2 * (k % 4), -0.5 + 0.3 * (k % 3))
        pos, nrm = scenes.blob(80 + 6 * k, seed=190 + k, radius=1.0)
        s.add_mesh(f"g{k}", pos, nrm, engine.placement(position=where, scale=(0.1, 0.13, 0.09), rotation=(12 * k, 31 * k, 7 * k)), [0, 2, 5, 1][k % 4])
    s.set_sphere(0, (0.3, 0.1, 0.2), 0.2, 5)
    s.read_obj(os.path.join(engine.ASSET_DIR, "light2.obj"), engine.placement(position=(0, -1.5, 0), frontOnly=True), 3)
    return s


def test_main_rays_with_and_without_a_seed_record(r):
    """Cornell with its real spheres: a main ray with a sphere in front of it carries that hit in its seed, its neighbour that
    passes all of them carries nothing and has no record. Then placed objects: a seed with an object mask is stored even though
    it holds no sphere hit. (Inverted, the traversal starts a sphere-bound ray from "no hit" or reads another round's hit record as a seed.)"""
    ref = _same(r, cornell_scene(True), engine.push_constants(97, 61, singleRender=1, sampleLimit=3), 97, 61, "Cornell with spheres")
    assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 100
    _same(r, model_scene("bunny.obj", material=5, spheres=True), engine.push_constants(96, 72, singleRender=1, sampleLimit=2), 96, 72, "bunny + sphere")
    _same(r, _placed_objects_scene(), engine.push_constants(112, 84, singleRender=1, sampleLimit=3, bounceLimit=6, environmentOn=True), 112, 84, "placed objects")


@pytest.mark.parametrize("kw", [dict(singleRender=1, sampleLimit=1), dict(singleRender=1, sampleLimit=5),
                                dict(singleRender=1, sampleLimit=3, debug=2, boxCap=300, triangleCap=60),
                                dict(singleRender=1, sampleLimit=3, debug=0, boxCap=300, triangleCap=60)],
                         ids=["1spp", "5spp", "heatmap-both", "heatmap-boxes"])
def test_kept_camera_hit_on_and_off(r, kw):
    """Several samples per pixel: every sample after the first starts from the kept camera hit (camReuse), which k_shade reads from
    camHit; the heat-map modes switch camReuse off (the camera ray is traced, and counted, per sample), and with 1 spp there is
    no later sample at all. The scene has spheres, glass and a mirror, so the first hit differs from pixel to pixel and a sample
    that read hit(RAY_MAIN) — the last bounce's hit — instead of camHit, or the reverse, shades another surface."""
    s = model_scene("klein_bottle.obj", material=4, scale=0.5, position=(0.0, -0.2, 0.0), spheres=True)
    _same(r, s, engine.push_constants(100, 75, **kw), 100, 75, str(kw))


@pytest.mark.parametrize("spp", [1, 3])
def test_kept_camera_hit_with_several_frames_per_dispatch(r, spp):
    """render_frames: the frames of a dispatch are slots of their own, each with its own camHit and its own sample count."""
    s = model_scene("bunny.obj", material=0, spheres=True)
    W, H, frames = 100, 75, 4
    pc = engine.push_constants(W, H, raysPerPixel=spp, progressive=1)
    prev, tot = None, {k: 0 for k in KEYS}
    for f in range(frames):
        pc.frameCount = f
        prev, rc = pyoracle.render(s, pc, W, H, prev=prev)
        for k in KEYS:
            tot[k] += rc[k]
    r.upload_scene(s)
    r.clear_framebuffer(); r.reset_counters()
    pc.frameCount = 0
    img = r.render_frames(pc, W, H, frames)
    assert np.array_equal(img.view(np.uint32), prev.view(np.uint32))
    c = r.counters()
    for k in KEYS:
        assert c[k] == tot[k], k
    pc.frameCount = 0
    r.clear_framebuffer(); r.reset_counters()
    for f in range(frames):     # ... and one frame per dispatch
        pc.frameCount = f
        img = r.render(pc, W, H)
    assert np.array_equal(img.view(np.uint32), prev.view(np.uint32))
    assert r.counters()["segments"] == tot["segments"]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5])
def test_light_queries_traced_and_answered_in_all_combinations(r, seed):
    """The random emitter scenes of tests/test_gpu_parity.py: several emissive meshes and spheres in front of, behind and inside
    other things, so that of a diffuse bounce's two light queries each is traced (an emitter on the ray, nothing known nearer) or
    answered by its creator (none on it, or a sphere nearer) — all four combinations in one image — with mirrors, glass, an open
    side (missing rays, with and without the environment) and bounce limits from 2 to 8 (terminated paths) after them. A
    direction record is only written for a traced query and the pending records only for a bounce that stays pending: a
    condition the wrong way round traces an earlier bounce's direction, or finishes the MIS with an earlier bounce's records."""
    s, pc, W, H = random_emitter_scene(seed)
    pc.sampleLimit = 3
    _same(r, s, pc, W, H, f"emitter scene {seed}")


def test_light_queries_switched_off_trace_both(r):
    """light_queries 0: no emitter list, every diffuse bounce traces both queries and leaves every record."""
    s, pc, W, H = random_emitter_scene(4)
    r.set_tuning("light_queries", 0)
    try:
        ref, rc = pyoracle.render(s, pc, W, H)
        r.upload_scene(s)
        r.reset_counters()
        img = r.render(pc, W, H)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
        c = r.counters()
        for k in ("paths", "segments", "raysReference"):
            assert c[k] == rc[k], k
    finally:
        r.set_tuning("light_queries", 1)
        r.upload_scene(s)


def _light_cosine_scene():
    s = engine.Scene()
    _materials(s)
    glow = s.add_material(engine.default_material(albedo=(0.8, 0.8, 0.8), emissionColor=(1.0, 0.8, 0.5), emissionStrength=1.5))

    def quad(y, x0, x1, z0, z1, ny):
        q = np.array([[[x0, y, z0], [x1, y, z0], [x1, y, z1]], [[x0, y, z0], [x1, y, z1], [x0, y, z1]]], np.float32)
        n = np.zeros_like(q); n[..., 1] = ny
        return q, n
    s.add_mesh("floor", *quad(1.0, -1.5, 1.5, -1.5, 1.5, -1.0), engine.placement(), 0)
    s.add_mesh("glowing_floor", *quad(0.99, -1.2, 1.2, -1.2, 1.2, -1.0), engine.placement(), glow)
    s.add_mesh("canopy", *quad(-2.0, -1.5, -0.2, -1.0, 1.0, 1.0), engine.placement(), 1)
    s.add_mesh("at_light_height", *quad(-1.51, 0.4, 1.5, -1.0, 1.0, 1.0), engine.placement(), 2)
    q, n = quad(-1.2, -0.1, 0.3, 0.2, 0.9, 0.0)   # zero normals on a real quad
    s.add_mesh("nan_normals", q, n, engine.placement(), 0)
    s.read_obj(os.path.join(engine.ASSET_DIR, "light2.obj"), engine.placement(position=(0, -1.5, 0), frontOnly=True), 3)
    return s


def test_light_cosines_zero_negative_and_nan(r):
    """lightSamplePDF's cosine, dot((0,-1,0), dir), is computed by the segment that makes the direction and kept in pendMis
    instead of the direction. The cosine is a component of a normalised vector, so it is in [-1, 1] or NaN, never infinite;
    what divides by it gets: negative values (a canopy above the light's height, y < -1.5, looking down: its light samples
    point downwards), values at and on either side of zero (a sheet whose shading points lie at the light's height to within
    rounding: y = -1.51 plus 0.01 times the normal), NaN (zero-length normals: normalize(0) is NaN in the reference, and so are
    the origin and both directions of the bounce), and ordinary ones (the floor). All of them with the box's light switched on,
    and a second, emissive sheet that the downward samples reach, so that the pdf is used and not only computed."""
    s = _light_cosine_scene()   # looking up: canopy, sheet, light, the quad without normals; looking down: the two floors
    W, H = 96, 72
    for kw in (dict(pos=(0.0, -0.2, -2.5), cameraAngles=(-25.0, 0.0, 0.0)), dict(pos=(0.0, -0.2, -2.5), cameraAngles=(25.0, 0.0, 0.0))):
        for env in (False, True):
            pc = engine.push_constants(W, H, singleRender=1, sampleLimit=4, bounceLimit=6, environmentOn=env, **kw)
            _same(r, s, pc, W, H, f"{kw} env {env}")
