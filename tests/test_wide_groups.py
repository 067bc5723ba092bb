"""The persistent-wave traversal in wide work-groups (k_trace_pw_wide<20, 192, 768>: two groups of 768 threads per CU, six waves
per SIMD, the whole top-level table in LDS) against the oracle, bit for bit.

By default only dispatches of a million paths or more take the wide kernel, so it is forced here ("wide_min_kslots" 0, and
"pipeline" 0 for the multi-kernel pipeline). The sizes are the ones at which a 768-thread group can go wrong and a 256-thread group
cannot: 64 paths in one group (eleven of its twelve waves find the queue empty, and still have to pass the barrier behind the
table fill before they leave), 800 paths (two groups, a multiple neither of 768 nor of 64) and the 64x48 tile of
tests/test_instantiations.py. Two scenes: a balanced soup whose BVH depth lands in the 20-entry bucket, and the Sponza stand-in,
whose 26 objects fill the LDS object table and share the pair table among many roots."""
import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine, scenes

from instantiation_scenes import _same, build_scene, soup

pytestmark = pytest.mark.gpu

WIDE = "k_trace_pw_wide<20, 192, 768>"
NARROW = "k_trace_pw<20, false, false, false, false, 144, 5>"
SIZES = [(8, 8), (40, 20), (64, 48)]
NEVER = 2 ** 31 - 1   # wide_min_kslots no dispatch reaches
DEFAULTS = (("pipeline", -1), ("wide_min_kslots", 1024), ("lanes_min_kslots", 1024), ("lanes", 0))
KEYS = ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests")


def _soup_scene():
    s, depth = build_scene(lambda: soup(40000, 3), False)
    assert 17 <= depth <= 20, f"the soup's BVH depth {depth} left the 20-entry bucket"
    return s, lambda W, H, **kw: engine.push_constants(W, H, bounceLimit=4, environmentOn=True, **kw)


def _sponza_scene():
    s, _ = scenes.CONFIGS["sponza"]()
    return s, lambda W, H, **kw: scenes.sponza_camera(W, H, bounceLimit=4, **kw)


@pytest.fixture(scope="module", params=["soup", "sponza"])
def case(request):
    """(name, scene, camera, {size: the oracle's (image, counters)}): made once per scene and left unchanged."""
    s, camera = {"soup": _soup_scene, "sponza": _sponza_scene}[request.param]()
    refs = {(W, H): pyoracle.render(s, camera(W, H, singleRender=1, sampleLimit=2), W, H) for W, H in SIZES}
    return request.param, s, camera, refs


def _reset(r):
    for k, v in DEFAULTS:
        r.set_tuning(k, v)


def test_wide_groups_against_the_oracle(renderer, case):
    name, s, camera, refs = case
    r = renderer
    try:
        r.set_tuning("pipeline", 0)
        r.set_tuning("wide_min_kslots", 0)
        r.upload_scene(s)
        for (W, H) in SIZES:
            r.reset_counters()
            img = r.render(camera(W, H, singleRender=1, sampleLimit=2), W, H)
            assert r.last_pipeline() == 0 and r.last_kernel() == WIDE, f"{name} {W}x{H}: {r.last_kernel()}"
            _same(img, r.counters(), *refs[(W, H)], what=f"{name} {W}x{H} wide")
        # the knob at its default: the 256-thread kernel, and the same bits
        W, H = SIZES[-1]
        r.set_tuning("wide_min_kslots", 1024)
        r.reset_counters()
        img = r.render(camera(W, H, singleRender=1, sampleLimit=2), W, H)
        assert r.last_kernel() == NARROW, f"{name} {W}x{H}, default knob: {r.last_kernel()}"
        _same(img, r.counters(), *refs[(W, H)], what=f"{name} {W}x{H} default")
    finally:
        _reset(r)


def test_wide_groups_in_parts_side_by_side(renderer, case):
    """Three frames in one dispatch, in three parts on three streams: wide launches run side by side, each on its share of the
    resident groups. The same call with the wide kernel switched off gives the same bits and counters."""
    name, s, camera, _ = case
    r = renderer
    W, H, frames = 64, 48, 3
    pc = camera(W, H, raysPerPixel=2, progressive=1)
    got = {}
    try:
        r.set_tuning("pipeline", 0)
        r.set_tuning("lanes_min_kslots", 1)
        r.upload_scene(s)
        for kernel, knob in ((WIDE, 0), (NARROW, NEVER)):
            r.set_tuning("wide_min_kslots", knob)
            r.clear_framebuffer(); r.reset_counters()
            pc.frameCount = 0
            img = r.render_frames(pc, W, H, frames)
            assert r.last_pipeline() == 0 and r.last_parts() == 3 and r.last_kernel() == kernel, f"{name}: {r.last_parts()} parts, {r.last_kernel()}"
            got[kernel] = (img.copy(), r.counters())
    finally:
        _reset(r)
    assert np.array_equal(got[WIDE][0].view(np.uint32), got[NARROW][0].view(np.uint32)), f"{name}: pixels differ between the wide and the 256-thread groups"
    for k in KEYS:
        assert got[WIDE][1][k] == got[NARROW][1][k], f"{name}: counter {k}: wide {got[WIDE][1][k]}, 256-thread {got[NARROW][1][k]}"
