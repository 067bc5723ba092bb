"""Temporal accumulation by reprojection (rt_temporal_accumulate, rt_temporal_accumulate_host, Renderer.temporal_accumulate,
InteractiveSession(temporal=True), render.py --temporal-frames).

The pass is the temporal half of SVGF (Schied et al. 2017) as include/rt_amd.h and DESIGN.md ("Temporal accumulation") specify
it. The reference has no such pass, so the kernel is pinned by `Restatement` (tests/temporal_float64.py), a numpy restatement of that specification which keeps
its own history from call to call: in float64 it is what the kernel is compared with, in float32 it measures how far fp32
rounding alone moves the result (T there). Kept pixels (misses, emitters) must come back bit for bit.
CPU: the ctypes layout, the defaults, the restatement's own properties, the CLI flags."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ray_tracer_amd import _capi, devmem, engine, render, session

from temporal_float64 import cam, camera_of, camera_path, distances, emission_of, EMISSION_TOY, filtered_set, FRAGILE_CAP, paths, pixel_yaw, planes_of, primary_dirs, rel, Restatement, synthetic, synthetic_frame, T, T_COLOUR
from util import cornell_scene, device_buffers, model_scene, progressive_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(max_history=32, normal_cos=0.9, depth_tolerance=0.02)


class Checker:
    """One sequence: every call's result against the float64 restatement, and the float32 restatement beside it."""

    def __init__(self, emission, what):
        self.emission, self.what = emission, what
        self.ref, self.f32 = Restatement(np.float64), Restatement(np.float32)
        self.worst_gpu, self.worst_f32, self.worst_fragile = [0.0, 0.0], [0.0, 0.0], 0.0

    def reset(self):
        self.ref.reset()
        self.f32.reset()

    def check(self, ci, planes, got, mom, **kw):
        """planes: (rgba, normalDepth, position, albedo, ids). Returns the restatement's (out, moments, F, fragile)."""
        rgba = planes[0]
        out, m, F, fragile = self.ref.step(ci, *planes, self.emission, **kw)
        o32, m32, _, _ = self.f32.step(ci, *planes, self.emission, **kw)
        cmp = F & ~fragile
        if F.any():
            self.worst_fragile = max(self.worst_fragile, float(fragile.sum()) / float(F.sum()))
        self.worst_f32 = [max(a, b) for a, b in zip(self.worst_f32, distances(o32, m32, out, m, cmp))]
        print(f"{self.what}: F {int(F.sum())}, fragile {int(fragile.sum())}, float32 restatement worst: colour {self.worst_f32[0]:.3g} "
              f"variance {self.worst_f32[1]:.3g}", end="")
        assert got.dtype == np.float32 and got.shape == rgba.shape and mom.shape == rgba.shape, self.what
        assert np.array_equal(got[~F].view(np.uint32), rgba[~F].view(np.uint32)), self.what      # kept pixels bit for bit
        assert not mom[~F].view(np.uint32).any(), self.what                                       # their moments are (0, 0, 0, 0)
        assert np.array_equal(got[F][:, 3].view(np.uint32), rgba[F][:, 3].view(np.uint32)), self.what   # alpha is copied
        assert np.isfinite(got[F]).all() and np.isfinite(mom[F]).all(), self.what
        now = distances(got, mom, out, m, cmp)
        self.worst_gpu = [max(a, b) for a, b in zip(self.worst_gpu, now)]
        print(f"; kernel worst: colour {self.worst_gpu[0]:.3g} variance {self.worst_gpu[1]:.3g}")
        assert now[0] <= T_COLOUR, (self.what, "rgb, m1, m2, N", now[0], T_COLOUR)
        assert max(now) <= T, (self.what, "variance", now[1], T)
        assert self.worst_fragile <= FRAGILE_CAP, (self.what, self.worst_fragile)
        return out, m, F, fragile


# ---------------------------------------------------------------- CPU
def test_params_layout_and_defaults(tmp_path):
    P = _capi.RtTemporalParams
    fields = [n for n, _ in P._fields_]
    src = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    body = re.search(r"typedef struct RtTemporalParams \{(.*?)\} RtTemporalParams;", src, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields
    checks = [f"static_assert(sizeof(RtTemporalParams) == {C.sizeof(P)}, \"size\");"]
    checks += [f"static_assert(offsetof(RtTemporalParams, {f}) == {getattr(P, f).offset}, \"{f}\");" for f in fields]
    cpp = tmp_path / "params.cpp"
    cpp.write_text("#include <cstddef>\n#include \"rt_amd.h\"\n" + "\n".join(checks) + "\nint main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(cpp)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    d = P()
    _capi.lib().rt_temporal_params_default(C.byref(d))
    assert (d.maxHistory, d.normalCos, d.depthTolerance) == (32, np.float32(0.9), np.float32(0.02))
    for name in ("rt_temporal_accumulate", "rt_temporal_reset", "rt_read_temporal_rgba_f32", "rt_read_temporal_moments",
                 "rt_temporal_accumulate_host", "rt_temporal_params_default"):
        assert name in _capi.SYMBOLS


def test_primary_dirs_invert():
    """The restatement's reprojection is the inverse of its primary_dir: a point along pixel (x, y)'s ray lands on (x, y), as far
    as the float32 rotation is orthonormal (its entries are rounded to 2^-24, which moves a pixel coordinate of up to 37 by
    less than 1e-5)."""
    W, H = 37, 23
    ci = cam(W, H, 20.0, (0.3, -0.2, 1.0), -7.0)
    c = camera_of(ci)
    P = c["pos"] + 4.2 * primary_dirs(ci, W, H)
    q = (P - c["pos"]) @ c["M"]
    s = c["bl"][2] / q[..., 2]
    gy, gx = np.mgrid[0:H, 0:W]
    np.testing.assert_allclose((q[..., 0] * s - c["bl"][0]) / c["pw"] * W, gx, atol=1e-5)
    np.testing.assert_allclose((q[..., 1] * s - c["bl"][1]) / c["ph"] * H, gy, atol=1e-5)


def test_restatement_running_mean_with_an_unchanged_camera():
    """k calls with one camera give the running mean of the k frames on F, to 1e-6. The planes are float64 and the camera
    unrotated, so a point lands on its own pixel to 1e-13 and no neighbour takes part (with float32 positions it lands up to
    1e-5 of a pixel off, and a neighbour of very different colour shows at that weight: that is part of T, not of this property)."""
    W, H = 37, 23
    ci = cam(W, H, 0.0, (0.1, 0.05, 0.0))
    nd, position, albedo, ids = synthetic(ci, W, H, EMISSION_TOY, 1, np.float64)
    r = Restatement()
    frames = [synthetic_frame(albedo, 10 + k) for k in range(5)]
    d = np.maximum(albedo[..., :3].astype(np.float64), 1e-3)
    for k, rgba in enumerate(frames):
        out, mom, F, fragile = r.step(ci, rgba, nd, position, albedo, ids, EMISSION_TOY)
        assert F.any() and (~F).any() and not fragile.any()
        mean = np.mean([x[..., :3].astype(np.float64) / d for x in frames[:k + 1]], axis=0) * d
        np.testing.assert_allclose(out[F][:, :3], mean[F], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(mom[F][:, 3], k + 1, rtol=1e-6)
        assert np.array_equal(out[~F], rgba[~F].astype(np.float64)) and not mom[~F].any()
    # maxHistory: the history length saturates and the blend becomes an exponential average
    r.reset()
    for k, rgba in enumerate(frames):
        out, mom, F, _ = r.step(ci, rgba, nd, position, albedo, ids, EMISSION_TOY, max_history=3)
        np.testing.assert_allclose(mom[F][:, 3], min(k + 1, 3), rtol=1e-6)
    r.reset()
    for rgba in frames[:3]:   # maxHistory 1 passes the frame through
        out, mom, F, _ = r.step(ci, rgba, nd, position, albedo, ids, EMISSION_TOY, max_history=1)
        np.testing.assert_allclose(out[F][:, :3], rgba[F][:, :3].astype(np.float64), rtol=1e-6, atol=1e-9)


def test_restatement_pan_by_three_pixels():
    """One patch (the plane z = 5) whose first frame holds its column number as the demodulated colour: after a yaw worth three
    pixels at the image's centre the history read back there is the column three over, and everywhere it is the column the
    rotation's homography x' = z0 tan(atan(x / z0) + yaw) gives (a bilinear read of a linear ramp is exact)."""
    W, H = 67, 9
    a, b = cam(W, H), cam(W, H, pixel_yaw(W, H, 3.0))
    em = np.array([0.0])

    def planes(ci):
        D = primary_dirs(ci, W, H)
        t = 5.0 / D[..., 2]
        nd, position = np.zeros((H, W, 4), np.float32), np.ones((H, W, 4), np.float32)
        nd[..., 2], nd[..., 3], position[..., :3] = -1.0, t, t[..., None] * D
        ids = np.zeros((H, W, 4), np.uint32)
        ids[..., 3] = 1
        return nd, position, np.ones((H, W, 4), np.float32), ids

    r = Restatement()
    ramp = np.zeros((H, W, 4), np.float32)
    ramp[..., :3] = np.arange(W, dtype=np.float32)[None, :, None]
    r.step(a, ramp, *planes(a), em)
    out, mom, F, fragile = r.step(b, np.zeros((H, W, 4), np.float32), *planes(b), em)
    assert F.all()
    two = mom[..., 3] == 2.0
    read = 2.0 * out[..., 0]          # N = 2: out = e_h + (0 - e_h) / 2
    c = camera_of(b)
    x = c["bl"][0] + c["pw"] * np.arange(W) / W
    yaw = np.radians(pixel_yaw(W, H, 3.0))
    want = (c["bl"][2] * np.tan(np.arctan(x / c["bl"][2]) - yaw) - c["bl"][0]) / c["pw"] * W
    inside = (want >= 0) & (want <= W - 1)
    assert inside.sum() >= W - 5 and two[:, inside].all() and (mom[:, want < -1, 3] == 1.0).all() and (want < -1).any()
    # float32 positions of magnitude 5 move a pixel coordinate of up to 67 by about 67 * 2^-24 * a few
    np.testing.assert_allclose(read[:, inside], np.broadcast_to(want[inside], (H, int(inside.sum()))), atol=1e-4)
    centre = int(np.argmin(np.abs(x)))   # the column nearest the optical axis: exactly three columns there, less towards the sides
    assert abs(want[centre] - (centre - 3)) < 0.02 and abs(read[H // 2, centre] - (centre - 3)) < 0.02


def test_restatement_half_turn_has_no_history():
    W, H = 37, 23
    a, b = cam(W, H), cam(W, H, 180.0)
    r = Restatement()
    pa, pb = synthetic(a, W, H, EMISSION_TOY, 3), synthetic(b, W, H, EMISSION_TOY, 4)
    r.step(a, synthetic_frame(pa[2], 5), *pa, EMISSION_TOY)
    rgba = synthetic_frame(pb[2], 6)
    out, mom, F, fragile = r.step(b, rgba, *pb, EMISSION_TOY)
    assert F.sum() > 200 and not fragile.any()
    assert (mom[F][:, 3] == 1.0).all()
    np.testing.assert_allclose(out[F][:, :3], rgba[F][:, :3].astype(np.float64), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("W,H", [(1, 1), (67, 1), (1, 67), (37, 23), (130, 70)])
def test_synthetic_sequences_are_rarely_fragile(W, H):
    """The synthetic inputs of the GPU test, on the restatement alone: fragile pixels within the cap, and the float32 run's
    distance from the float64 one (the part of T these inputs give)."""
    worst = [0.0, 0.0]
    for name, cams in paths(W, H).items():
        ref, f32 = Restatement(), Restatement(np.float32)
        for k, ci in enumerate(cams):
            planes = synthetic(ci, W, H, EMISSION_TOY, 100 * k + W)
            rgba = synthetic_frame(planes[2], 7 * k + H)
            out, mom, F, fragile = ref.step(ci, rgba, *planes, EMISSION_TOY)
            o32, m32, _, _ = f32.step(ci, rgba, *planes, EMISSION_TOY)
            assert (F.any() or (k > 0 and W * H == 1)) and fragile.sum() <= FRAGILE_CAP * F.sum(), (name, k, int(fragile.sum()), int(F.sum()))
            worst = [max(a, b) for a, b in zip(worst, distances(o32, m32, out, mom, F & ~fragile))]
    print(f"synthetic {W}x{H}: float32 restatement against float64, worst relative difference: colour {worst[0]:.3g} variance {worst[1]:.3g}")
    assert worst[0] <= T_COLOUR / 4 and max(worst) <= T / 4


def test_cli_flags():
    p = render.build_parser()
    assert p.parse_args([]).temporal_frames == 0
    assert p.parse_args(["--temporal-frames", "4"]).temporal_frames == 4


# ---------------------------------------------------------------- GPU helpers
def _params(max_history=32, normal_cos=0.9, depth_tolerance=0.02):
    return _capi.RtTemporalParams(max_history, normal_cos, depth_tolerance)


def _host(r, ci, rgba, nd, position, albedo, ids, **kw):
    H, W = rgba.shape[:2]
    b = _capi.RtAovBuffers(normalDepth=nd.ctypes.data, position=position.ctypes.data, albedo=albedo.ctypes.data, ids=ids.ctypes.data)
    out, mom = np.empty_like(rgba), np.empty_like(rgba)
    r._check(r._l.rt_temporal_accumulate_host(r._h, W, H, C.byref(ci), rgba.ctypes.data, C.byref(b), C.byref(_params(**kw)), out.ctypes.data,
                                              mom.ctypes.data), "rt_temporal_accumulate_host")
    return out, mom


# ---------------------------------------------------------------- 1. synthetic planes against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (67, 1), (1, 67), (37, 23), (130, 70)])
def test_synthetic_planes_against_the_restatement(renderer, W, H):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    emission = emission_of(s)
    assert (emission > 0).any() and (emission == 0).any()
    for name, cams in paths(W, H).items():
        for kw in ({}, dict(max_history=1), dict(max_history=4)) if name == "unchanged" else ({},):
            renderer.temporal_reset()
            chk = Checker(emission, (W, H, name, kw))
            for k, ci in enumerate(cams + cams[-1:] * 2 if kw else cams):
                planes = synthetic(ci, W, H, emission, 100 * k + W)
                rgba = synthetic_frame(planes[2], 7 * k + H)
                got, mom = _host(renderer, ci, rgba, *planes, **dict(DEFAULTS, **kw))
                out, m, F, fragile = chk.check(ci, (rgba,) + planes, got, mom, **dict(DEFAULTS, **kw))
                assert F.any() or (k > 0 and W * H == 1)   # the one pixel of 1 x 1 may turn away from the patches
                if name == "jump" and k == 2:    # all history off-screen: N = 1 and the frame passes
                    assert (mom[F][:, 3] == 1.0).all()
                    assert (rel(got[F][:, :3], rgba[F][:, :3].astype(np.float64)) <= T).all()
                if kw.get("max_history") == 1:
                    assert (mom[F][:, 3] == 1.0).all()
                    assert (rel(got[F][:, :3], rgba[F][:, :3].astype(np.float64)) <= T).all()
                if kw.get("max_history") == 4 and k >= 4:   # N_h + 1 is about 5 by now: the clamp gives exactly 4
                    ok = F & ~fragile
                    assert (rel(mom[ok][:, 3], m[ok][:, 3]) <= T).all() and mom[F][:, 3].max() == 4.0


# ---------------------------------------------------------------- 2. rendered frames against the restatement
def _rendered_sequence(renderer, s, W, H, frames, spp=1):
    """render -> render_aovs -> temporal_accumulate on the context's own planes along camera_path; yields per frame
    (pc, frame, aovs, accumulated, moments)."""
    renderer.upload_scene(s)
    for k in range(frames):
        pc = camera_path(W, H, k, raysPerPixel=spp)
        frame = renderer.render(pc, W, H)
        a = renderer.render_aovs(pc, W, H)
        got, mom = renderer.temporal_accumulate(pc, moments=True)
        yield pc, frame, a, got, mom


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_spheres", "bunny"])
def test_rendered_frames_against_the_restatement(renderer, name):
    s = cornell_scene(True) if name == "cornell_spheres" else model_scene("bunny.obj", spheres=True)
    W, H = 160, 120
    chk = Checker(emission_of(s), name)
    for k, (pc, frame, a, got, mom) in enumerate(_rendered_sequence(renderer, s, W, H, 8)):
        out, m, F, fragile = chk.check(pc.camInfo, (frame,) + planes_of(a), got, mom)
        assert F.mean() > 0.5 and (~F).any()
        ok = F & ~fragile
        assert (rel(mom[ok][:, 3], m[ok][:, 3]) <= T).all()       # history lengths
        if k == 7:
            assert np.median(mom[F][:, 3]) >= 6.0                 # most of the frame kept its history along the path


# ---------------------------------------------------------------- 3. kept pixels
@pytest.mark.gpu
def test_kept_pixels(renderer):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    emission = emission_of(s)
    dark, light = int(np.flatnonzero(emission == 0)[0]), int(np.argmax(emission))
    W, H = 40, 24
    ci = cam(W, H)
    D = primary_dirs(ci, W, H)
    t = 5.0 / D[..., 2]
    nd, position, albedo = np.zeros((H, W, 4), np.float32), np.ones((H, W, 4), np.float32), np.full((H, W, 4), 0.5, np.float32)
    nd[..., 2], nd[..., 3], position[..., :3] = -1.0, t, t[..., None] * D
    ids = np.zeros((H, W, 4), np.uint32)
    ids[..., 2], ids[..., 3] = dark, 1
    first = ids.copy()
    first[:, :10, 3] = 0                  # misses
    first[:12, 10:20, 2] = light          # an emitter
    first[12:, 10:20, 2] = len(emission)  # a material index past the table
    rng = np.random.default_rng(11)
    rgba = rng.random((H, W, 4)).astype(np.float32)
    rgba[:, :20, :3] = 1e6
    F1 = filtered_set(first, emission)
    got, mom = _host(renderer, ci, rgba, nd, position, albedo, first)
    assert np.array_equal(got[~F1].view(np.uint32), rgba[~F1].view(np.uint32)) and not mom[~F1].view(np.uint32).any()
    assert (mom[F1][:, 3] == 1.0).all()
    # the same camera, every pixel filtered now: those that were kept have no history, and none of the 1e6 leaks
    rgba2 = rng.random((H, W, 4)).astype(np.float32)
    got, mom = _host(renderer, ci, rgba2, nd, position, albedo, ids)
    N = mom[..., 3]
    assert (N[:, :19] == 1.0).all() and (N[:, 21:] == 2.0).all()
    assert got[..., :3].max() < 2.0
    assert (rel(got[:, :19, :3], rgba2[:, :19, :3].astype(np.float64)) <= T).all()
    # and kept again: bit for bit whatever the history holds
    got, mom = _host(renderer, ci, rgba, nd, position, albedo, first)
    assert np.array_equal(got[~F1].view(np.uint32), rgba[~F1].view(np.uint32)) and not mom[~F1].view(np.uint32).any()


# ---------------------------------------------------------------- 4. one result by every route
@pytest.mark.gpu
def test_every_route_gives_the_same_frames(renderer):
    import torch  # noqa: F401  (its wheel's copy of the HIP runtime now sits beside the library's: devmem.hip must not take it)
    s = model_scene("bunny.obj", spheres=True)
    W, H = 72, 40
    renderer.upload_scene(s)
    pcs = [camera_path(W, H, k) for k in range(3)]
    own, frames, aovs = [], [], []
    for pc in pcs:
        frames.append(renderer.render(pc, W, H))
        aovs.append(renderer.render_aovs(pc, W, H))
        own.append(renderer.temporal_accumulate(pc, moments=True))
    assert (own[2][1][..., 3] > 1.0).any()
    renderer.temporal_reset()
    for pc, frame, a, (o, m) in zip(pcs, frames, aovs, own):   # host arrays
        o2, m2 = renderer.temporal_accumulate(pc, frame, a, moments=True)
        assert np.array_equal(o2.view(np.uint32), o.view(np.uint32)) and np.array_equal(m2.view(np.uint32), m.view(np.uint32))
    renderer.temporal_reset()
    nbytes = H * W * 16
    with device_buffers(("frame", "out", "moments") + engine.AOV_PLANES, nbytes, fill=7) as bufs:
        d = _capi.RtAovBuffers(**{k: bufs[k].ptr for k in engine.AOV_PLANES})
        for pc, (o, m) in zip(pcs, own):                        # device pointers
            renderer.render(pc, W, H, out_ptr=bufs["frame"].ptr)
            renderer.render_aovs(pc, W, H, out_ptrs={k: bufs[k].ptr for k in engine.AOV_PLANES})
            renderer._check(renderer._l.rt_temporal_accumulate(renderer._h, W, H, C.byref(pc.camInfo), bufs["frame"].ptr, C.byref(d), None,
                                                               bufs["out"].ptr, bufs["moments"].ptr), "rt_temporal_accumulate")
            renderer.sync()
            o3, m3 = bufs["out"].download((H, W, 4), np.float32), bufs["moments"].download((H, W, 4), np.float32)
            assert np.array_equal(o3.view(np.uint32), o.view(np.uint32)) and np.array_equal(m3.view(np.uint32), m.view(np.uint32))
        # the accumulated device plane goes straight into rt_denoise
        renderer._check(renderer._l.rt_denoise(renderer._h, W, H, bufs["out"].ptr, C.byref(d), None, bufs["frame"].ptr), "rt_denoise")
        renderer.sync()
        den = bufs["frame"].download((H, W, 4), np.float32)
    assert np.array_equal(den.view(np.uint32), renderer.denoise(own[2][0], aovs[2]).view(np.uint32))


# ---------------------------------------------------------------- 5. no side effects
@pytest.mark.gpu
def test_temporal_leaves_the_context_untouched(renderer):
    s = cornell_scene(True)
    W, H = 64, 48
    renderer.upload_scene(s)
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2)
    frame = renderer.render(pc, W, H)
    a = renderer.render_aovs(pc, W, H)
    den = renderer.denoise()
    state = lambda: (renderer.counters(), renderer.ray_cost(), renderer.last_pipeline(), renderer.last_parts(), renderer.last_kernel())  # noqa: E731
    before = state()
    renderer.temporal_accumulate(pc)
    renderer.temporal_accumulate(pc, frame, a, max_history=3, normal_cos=0.5, depth_tolerance=0.1)
    renderer.temporal_accumulate(pc.camInfo, moments=True)
    renderer.temporal_reset()
    assert state() == before
    assert np.array_equal(renderer.read_rgba().view(np.uint32), frame.view(np.uint32))
    again = renderer.read_aovs()
    for k in a:
        assert np.array_equal(again[k].view(np.uint8), a[k].view(np.uint8)), k
    last = np.empty((H, W, 4), np.float32)
    renderer._check(renderer._l.rt_read_denoised_rgba_f32(renderer._h, last.ctypes.data_as(C.POINTER(C.c_float)), last.size), "rt_read_denoised_rgba_f32")
    assert np.array_equal(last.view(np.uint32), den.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1])
def test_progressive_history_is_untouched(renderer, pipeline):
    s = model_scene("bunny.obj", spheres=True)
    W, H = 64, 48
    renderer.set_tuning("pipeline", pipeline)

    def temporal(pc):
        renderer.temporal_accumulate(pc)
        renderer.temporal_accumulate(pc, max_history=2, normal_cos=0.0, depth_tolerance=0.5)

    try:
        a = progressive_frames(renderer, s, W, H)
        b = progressive_frames(renderer, s, W, H, temporal)
    finally:
        renderer.set_tuning("pipeline", -1)
    assert a[2][1] == pipeline
    for fa, fb in zip(a[0], b[0]):
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert a[1] == b[1]
    assert a[2] == b[2]


# ---------------------------------------------------------------- 6. reset
@pytest.mark.gpu
def test_reset_upload_and_resize_start_a_new_history(renderer):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    emission = emission_of(s)

    def call(W, H, seed):
        ci = cam(W, H)
        planes = synthetic(ci, W, H, emission, 5)
        got, mom = _host(renderer, ci, synthetic_frame(planes[2], seed), *planes)
        F = filtered_set(planes[3], emission)
        assert F.sum() > 100
        return mom[F][:, 3]

    assert (call(37, 23, 1) == 1.0).all()
    assert (call(37, 23, 2) == 2.0).all()
    renderer.temporal_reset()
    assert (call(37, 23, 3) == 1.0).all()
    assert (call(37, 23, 4) == 2.0).all()
    renderer.upload_scene(s)
    assert (call(37, 23, 5) == 1.0).all()
    assert (call(37, 23, 6) == 2.0).all()
    assert (call(23, 37, 7) == 1.0).all()     # the same pixel count, another shape
    assert (call(23, 37, 8) == 2.0).all()
    assert (call(40, 23, 9) == 1.0).all()
    assert (call(37, 23, 10) == 1.0).all()    # and back: the history of the first size is gone


# ---------------------------------------------------------------- 7. it does what it is for
def quality(r, s, W, H):
    """Eight 4-spp frames along camera_path, accumulated, against a 1024-spp render at the last camera, all clamped to [0, 1]:
    the MSE of the accumulated frame over that of the last raw frame on the pixels of F whose history is four frames or longer,
    and the MSE of accumulate-then-denoise over that of denoising the last raw frame alone, on the whole frame."""
    for pc, frame, a, got, mom in _rendered_sequence(r, s, W, H, 8, spp=4):
        pass
    clean = r.render(camera_path(W, H, 7, singleRender=1, sampleLimit=1024), W, H)
    F = filtered_set(planes_of(a)[3], emission_of(s))
    long = F & (mom[..., 3] >= 4.0)
    c = lambda x: np.clip(np.asarray(x, np.float64)[..., :3], 0.0, 1.0)  # noqa: E731
    mse = lambda x, m=Ellipsis: float(((c(x) - c(clean))[m] ** 2).mean())  # noqa: E731
    den_acc, den_raw = r.denoise(got, a), r.denoise(frame, a)
    return dict(filtered_pixels=int(F.sum()), long_history_pixels=int(long.sum()), raw_mse=mse(frame, long), accumulated_mse=mse(got, long),
                ratio=mse(got, long) / mse(frame, long), denoised_raw_mse=mse(den_raw), denoised_accumulated_mse=mse(den_acc),
                denoised_ratio=mse(den_acc) / mse(den_raw))


@pytest.mark.gpu
def test_accumulation_lowers_the_error(renderer):
    q = quality(renderer, cornell_scene(True), 160, 120)
    print(q)
    assert q["long_history_pixels"] >= 0.5 * q["filtered_pixels"], q
    assert q["ratio"] < 0.5, q
    assert q["denoised_accumulated_mse"] < q["denoised_raw_mse"], q


# ---------------------------------------------------------------- 8. session and CLI
@pytest.mark.gpu
def test_session_with_temporal(renderer):
    s = cornell_scene(True)
    W, H = 64, 48
    ses = session.InteractiveSession(renderer, s, W, H, temporal=True)
    longest = []
    for k in range(4):
        ses.frame(keys="W", frame_time_ms=2.0)
        assert ses.filtered.shape == (H, W, 4) and ses.image.shape == (H, W, 4)
        longest.append(float(ses.history_length.max()))
    assert longest == pytest.approx([1.0, 2.0, 3.0, 4.0], abs=1e-3)   # a weighted mean of equal lengths may round by an ulp
    assert not np.array_equal(ses.filtered, ses.image)
    for k in range(4):   # the camera rests: the reference's progressive accumulation takes over
        ses.frame()
        assert np.array_equal(ses.filtered.view(np.uint32), renderer.read_rgba().view(np.uint32))
        assert np.array_equal(ses.filtered.view(np.uint32), ses.image.view(np.uint32))
    ses.frame(keys="W", frame_time_ms=2.0)     # moving again: the history was re-seeded from the progressive image
    assert ses.history_length.max() == 2.0
    ses.frame(keys="W", frame_time_ms=2.0)
    assert ses.history_length.max() == pytest.approx(3.0, abs=1e-3)
    m = ses.material(0)
    m.albedo[0] = 0.25
    ses.set_material(0, m)                     # an edit resets
    ses.frame(keys="W", frame_time_ms=2.0)
    assert ses.history_length.max() == 1.0
    ses.frame(keys="W", frame_time_ms=2.0)
    ses.set_sphere(0, (0.0, 0.1, -0.3), 0.4, 5)
    ses.frame(keys="W", frame_time_ms=2.0)
    assert ses.history_length.max() == 1.0
    both = session.InteractiveSession(renderer, s, W, H, temporal=True, denoise=True)
    both.frame(keys="W", frame_time_ms=2.0)
    both.frame(keys="W", frame_time_ms=2.0)
    assert both.filtered.shape == (H, W, 4) and not np.array_equal(both.filtered, both.image)
    plain = session.InteractiveSession(renderer, s, W, H)
    plain.frame(keys="W", frame_time_ms=2.0)
    assert plain.filtered is None


@pytest.mark.gpu
def test_cli_temporal_frames_on_one_and_two_ranks(tmp_path):
    job = "--scene cornell --width 56 --height 37 --rays-per-pixel 1 --temporal-frames 4"
    one, den, plain = tmp_path / "one.npy", tmp_path / "den.npy", tmp_path / "plain.npy"
    assert render.main(f"{job} --out {one}".split()) == 0
    assert render.main(f"{job} --denoise --out {den}".split()) == 0
    a, b = np.load(one), np.load(den)
    assert a.shape == (37, 56, 4) and a.dtype == np.float32 and b.shape == a.shape
    assert np.isfinite(a).all() and not np.array_equal(a, b)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29554", "-m", "ray_tracer_amd.render", *job.split(), "--backend", "gloo", "--out", str(plain)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert "--temporal-frames needs the whole frame on one GPU" in p.stdout + p.stderr
    assert not plain.exists()


# ---------------------------------------------------------------- 9. errors
@pytest.mark.gpu
def test_errors(built):
    r = engine.Renderer(0)
    buf = devmem.DeviceBuffer(16 * 8 * 8 * 16)
    ci = cam(8, 8)
    try:
        def fails(match, W=8, H=8, camera=ci, rgba=None, aovs=None, params=None, out=None, moments=None):
            rc = r._l.rt_temporal_accumulate(r._h, W, H, C.byref(camera) if camera is not None else None, rgba,
                                             C.byref(aovs) if aovs is not None else None, C.byref(params) if params is not None else None, out, moments)
            assert rc < 0 and match in r._l.rt_last_error(r._h).decode(), (match, rc, r._l.rt_last_error(r._h).decode())

        fails("rt_temporal_accumulate before rt_upload_scene")
        host = np.zeros((8, 8, 4), np.float32)
        fp = C.POINTER(C.c_float)
        assert r._l.rt_read_temporal_rgba_f32(r._h, host.ctypes.data_as(fp), host.size) < 0
        assert "no ctx-owned accumulated frame" in r._l.rt_last_error(r._h).decode()
        assert r._l.rt_read_temporal_moments(r._h, host.ctypes.data_as(fp), host.size) < 0
        assert "no ctx-owned moments" in r._l.rt_last_error(r._h).decode()
        assert r._l.rt_temporal_reset(r._h) == 0
        r.upload_scene(cornell_scene(True))
        fails("bad image geometry", W=0)
        fails("bad image geometry", H=0)
        fails("image too large", W=1 << 15, H=1 << 15)
        fails("camera", camera=None)
        fails("no ctx-owned framebuffer")
        pc = engine.push_constants(8, 8, singleRender=1, sampleLimit=1)
        r.render(pc, 8, 8, row0=0, rowStride=2)   # a strip
        fails("the ctx framebuffer: rows 0 + k*2, k < 4 of a 8 x 8 image")
        r.render(pc, 8, 8)
        fails("no ctx-owned AOV planes")
        r.render_aovs(pc, 8, 8, row0=1, nRows=7)
        fails("the ctx AOV planes: rows 1 + k*1, k < 7")
        r.render_aovs(pc, 8, 8)
        fails("not the whole 16 x 8 frame", W=16)
        fails("d_aovs needs the normalDepth, position, albedo and ids planes",
              aovs=_capi.RtAovBuffers(normalDepth=host.ctypes.data, albedo=host.ctypes.data, ids=host.ctypes.data))
        for bad, what in ((dict(max_history=0), "maxHistory"), (dict(normal_cos=1.5), "normalCos"), (dict(normal_cos=-1.01), "normalCos"),
                          (dict(normal_cos=float("nan")), "normalCos"), (dict(depth_tolerance=0.0), "depthTolerance"),
                          (dict(depth_tolerance=-1.0), "depthTolerance"), (dict(depth_tolerance=float("nan")), "depthTolerance"),
                          (dict(depth_tolerance=float("inf")), "depthTolerance")):
            fails(what, params=_params(**bad))
            with pytest.raises(engine.RtError, match=what):
                r.temporal_accumulate(pc, **bad)
        plane = 8 * 8 * 16
        fails("an output overlaps an input", rgba=buf.ptr, out=buf.ptr)
        fails("an output overlaps an input", rgba=buf.ptr, moments=buf.ptr + 16)
        planes = _capi.RtAovBuffers(normalDepth=buf.ptr, position=buf.ptr + plane, albedo=buf.ptr + 2 * plane, ids=buf.ptr + 3 * plane)
        fails("an output overlaps an input", aovs=planes, out=buf.ptr + 3 * plane + 512)
        fails("d_out overlaps d_moments", aovs=planes, out=buf.ptr + 5 * plane, moments=buf.ptr + 5 * plane + 64)
        nd, albedo, ids = (np.zeros((8, 8, 4), t) for t in (np.float32, np.float32, np.uint32))
        b = _capi.RtAovBuffers(normalDepth=nd.ctypes.data, albedo=albedo.ctypes.data, ids=ids.ctypes.data)
        assert r._l.rt_temporal_accumulate_host(r._h, 8, 8, C.byref(ci), host.ctypes.data, C.byref(b), None, host.ctypes.data, None) < 0
        assert "aovs needs the normalDepth, position, albedo and ids planes" in r._l.rt_last_error(r._h).decode()
        b.position = nd.ctypes.data
        assert r._l.rt_temporal_accumulate_host(r._h, 8, 8, C.byref(ci), None, C.byref(b), None, host.ctypes.data, None) < 0
        assert "rgba and out are required" in r._l.rt_last_error(r._h).decode()
        with pytest.raises(ValueError):
            r.temporal_accumulate(pc, host[:4], r.read_aovs())
        with pytest.raises(ValueError):
            r.temporal_accumulate(pc, host)
        out, mom = r.temporal_accumulate(pc, moments=True)   # the context is still good, and no refused call left a history
        assert out.shape == (8, 8, 4) and np.isfinite(out).all() and mom[..., 3].max() == 1.0
        small = np.zeros((7, 4), np.float32)
        assert r._l.rt_read_temporal_rgba_f32(r._h, small.ctypes.data_as(fp), small.size) < 0
        assert "size mismatch" in r._l.rt_last_error(r._h).decode()
        assert r.temporal_accumulate(pc, moments=True)[1][..., 3].max() == 2.0
    finally:
        buf.free()
        r.close()
