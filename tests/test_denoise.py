"""Edge-aware a-trous denoiser (rt_denoise, rt_denoise_host, Renderer.denoise, render.py --denoise).

The filter is the spatial part of SVGF (Schied et al. 2017, after Dammertz et al. 2010) as include/rt_amd.h and DESIGN.md
("Denoising") specify it. The reference has no denoiser, so the kernels are pinned by `restate`, a float64 restatement of that
specification, as the GLSL built-ins are pinned by theirs. Kept pixels (misses, emitters) and K = 0 must come back bit for bit.
CPU: the ctypes layout, the defaults, the restatement's own properties and the CLI flag."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ray_tracer_amd import _capi, devmem, engine, render, scenes

from denoise_float64 import _checker_scene, _shift, planes_of, restate
from temporal_float64 import emission_of, filtered_set
from util import cornell_scene, device_buffers, model_scene, progressive_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0)
OTHER = dict(sigma_luminance=1.5, sigma_normal=0.0, sigma_depth=0.25)   # sigma_normal 0: normals do not stop the filter
REL = 1e-4   # |gpu - ref| <= REL * max(|ref|, 1e-3): an estimate from fp32 rounding (rt_exp2, rt_pow and the divisions against float64)


def assert_matches(got, rgba, ref, F, what):
    """Filtered pixels within REL of the restatement, kept pixels bit for bit; returns the largest relative difference."""
    assert got.dtype == np.float32 and got.shape == rgba.shape, what
    assert np.array_equal(got[~F].view(np.uint32), rgba[~F].view(np.uint32)), what
    assert np.array_equal(got[F][:, 3].view(np.uint32), rgba[F][:, 3].view(np.uint32)), what   # alpha is copied
    g, r = got[F][:, :3].astype(np.float64), ref[F][:, :3]
    rel = np.abs(g - r) / np.maximum(np.abs(r), 1e-3)
    worst = float(rel.max()) if rel.size else 0.0
    assert np.all(np.isfinite(g)), what
    assert worst <= REL, (what, worst, np.argwhere(rel > REL)[:5].tolist())
    return worst


# ---------------------------------------------------------------- CPU
def test_params_layout_and_defaults(tmp_path):
    P = _capi.RtDenoiseParams
    fields = [n for n, _ in P._fields_]
    src = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    body = re.search(r"typedef struct RtDenoiseParams \{(.*?)\} RtDenoiseParams;", src, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields
    checks = [f"static_assert(sizeof(RtDenoiseParams) == {C.sizeof(P)}, \"size\");"]
    checks += [f"static_assert(offsetof(RtDenoiseParams, {f}) == {getattr(P, f).offset}, \"{f}\");" for f in fields]
    cpp = tmp_path / "params.cpp"
    cpp.write_text("#include <cstddef>\n#include \"rt_amd.h\"\n" + "\n".join(checks) + "\nint main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(cpp)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    d = P()
    _capi.lib().rt_denoise_params_default(C.byref(d))
    assert (d.iterations, d.sigmaLuminance, d.sigmaNormal, d.sigmaDepth) == (5, 4.0, 128.0, 1.0)
    for name in ("rt_denoise", "rt_read_denoised_rgba_f32", "rt_denoise_host", "rt_denoise_params_default"):
        assert name in _capi.SYMBOLS


def _synthetic(H, W, nmat, seed):
    """Seeded planes: normals in four clusters, depth ramps with a step, albedo with zeros, colours in [0, 1], ids with misses,
    material indices past the table and every flag combination."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    k = (x // 9 + y // 7) % 4
    base = np.array([[0, 0, -1], [1, 0, 0], [0, 1, 0], [0.6, 0.8, 0]], np.float64)
    n = base[k] + 0.08 * rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nd = np.empty((H, W, 4), np.float32)
    nd[..., :3] = n
    nd[..., 3] = 2.0 + 0.01 * x + 0.02 * y + 0.5 * (k == 1) + 0.003 * rng.random((H, W))
    albedo = rng.random((H, W, 4)).astype(np.float32)
    albedo[rng.random((H, W)) < 0.1, :3] = 0.0
    rgba = rng.random((H, W, 4)).astype(np.float32)
    ids = np.zeros((H, W, 4), np.uint32)
    ids[..., 0] = rng.integers(0, 9, (H, W))
    ids[..., 2] = rng.integers(0, nmat + 2, (H, W))
    ids[..., 3] = (rng.random((H, W)) < 0.85) | (rng.integers(0, 4, (H, W)) << 1)
    return rgba, nd, albedo, ids


def test_restatement_properties():
    H, W = 24, 30
    emission = np.array([0.0, 0.0, 5.0])
    rgba, nd, albedo, ids = _synthetic(H, W, 3, 1)
    # K = 0 is the identity; kept pixels hold their input
    out, F = restate(rgba, nd, albedo, ids, emission, iterations=0)
    assert np.array_equal(out, rgba.astype(np.float64))
    out, F = restate(rgba, nd, albedo, ids, emission)
    assert (~F).any() and F.any()
    assert np.array_equal(out[~F], rgba[~F].astype(np.float64)) and np.array_equal(out[..., 3], rgba[..., 3].astype(np.float64))
    # a constant e stays constant
    flat = rgba.copy()
    flat[..., :3] = 0.25 * np.maximum(albedo[..., :3], np.float32(1e-3))
    out, F = restate(flat, nd, albedo, ids, emission)
    np.testing.assert_allclose(out[F][:, :3] / np.maximum(albedo[F][:, :3].astype(np.float64), 1e-3), 0.25, rtol=1e-6)
    # two half-planes with orthogonal normals: nothing crosses
    half = np.arange(W)[None, :].repeat(H, 0) < W // 2
    nd2 = nd.copy()
    nd2[..., :3] = np.where(half[..., None], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    ids2 = ids.copy()
    ids2[..., 2], ids2[..., 3] = 0, 1
    col = np.where(half[..., None], 1.0, 5.0) * np.maximum(albedo[..., :3], np.float32(1e-3))
    rgba2 = rgba.copy()
    rgba2[..., :3] = col
    out, F = restate(rgba2, nd2, albedo, ids2, emission)
    assert F.all()
    e = out[..., :3] / np.maximum(albedo[..., :3].astype(np.float64), 1e-3)
    np.testing.assert_allclose(e[half], 1.0, rtol=1e-6)   # the float32 rounding of the input
    np.testing.assert_allclose(e[~half], 5.0, rtol=1e-6)
    # the blind filter does mix them
    out, _ = restate(rgba2, nd2, albedo, ids2, emission, blind=True)
    e = out[..., :3] / np.maximum(albedo[..., :3].astype(np.float64), 1e-3)
    assert e[half].max() > 1.5


def test_denoise_flag():
    assert render.build_parser().parse_args([]).denoise is False
    assert render.build_parser().parse_args(["--denoise"]).denoise is True


# ---------------------------------------------------------------- GPU helpers
def _params(iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0):
    return _capi.RtDenoiseParams(iterations, sigma_luminance, sigma_normal, sigma_depth)


def _denoise_host(r, rgba, nd, albedo, ids, **kw):
    H, W = rgba.shape[:2]
    planes = _capi.RtAovBuffers(normalDepth=nd.ctypes.data, albedo=albedo.ctypes.data, ids=ids.ctypes.data)
    out = np.empty_like(rgba)
    r._check(r._l.rt_denoise_host(r._h, W, H, rgba.ctypes.data, C.byref(planes), C.byref(_params(**kw)), out.ctypes.data),
             "rt_denoise_host")
    return out


def _render_frame(r, scene, pc, W, H):
    """One frame and its planes into the context's own buffers; returns both as numpy."""
    r.upload_scene(scene)
    frame = r.render(pc, W, H)
    return frame, r.render_aovs(pc, W, H)


def _check_rendered(r, scene, frame, a, what, rows=None):
    nd, albedo, ids = planes_of(a)
    got = r.denoise()
    if rows is None:
        ref, F = restate(frame, nd, albedo, ids, emission_of(scene))
        return assert_matches(got, frame, ref, F, what)
    worst = 0.0
    for band, keep in rows:   # row bands wider than the filter's reach (2 + 2 * 31 + 1 rows at K = 5) by a margin each side
        ref, F = restate(frame[band], nd[band], albedo[band], ids[band], emission_of(scene))
        worst = max(worst, assert_matches(got[band][keep], frame[band][keep], ref[keep], F[keep], f"{what} rows {band}"))
    return worst


# ---------------------------------------------------------------- 3. synthetic planes against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (1, 67), (67, 1), (37, 23), (130, 70)])
def test_synthetic_planes_against_the_restatement(renderer, W, H):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    emission = emission_of(s)
    assert (emission > 0).any() and (emission == 0).any()
    worst = 0.0
    for seed, extra in ((W * 1000 + H, {}), (W * 1000 + H + 1, OTHER)):
        rgba, nd, albedo, ids = _synthetic(H, W, len(emission), seed)
        for K in (0, 1, 3, 5, 10):
            kw = dict(DEFAULTS, iterations=K, **extra)
            got = _denoise_host(renderer, rgba, nd, albedo, ids, **kw)
            if K == 0:
                assert np.array_equal(got.view(np.uint32), rgba.view(np.uint32))
                continue
            ref, F = restate(rgba, nd, albedo, ids, emission, **kw)
            worst = max(worst, assert_matches(got, rgba, ref, F, (W, H, K, extra)))
    print(f"synthetic {W}x{H}: largest relative difference {worst:.3g}")


# ---------------------------------------------------------------- 4. rendered frames against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_spheres", "bunny"])
def test_rendered_frames_against_the_restatement(renderer, name):
    s = cornell_scene(True) if name == "cornell_spheres" else model_scene("bunny.obj", spheres=True)
    W, H = 96, 72
    frame, a = _render_frame(renderer, s, engine.push_constants(W, H, singleRender=1, sampleLimit=4), W, H)
    F = filtered_set(planes_of(a)[2], emission_of(s))
    assert F.mean() > 0.5 and (~F).any()   # the light (and any miss) is kept
    worst = _check_rendered(renderer, s, frame, a, name)
    print(f"{name} {W}x{H} 4 spp: largest relative difference {worst:.3g}")


@pytest.mark.gpu
def test_sponza_1080p_against_the_restatement(renderer):
    s = scenes.sponza(0)[0]
    W, H = 1920, 1080
    frame, a = _render_frame(renderer, s, scenes.sponza_camera(W, H, singleRender=1, sampleLimit=1), W, H)
    assert (~a["hit"]).any() and a["hit"].mean() > 0.5
    worst = _check_rendered(renderer, s, frame, a, "sponza",
                            rows=[(slice(0, 200), slice(0, 130)), (slice(H - 200, H), slice(70, 200))])
    print(f"sponza {W}x{H} 1 spp: largest relative difference {worst:.3g}")


# ---------------------------------------------------------------- 5. no leakage
@pytest.mark.gpu
def test_misses_and_emitters_do_not_leak(renderer):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    emission = emission_of(s)
    light = int(np.argmax(emission))
    H, W = 48, 64
    rgba, nd, albedo, ids = _synthetic(H, W, len(emission), 7)
    ids[..., 2] = 0
    ids[..., 3] = 1
    ids[:, : W // 3, 3] = 0                 # misses
    ids[H // 2:, W // 3: W // 2, 2] = light   # an emitter
    F = filtered_set(ids, emission)
    rgba[..., :3] = np.where(F[..., None], 0.0, 1e6)
    for kw in (DEFAULTS, dict(DEFAULTS, iterations=10, **OTHER)):
        got = _denoise_host(renderer, rgba, nd, albedo, ids, **kw)
        assert np.array_equal(got[~F].view(np.uint32), rgba[~F].view(np.uint32))
        assert not got[F][:, :3].any()


# ---------------------------------------------------------------- 6. one result by every route
@pytest.mark.gpu
def test_every_route_gives_the_same_frame(renderer):
    import torch  # noqa: F401  (its wheel's copy of the HIP runtime now sits beside the library's: devmem.hip must not take it)
    s = model_scene("bunny.obj", spheres=True)
    W, H = 72, 40
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=4)
    frame, a = _render_frame(renderer, s, pc, W, H)
    first = renderer.denoise()
    assert np.array_equal(renderer.denoise().view(np.uint32), first.view(np.uint32))   # two calls in a row
    assert np.array_equal(renderer.denoise(frame, a).view(np.uint32), first.view(np.uint32))   # host path
    nbytes = H * W * 16
    with device_buffers(("frame", "out") + engine.AOV_PLANES, nbytes, fill=7) as bufs:
        renderer.render(pc, W, H, out_ptr=bufs["frame"].ptr)
        renderer.render_aovs(pc, W, H, out_ptrs={k: bufs[k].ptr for k in engine.AOV_PLANES})
        d = _capi.RtAovBuffers(**{k: bufs[k].ptr for k in engine.AOV_PLANES})
        renderer._check(renderer._l.rt_denoise(renderer._h, W, H, bufs["frame"].ptr, C.byref(d), None, bufs["out"].ptr), "rt_denoise")
        renderer.sync()
        out, dev_frame = bufs["out"].download((H, W, 4), np.float32), bufs["frame"].download((H, W, 4), np.float32)
    assert np.array_equal(dev_frame.view(np.uint32), frame.view(np.uint32))
    assert np.array_equal(out.view(np.uint32), first.view(np.uint32))
    assert np.array_equal(renderer.denoise().view(np.uint32), first.view(np.uint32))   # the context's planes are still its own


# ---------------------------------------------------------------- 7. no side effects
@pytest.mark.gpu
def test_denoise_leaves_the_context_untouched(renderer):
    s = cornell_scene(True)
    W, H = 64, 48
    frame, a = _render_frame(renderer, s, engine.push_constants(W, H, singleRender=1, sampleLimit=2), W, H)
    state = lambda: (renderer.counters(), renderer.ray_cost(), renderer.last_pipeline(), renderer.last_parts(), renderer.last_kernel())  # noqa: E731
    before = state()
    renderer.denoise()
    renderer.denoise(frame, a, iterations=3, **OTHER)
    renderer.denoise(iterations=0)
    assert state() == before
    assert np.array_equal(renderer.read_rgba().view(np.uint32), frame.view(np.uint32))
    again = renderer.read_aovs()
    for k in a:
        assert np.array_equal(again[k].view(np.uint8), a[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1])
def test_progressive_history_is_untouched(renderer, pipeline):
    s = model_scene("bunny.obj", spheres=True)
    W, H = 64, 48
    renderer.set_tuning("pipeline", pipeline)

    def denoise(pc):
        renderer.denoise()
        renderer.denoise(iterations=2, **OTHER)

    try:
        a = progressive_frames(renderer, s, W, H)
        b = progressive_frames(renderer, s, W, H, denoise)
    finally:
        renderer.set_tuning("pipeline", -1)
    assert a[2][1] == pipeline
    for fa, fb in zip(a[0], b[0]):
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert a[1] == b[1]
    assert a[2] == b[2]


def _edges(a):
    """Pixels with a 4-neighbour of a different object, material or hit flag."""
    key = np.stack([a["object"].astype(np.int64), a["material"].astype(np.int64), a["hit"].astype(np.int64), a["sphere"].astype(np.int64)], -1)
    e = np.zeros(a["hit"].shape, bool)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        inside = _shift(np.ones(e.shape, bool), dy, dx, False)
        e |= inside & (_shift(key, dy, dx, -1) != key).any(-1)
    return e


def quality(r, scene, W, H, textures=None):
    """Noisy 4-spp, denoised and blind-B3 frames against a 1024-spp render, all clamped to [0, 1]: the MSE ratios."""
    r.upload_scene(scene)
    if textures is not None:
        r.upload_textures(textures)
    try:
        clean = r.render(engine.push_constants(W, H, singleRender=1, sampleLimit=1024), W, H)
        noisy = r.render(engine.push_constants(W, H, singleRender=1, sampleLimit=4), W, H)
        a = r.render_aovs(engine.push_constants(W, H), W, H)
        den = r.denoise()
    finally:
        if textures is not None:
            r.upload_textures([])
    nd, albedo, ids = planes_of(a)
    blind, _ = restate(noisy, nd, albedo, ids, emission_of(scene), blind=True)
    c = lambda x: np.clip(np.asarray(x, np.float64)[..., :3], 0.0, 1.0)  # noqa: E731
    edge = _edges(a)
    mse = lambda x, m=Ellipsis: float(((c(x) - c(clean))[m] ** 2).mean())  # noqa: E731
    return dict(noisy_mse=mse(noisy), denoised_mse=mse(den), ratio=mse(den) / mse(noisy), edge_pixels=int(edge.sum()),
                edge_denoised_mse=mse(den, edge), edge_blind_mse=mse(blind, edge), edge_ratio_to_blind=mse(den, edge) / mse(blind, edge)), a


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["cornell_spheres", "checkerboard"])
def test_quality_against_1024_spp(renderer, variant):
    W, H = 160, 120
    if variant == "checkerboard":
        s, m, tex = _checker_scene()
        q, a = quality(renderer, s, W, H, [tex])
        quad = a["material"] == m
        assert quad.sum() > 1000 and len(np.unique(a["albedo"][quad], axis=0)) >= 2   # the map is in the albedo plane
    else:
        q, a = quality(renderer, cornell_scene(True), W, H)
    print(variant, q)
    assert q["edge_pixels"] > 200
    assert q["ratio"] <= 0.5, q
    assert q["edge_denoised_mse"] < q["edge_blind_mse"], q


# ---------------------------------------------------------------- 9. CLI
@pytest.mark.gpu
def test_cli_denoise_on_one_and_two_ranks(tmp_path):
    job = "--scene cornell --width 56 --height 37 --single-render --sample-limit 2 --denoise"
    one, two, png = tmp_path / "one.npy", tmp_path / "two.npy", tmp_path / "one.png"
    assert render.main(f"{job} --out {one}".split()) == 0
    assert render.main(f"{job} --out {png}".split()) == 0
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29553", "-m", "ray_tracer_amd.render", *job.split(), "--backend", "gloo", "--out", str(two)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    a, b = np.load(one), np.load(two)
    assert a.shape == (37, 56, 4) and a.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    from PIL import Image
    assert Image.open(png).size == (56, 37)
    plain = tmp_path / "plain.npy"
    assert render.main(f"{job.replace(' --denoise', '')} --out {plain}".split()) == 0
    assert not np.array_equal(np.load(plain), a)   # the file is the denoised frame


# ---------------------------------------------------------------- 10. errors
@pytest.mark.gpu
def test_errors(built):
    r = engine.Renderer(0)
    buf = devmem.DeviceBuffer(8 * 8 * 16)
    try:
        def fails(match, W=8, H=8, rgba=None, aovs=None, params=None, out=None):
            rc = r._l.rt_denoise(r._h, W, H, rgba, C.byref(aovs) if aovs is not None else None,
                                 C.byref(params) if params is not None else None, out)
            assert rc != 0 and match in r._l.rt_last_error(r._h).decode(), (match, r._l.rt_last_error(r._h).decode())

        fails("rt_denoise before rt_upload_scene")
        host = np.zeros((8, 8, 4), np.float32)
        assert r._l.rt_read_denoised_rgba_f32(r._h, host.ctypes.data_as(C.POINTER(C.c_float)), host.size) != 0
        assert "no ctx-owned denoised frame" in r._l.rt_last_error(r._h).decode()
        r.upload_scene(cornell_scene(True))
        fails("bad image geometry", W=0)
        fails("bad image geometry", H=0)
        fails("image too large", W=1 << 15, H=1 << 15)
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
        fails("d_aovs needs the normalDepth, albedo and ids planes", aovs=_capi.RtAovBuffers(normalDepth=host.ctypes.data))
        for bad, what in ((dict(iterations=11), "iterations must be 0..10"), (dict(sigma_luminance=0.0), "sigmaLuminance"),
                          (dict(sigma_luminance=float("nan")), "sigmaLuminance"), (dict(sigma_luminance=float("inf")), "sigmaLuminance"),
                          (dict(sigma_normal=-1.0), "sigmaNormal"), (dict(sigma_normal=float("nan")), "sigmaNormal"),
                          (dict(sigma_depth=0.0), "sigmaDepth"), (dict(sigma_depth=float("-inf")), "sigmaDepth")):
            fails(what, params=_params(**bad))
            with pytest.raises(engine.RtError, match=what):
                r.denoise(**bad)
        fails("d_out overlaps an input", rgba=buf.ptr, out=buf.ptr)
        planes = _capi.RtAovBuffers(normalDepth=buf.ptr, albedo=buf.ptr + 64, ids=buf.ptr + 128)
        fails("d_out overlaps an input", aovs=planes, out=buf.ptr + 512)
        nd, albedo, ids = (np.zeros((8, 8, 4), t) for t in (np.float32, np.float32, np.uint32))
        b = _capi.RtAovBuffers(normalDepth=nd.ctypes.data, albedo=albedo.ctypes.data)
        assert r._l.rt_denoise_host(r._h, 8, 8, host.ctypes.data, C.byref(b), None, host.ctypes.data) != 0
        assert "aovs needs the normalDepth, albedo and ids planes" in r._l.rt_last_error(r._h).decode()
        assert r._l.rt_denoise_host(r._h, 8, 8, None, C.byref(b), None, host.ctypes.data) != 0
        with pytest.raises(ValueError):
            r.denoise(host[:4], r.read_aovs())
        with pytest.raises(ValueError):
            r.denoise(host)
        out = r.denoise()   # the context is still good
        assert out.shape == (8, 8, 4) and np.isfinite(out).all()
        small = np.zeros((7, 4), np.float32)
        assert r._l.rt_read_denoised_rgba_f32(r._h, small.ctypes.data_as(C.POINTER(C.c_float)), small.size) != 0
        assert "size mismatch" in r._l.rt_last_error(r._h).decode()
        assert np.array_equal(r.denoise().view(np.uint32), out.view(np.uint32))
    finally:
        buf.free()
        r.close()
