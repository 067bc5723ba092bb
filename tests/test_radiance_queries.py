"""Radiance queries: the path-traced radiance along the caller's own rays (rt_query_radiance and its _host form;
Renderer.query_radiance; include/rt_amd.h, DESIGN.md "Radiance queries").

The contract makes the pass a pixel-exact relative of rt_render: ray i, seeded from its id and the frame, runs the estimator
`samples` times from its own origin and direction, and a batch holding a frame's camera rays (origin camInfo.pos, directions the
rayDir plane of rt_render_aovs, ids the pixel indices) equals rt_render's image bit for bit. So every case here is held to
rt_render with the pipeline forced to 0 (k_trace_pw + k_shade), which tests/test_gpu_parity.py and tests/test_paths_float64.py
hold to the oracle and to the float64 restatement; tests/test_radiance_float64.py holds the queries to the restatement directly,
on seeds no rt_render uses."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_amd import _capi, devmem, engine

import radiance_fans as fans
from paths_float64 import _maps_scene, _sky_scene
from util import bits, cornell_scene

W, H = 64, 48
DEFAULTS = dict(pipeline=-1, camera_reuse=1, light_queries=1, lanes=0, lanes_min_kslots=1024, radiance_max_kslots=0, fused_maps=0)


@pytest.fixture
def gpu(renderer):
    """The session's renderer; afterwards no textures, a cleared progressive history and the knobs these tests turn at their defaults."""
    try:
        yield renderer
    finally:
        renderer.upload_textures([])
        renderer.clear_framebuffer()
        for k, v in DEFAULTS.items():
            renderer.set_tuning(k, v)


def _same(got, want, what):
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} rays differ from rt_render, first at {bad[:5].tolist()}: {got[bad[:2]].tolist()} against {want[bad[:2]].tolist()}"


def _camera_rays(gpu, pc, w, h):
    """A frame's camera rays in row-major order: camInfo.pos repeated, the rayDir plane of rt_render_aovs."""
    d = np.ascontiguousarray(gpu.render_aovs(pc, w, h)["ray_dir"].reshape(w * h, 3), np.float32)
    o = np.ascontiguousarray(np.repeat(np.array(list(pc.camInfo.pos), np.float32)[None], w * h, 0))
    return o, d


def _render0(gpu, pc, w, h):
    """rt_render through the multi-kernel pipeline, from a cleared history."""
    gpu.set_tuning("pipeline", 0)
    gpu.clear_framebuffer()
    img = gpu.render(pc, w, h)
    assert gpu.last_pipeline() == 0
    return img


# ---------------------------------------------------------------------------------------------------------------- camera parity
@pytest.mark.gpu
@pytest.mark.parametrize("camera_reuse", [0, 1])
@pytest.mark.parametrize("light_queries", [0, 1])
def test_cornell_frame_equals_rt_render(gpu, camera_reuse, light_queries):
    """Cornell 64 x 48, 4 samples, bounce limit 4, ids NULL for the whole frame in row-major order; camera_reuse 0 and 1,
    light_queries 0 and 1, and under each one part and three ("lanes_min_kslots" 0)."""
    gpu.upload_scene(cornell_scene(True))
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=4, bounceLimit=4)
    o, d = _camera_rays(gpu, pc, W, H)
    want = _render0(gpu, pc, W, H)          # (at the default knobs: they change no pixel)
    gpu.set_tuning("lanes_min_kslots", 0)
    gpu.set_tuning("camera_reuse", camera_reuse)
    gpu.set_tuning("light_queries", light_queries)
    for lanes in (1, 3):
        gpu.set_tuning("lanes", lanes)
        knobs = f"camera_reuse {camera_reuse} light_queries {light_queries} lanes {lanes}"
        got = gpu.query_radiance(o, d, samples=4, bounces=4)
        assert got.shape == (W * H, 4) and got.dtype == np.float32 and np.all(got[:, 3] == 1.0)
        assert "k_trace_pw" in gpu.last_kernel(), gpu.last_kernel()
        _same(got, want, f"cornell, {knobs}")
        _same(_render0(gpu, pc, W, H), want, f"rt_render, {knobs}")


def _fan_batch(gpu, samples=3, bounces=4):
    """The three-fan batch with the device's own camera directions, and each fan's rt_render (multi-kernel pipeline)."""
    gpu.upload_scene(fans.scene())
    pcs = [fans.fan_constants(k, samples, bounces) for k in range(3)]
    dirs = [_camera_rays(gpu, pc, fans.FW, fans.FH)[1] for pc in pcs]
    o, d, ids = fans.batch(lambda k: dirs[k])
    want = np.concatenate([_render0(gpu, pc, fans.FW, fans.FH).reshape(-1, 4) for pc in pcs])[:fans.N]
    return o, d, ids, want


@pytest.mark.gpu
def test_three_fans_equal_their_cameras_and_rays_are_independent(gpu):
    """Three cameras in the Cornell box + bunny scene, 32 x 24 each, concatenated with ids set to each fan's own pixel indices, the
    last 5 rays dropped (n = 2299), 3 samples: each fan equals its camera's rt_render. The origins differ per ray and samples
    restart, so a restart that reads one origin for all fails here. Then: the first 1, 63 and 257 rays submitted alone, and the
    whole batch in three pieces ("radiance_max_kslots" 1), give the same bits."""
    o, d, ids, want = _fan_batch(gpu)
    assert len(o) == fans.N == 2299
    full = gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids)
    for k in range(3):
        first, count = fans.fan_rows(k)
        _same(full[first:first + count], want[first:first + count], f"fan {k}")
    # the fans do differ: the check above is not three times the same image
    assert not np.array_equal(want[:700], want[768:1468]) and not np.array_equal(want[768:1468], want[1536:2236])
    for m in (1, 63, 257):
        _same(gpu.query_radiance(o[:m], d[:m], samples=3, bounces=4, ids=ids[:m]), full[:m], f"the first {m} rays alone")
    gpu.set_tuning("radiance_max_kslots", 1)
    _same(gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids), full, "three pieces")
    # ... and in parts, each piece
    gpu.set_tuning("lanes_min_kslots", 0)
    gpu.set_tuning("lanes", 3)
    _same(gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids), full, "three pieces in three parts")


@pytest.mark.gpu
def test_progressive_chain_equals_rt_render(gpu):
    """Frames 0, 1, 2 with progressive = 1, feeding `out` back, against rt_render's chain in the ctx framebuffer."""
    gpu.upload_scene(cornell_scene(True))
    pcs = [engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=3, progressive=1, frameCount=f) for f in (0, 1, 2)]
    o, d = _camera_rays(gpu, pcs[0], W, H)
    gpu.set_tuning("pipeline", 0)
    gpu.clear_framebuffer()
    want = [gpu.render(pc, W, H).copy() for pc in pcs]
    prev = np.zeros((W * H, 4), np.float32)
    for f in (0, 1, 2):
        got = gpu.query_radiance(o, d, samples=2, bounces=3, progressive=True, frame=f, out=prev)
        assert got is not prev
        _same(got, want[f], f"progressive frame {f}")
        prev = got
    assert not np.array_equal(want[0], want[2])


@pytest.mark.gpu
def test_map_scene_equals_rt_render(gpu):
    """The metalness + albedo map scene of tests/test_paths_float64.py: k_shade_rays_maps against k_shade_maps."""
    s, tex = _maps_scene()
    gpu.upload_scene(s)
    gpu.upload_textures(tex)
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=3, bounceLimit=3)
    o, d = _camera_rays(gpu, pc, W, H)
    want = _render0(gpu, pc, W, H)
    _same(gpu.query_radiance(o, d, samples=3, bounces=3), want, "maps")
    assert len(np.unique(bits(want).reshape(-1, 4)[:, :3])) > 100, "the frame is not flat"


@pytest.mark.gpu
def test_sky_scene_equals_rt_render(gpu):
    """Spheres under the environment: a wrong or missing env shows here."""
    gpu.upload_scene(_sky_scene())
    sun = dict(lightDir=(0.3, 0.8, -0.5, 1.0), horizonColor=(0.9, 0.8, 0.7, 40.0), zenithColor=(0.2, 0.4, 0.9, 5.0), groundColor=(0.3, 0.25, 0.2))
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=3, pos=(0.0, -0.6, -3.5), **sun)
    o, d = _camera_rays(gpu, pc, W, H)
    want = _render0(gpu, pc, W, H)
    got = gpu.query_radiance(o, d, samples=2, bounces=3, environment=pc.environment)
    _same(got, want, "open sky")
    dark = gpu.query_radiance(o, d, samples=2, bounces=3)      # environment off: not the same picture
    assert not np.array_equal(dark, got)


@pytest.mark.gpu
def test_no_bounce_one_sample_equals_rt_render(gpu):
    gpu.upload_scene(cornell_scene(True))
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=1, bounceLimit=0)
    o, d = _camera_rays(gpu, pc, W, H)
    want = _render0(gpu, pc, W, H)
    _same(gpu.query_radiance(o, d, samples=1, bounces=0), want, "bounce limit 0, one sample")


# ---------------------------------------------------------------------------------------------------------------- the device form
@pytest.mark.gpu
def test_device_form_equals_host_form(gpu):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    o, d, ids, _ = _fan_batch(gpu)
    host = gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids)
    dev = torch.device("cuda:0")
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    ti = torch.from_numpy(ids.astype(np.int32)).to(dev)
    out = torch.zeros((fans.N, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert gpu.query_radiance(to, td, samples=3, bounces=4, ids=ti, out=out, sync=False) is None
    gpu.sync()
    _same(out.cpu().numpy(), host, "torch tensors, sync=False")
    # progressive on the device: `out` holds the previous result
    gpu.query_radiance(to, td, samples=3, bounces=4, ids=ti, progressive=True, frame=1, out=out)
    _same(out.cpu().numpy(), gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids, progressive=True, frame=1, out=host), "progressive on the device")
    with pytest.raises(ValueError):
        gpu.query_radiance(to, td, out=torch.zeros((fans.N, 3), dtype=torch.float32, device=dev))       # too small
    with pytest.raises(ValueError):
        gpu.query_radiance(to, td.double(), out=out)


@pytest.mark.gpu
def test_device_pointers_equal_host_form(gpu):
    """The asynchronous form on device memory the test owns (integer pointers with n=), where no framework is needed: sync=False,
    then rt_sync, equals the host form; then a progressive frame on top of the result in `out`."""
    o, d, ids, _ = _fan_batch(gpu)
    host = gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids)
    bufs = []

    def device(a):
        bufs.append(devmem.DeviceBuffer(a.nbytes).upload(a))
        return bufs[-1].ptr

    try:
        d_o, d_d, d_i, d_out = device(o), device(d), device(ids), device(np.full((fans.N, 4), 7.0, np.float32))
        assert gpu.query_radiance(d_o, d_d, samples=3, bounces=4, ids=d_i, n=fans.N, out=d_out, sync=False) is None
        gpu.sync()
        got = bufs[-1].download((fans.N, 4), np.float32)
        _same(got, host, "device pointers, sync=False")
        gpu.query_radiance(d_o, d_d, samples=3, bounces=4, ids=d_i, n=fans.N, progressive=True, frame=1, out=d_out)
        got = bufs[-1].download((fans.N, 4), np.float32)
        _same(got, gpu.query_radiance(o, d, samples=3, bounces=4, ids=ids, progressive=True, frame=1, out=host), "progressive on the device")
        with pytest.raises(ValueError):
            gpu.query_radiance(d_o, d_d, out=d_out)             # integer pointers need n=
        with pytest.raises(ValueError):
            gpu.query_radiance(d_o, d_d, n=fans.N)              # ... and out=
    finally:
        gpu.sync()
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- what it leaves alone
@pytest.mark.gpu
def test_query_leaves_rendering_alone(gpu):
    """Two progressive frames into the ctx framebuffer with a query between them equal the two frames without it; rt_last_pipeline,
    rt_last_parts and rt_ray_cost are what they were; rt_get_counters().paths grows by n x samples."""
    s = fans.scene()
    gpu.upload_scene(s)
    pcs = [fans.fan_constants(0, 2, 3, frame=f, progressive=1) for f in (0, 1)]
    o, d = _camera_rays(gpu, pcs[0], fans.FW, fans.FH)
    gpu.set_tuning("pipeline", 0)
    gpu.set_tuning("lanes", 1)
    gpu.clear_framebuffer()
    gpu.render(pcs[0], fans.FW, fans.FH)
    want = gpu.render(pcs[1], fans.FW, fans.FH).copy()

    gpu.clear_framebuffer()
    first = gpu.render(pcs[0], fans.FW, fans.FH).copy()
    gpu.sync()
    before = dict(pipeline=gpu.last_pipeline(), parts=gpu.last_parts(), cost=gpu.ray_cost(), counters=gpu.counters())
    gpu.set_tuning("lanes_min_kslots", 0)
    gpu.set_tuning("lanes", 3)
    n = 700
    got = gpu.query_radiance(o[:n], d[:n], samples=5, bounces=3)
    after = dict(pipeline=gpu.last_pipeline(), parts=gpu.last_parts(), cost=gpu.ray_cost(), counters=gpu.counters())
    assert after["pipeline"] == before["pipeline"] and after["parts"] == before["parts"] == 1 and after["cost"] == before["cost"], (before, after)
    assert after["counters"]["paths"] - before["counters"]["paths"] == n * 5
    assert after["counters"]["segments"] - before["counters"]["segments"] >= n * 5
    assert after["counters"]["raysReference"] > before["counters"]["raysReference"]
    assert np.isfinite(got).all()
    _same(gpu.read_rgba(), first, "the ctx framebuffer after the query")
    gpu.set_tuning("lanes", 1)
    _same(gpu.render(pcs[1], fans.FW, fans.FH), want, "the second progressive frame with a query in between")


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals_through_python(gpu):
    gpu.upload_scene(cornell_scene(True))
    o = np.zeros((4, 3), np.float32)
    d = np.tile(np.array((0, 0, 1), np.float32), (4, 1))
    with pytest.raises(engine.RtError, match="samples must be >= 1"):
        gpu.query_radiance(o, d, samples=0)
    # tmax given: Renderer.query_radiance has no such argument, so through the C ABI as the renderer calls it
    t = np.ones(4, np.float32)
    out = np.zeros((4, 4), np.float32)
    batch = _capi.RtRayBatch(o.ctypes.data, d.ctypes.data, t.ctypes.data, 4)
    p = _capi.RtRadianceParams(1, 8, 0, 0)
    with pytest.raises(engine.RtError, match="tmax must be NULL"):
        gpu._check(gpu._l.rt_query_radiance_host(gpu._h, C.byref(batch), None, C.byref(p), None, out.ctypes.data), "rt_query_radiance_host")
    assert not out.any(), "a refused call writes nothing"
    fresh = engine.Renderer(0)
    try:
        with pytest.raises(engine.RtError, match="before rt_upload_scene"):
            fresh.query_radiance(o, d)
    finally:
        fresh.close()


def test_wrong_dtype_or_shape_raises_before_the_library_is_called():
    """(no GPU: the checks run before any entry point)"""
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")
    r = engine.Renderer.__new__(engine.Renderer)
    r._l, r._h = NoLibrary(), None
    o, d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for bad, err in (((o.astype(np.float64), d), TypeError), ((o, d.astype(np.float16)), TypeError), ((o.reshape(-1), d), ValueError),
                     ((o, d[:3]), ValueError), ((o[:, :2], d[:, :2]), ValueError)):
        with pytest.raises(err):
            r.query_radiance(*bad)
    with pytest.raises(TypeError):
        r.query_radiance(o, d, ids=np.arange(4))                     # int64
    with pytest.raises(ValueError):
        r.query_radiance(o, d, ids=np.arange(5, dtype=np.uint32))
    with pytest.raises(ValueError):
        r.query_radiance(o, d, progressive=True)                     # no previous result
    with pytest.raises(ValueError):
        r.query_radiance(o, d, progressive=True, out=np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError):
        r.query_radiance(o, d, progressive=True, out=np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError):
        r.query_radiance(o, d, sync=False)
    with pytest.raises(ValueError):
        r.query_radiance(o, 12345, n=4)                              # host origins, device dirs
    with pytest.raises(TypeError):
        r.query_radiance(o, d, environment=(0, 0, 0))
