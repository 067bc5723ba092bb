"""Baked light at points on the device: rt_query_irradiance and rt_query_sh_probes with their _host forms (Renderer.query_irradiance,
Renderer.query_sh_probes; include/rt_amd.h, DESIGN.md "Irradiance and SH probes").

The contract makes the device's answer a composition of pieces that are held elsewhere: the rays of the rule
(engine.irradiance_rays, held to float64 by tests/test_irradiance_host.py), rt_query_radiance on those rays (held to rt_render by
tests/test_radiance_queries.py) and the rule's sum (engine.irradiance_gather, held to a hand-written fold and to float64 sums on the
CPU). So the definition test asks for every bit. The shapes are the ones where the two kernels can go wrong: n = 37 points (no
multiple of the four waves of a work-group: a tail wave) and S = 1, 5, 64, 65, 200 (below a wave, one exact wave, one past,
several rounds with a ragged last one)."""
import ctypes as C
import math

import numpy as np
import pytest

from ray_tracer_amd import _capi, devmem, engine

import irradiance_float64 as f64
import radiance_fans as fans
from paths_float64 import _sky_scene, _spheres_scene
from util import bits, cornell_scene

N = 37
SAMPLES = (1, 5, 64, 65, 200)
BOUNCES = 3
DEFAULTS = dict(pipeline=-1, lanes=0, lanes_min_kslots=1024, radiance_max_kslots=0)
SKY = dict(lightDir=(0.3, 0.8, -0.5, 1.0), horizonColor=(0.9, 0.8, 0.7, 40.0), zenithColor=(0.2, 0.4, 0.9, 5.0), groundColor=(0.3, 0.25, 0.2))


@pytest.fixture
def gpu(renderer):
    """The session's renderer; afterwards a cleared progressive history and the knobs these tests turn at their defaults."""
    try:
        yield renderer
    finally:
        renderer.clear_framebuffer()
        for k, v in DEFAULTS.items():
            renderer.set_tuning(k, v)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
    bad = np.flatnonzero((bits(g) != bits(w)).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} of {len(g)} points differ, first at {bad[:5].tolist()}: {g[bad[:2]].tolist()} against {w[bad[:2]].tolist()}"


def _ids():
    """Caller ids in no order, with values whose product with S wraps."""
    ids = (np.arange(N, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    ids[3], ids[4] = 0xFFFFFFFF, 0
    return ids


def _cornell_points(gpu):
    """37 first-hit points of a small frame of the Cornell box with its spheres (floor, walls, ceiling, spheres), pushed along the
    normals, with the normals of the AOV pass. The scene stays uploaded."""
    gpu.upload_scene(cornell_scene(True))
    a = gpu.render_aovs(engine.push_constants(24, 18), 24, 18)
    hit = np.flatnonzero(a["hit"].reshape(-1))
    pick = hit[np.linspace(0, len(hit) - 1, N).astype(int)]
    nrm = np.ascontiguousarray(a["normal"].reshape(-1, 3)[pick], np.float32)
    pts = np.ascontiguousarray(a["position"].reshape(-1, 3)[pick] + np.float32(1e-3) * nrm, np.float32)
    assert len(np.unique(np.round(nrm, 3), axis=0)) >= 4, "the points lie on several surfaces"
    return pts, nrm, None


def _sky_points(gpu):
    """37 points on the upper side of the sky scene's ground sphere around its small spheres, pushed along the normals; its
    environment on."""
    gpu.upload_scene(_sky_scene())
    rng = np.random.default_rng(37)
    nrm = rng.normal(size=(N, 3)) * (0.35, 0.0, 0.35) + (0.0, -1.0, 0.0)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    pts = (np.array((0.0, 3.5, 0.0), np.float32) + np.float32(3.002) * nrm).astype(np.float32)
    return pts, nrm, engine.push_constants(8, 8, **SKY).environment


def _definition(gpu, pts, nrm, S, sphere, ids, frame, env):
    """irradiance_gather(query_radiance(irradiance_rays(...), ids=rayIds)): the definition, its pieces all public."""
    o, d, rid = engine.irradiance_rays(pts, None if sphere else nrm, samples=S, ids=ids, frame=frame)
    rad = gpu.query_radiance(o, d, samples=1, bounces=BOUNCES, ids=rid, frame=frame, environment=env)
    return engine.irradiance_gather(rad, len(pts), samples=S, ids=ids, frame=frame, sphere=sphere), rad


def _query(gpu, pts, nrm, S, sphere, **kw):
    if sphere:
        return gpu.query_sh_probes(pts, samples=S, bounces=BOUNCES, **kw)
    return gpu.query_irradiance(pts, nrm, samples=S, bounces=BOUNCES, **kw)


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sky"])
def test_device_equals_the_definition_in_every_bit(gpu, scene):
    """Both forms, every S, with the points' indices and with caller ids, frames 0 and 2: the device's rays, ids, weights and fold
    at once. The answers are not flat: the points differ, and lit points are not black."""
    pts, nrm, env = (_cornell_points if scene == "cornell" else _sky_points)(gpu)
    for sphere in (False, True):
        for S in SAMPLES:
            for ids, frame in ((None, 0), (_ids(), 2)):
                what = f"{scene}, {'probes' if sphere else 'irradiance'}, S {S}, {'caller ids' if ids is not None else 'no ids'}, frame {frame}"
                want, rad = _definition(gpu, pts, nrm, S, sphere, ids, frame, env)
                got = _query(gpu, pts, nrm, S, sphere, ids=ids, frame=frame, environment=env)
                assert "k_trace_pw" in gpu.last_kernel(), gpu.last_kernel()
                _same(got, want, what)
                assert got.shape == ((N, 9, 3) if sphere else (N, 4))
                if not sphere:
                    assert (got[:, 3] == 1.0).all()
                if S >= 64:
                    assert np.isfinite(got).all() and got[..., :3].max() > 0.0 and len(np.unique(bits(got[..., 0, :1] if sphere else got[:, :1]))) > N // 2, what


@pytest.mark.gpu
def test_device_pointers_equal_the_host_forms(gpu):
    """The asynchronous forms on device memory the test owns (integer pointers with n=), sync=False then rt_sync: the same bits as
    the _host forms, with caller ids; the output's neighbours stay as they were."""
    pts, nrm, env = _sky_points(gpu)
    ids = _ids()
    bufs = []

    def device(a):
        bufs.append(devmem.DeviceBuffer(a.nbytes).upload(a))
        return bufs[-1]

    try:
        d_p, d_n, d_i = device(pts).ptr, device(nrm).ptr, device(ids).ptr
        for sphere, width in ((False, 4), (True, 27)):
            for S in (5, 65):
                host = _query(gpu, pts, nrm, S, sphere, ids=ids, frame=1, environment=env)
                out = device(np.full((N + 1, width), 7.0, np.float32))
                assert _query(gpu, d_p, d_n, S, sphere, ids=d_i, frame=1, environment=env, n=N, out=out.ptr, sync=False) is None
                gpu.sync()
                got = out.download((N + 1, width), np.float32)
                _same(got[:N].reshape(host.shape), host, f"device pointers, sphere {sphere}, S {S}")
                assert (got[N] == 7.0).all(), "the floats behind the last point's are not the pass's"
        with pytest.raises(ValueError):
            gpu.query_irradiance(d_p, d_n, out=bufs[-1].ptr)             # integer pointers need n=
        with pytest.raises(ValueError):
            gpu.query_sh_probes(d_p, n=N)                                # ... and out=
    finally:
        gpu.sync()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_torch_tensors_equal_the_host_forms(gpu):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    pts, nrm, env = _sky_points(gpu)
    dev = torch.device("cuda:0")
    tp, tn = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
    ti = torch.from_numpy(_ids().astype(np.int32)).to(dev)
    E = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    c = torch.zeros((N, 9, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    gpu.query_irradiance(tp, tn, samples=65, bounces=BOUNCES, ids=ti, environment=env, out=E, sync=False)
    gpu.query_sh_probes(tp, samples=65, bounces=BOUNCES, ids=ti, environment=env, out=c)
    _same(E.cpu().numpy(), gpu.query_irradiance(pts, nrm, samples=65, bounces=BOUNCES, ids=_ids(), environment=env), "torch, irradiance")
    _same(c.cpu().numpy(), gpu.query_sh_probes(pts, samples=65, bounces=BOUNCES, ids=_ids(), environment=env), "torch, probes")
    with pytest.raises(ValueError):
        gpu.query_sh_probes(tp, out=E)                                   # too small
    with pytest.raises(ValueError):
        gpu.query_irradiance(tp, tn.double(), out=E)


# ---------------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.gpu
def test_chunks_and_permutations_change_no_bit(gpu):
    """"radiance_max_kslots" 1 (1024 rays a piece): 37 points of 64 samples run in three chunks, of 65 in three, of 200 in eight,
    each in parts as well, with the bits of the single-chunk run; and a batch permuted with its ids carried along gives each point
    its answer."""
    pts, nrm, env = _sky_points(gpu)
    ids = _ids()
    perm = np.random.default_rng(5).permutation(N)
    for sphere in (False, True):
        for S in (64, 65, 200):
            gpu.set_tuning("radiance_max_kslots", 0)
            gpu.set_tuning("lanes", 0)
            gpu.set_tuning("lanes_min_kslots", 1024)
            one = _query(gpu, pts, nrm, S, sphere, ids=ids, environment=env)
            moved = _query(gpu, pts[perm].copy(), nrm[perm].copy(), S, sphere, ids=ids[perm].copy(), environment=env)
            _same(moved, one[perm], f"permuted, sphere {sphere}, S {S}")
            _same(_query(gpu, pts[:5].copy(), nrm[:5].copy(), S, sphere, ids=ids[:5].copy(), environment=env), one[:5], "the first five points alone")
            gpu.set_tuning("radiance_max_kslots", 1)
            _same(_query(gpu, pts, nrm, S, sphere, ids=ids, environment=env), one, f"chunks of 1024 rays, sphere {sphere}, S {S}")
            gpu.set_tuning("lanes_min_kslots", 0)
            gpu.set_tuning("lanes", 3)
            _same(_query(gpu, pts, nrm, S, sphere, ids=ids, environment=env), one, f"chunks in three parts, sphere {sphere}, S {S}")


# ---------------------------------------------------------------------------------------------------------------- the analytic pin
@pytest.mark.gpu
def test_constant_sky_gives_pi_L_and_two_root_pi_L(gpu):
    """One colour L for horizon, zenith and ground, sun intensity 0, and points far from the scene's one small sphere, so that no ray
    reaches a surface (checked: rt_query_occluded on the rule's rays): E = pi L and c_0 = 2 sqrt(pi) L, and c_1..c_8 are the float64
    restatement's projection of its own directions. The bound is tests/irradiance_float64.py's for the sum, with the records'
    own roundings added: a record is mix(L, mix(L, L, skyT), g2s) + 0, two products and a sum per mix, so L (1 + d) with
    |d| <= 6u, which the linear sum passes on: + 6u x 1.1 |L| x 4 pi for a coefficient, + 6u pi |L| for E."""
    gpu.upload_scene(_spheres_scene([dict(albedo=(0.5, 0.5, 0.5))], [((0.0, 0.0, 0.0), 0.01, 0)]))
    L = np.array((0.75, 2.0, 0.125), np.float32)
    env = engine.push_constants(8, 8, lightDir=(0.0, 1.0, 0.0, 1.0), horizonColor=(*L, 1.0), zenithColor=(*L, 0.0), groundColor=tuple(L)).environment
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=(N, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    pts = (np.float32(500.0) * nrm + rng.normal(size=(N, 3)).astype(np.float32)).astype(np.float32)    # the normals point away from the origin
    L64 = L.astype(np.float64)
    for S in (65, 200):
        for sphere in (False, True):
            o, d, _ = engine.irradiance_rays(pts, None if sphere else nrm, samples=S)
            assert not gpu.query_occluded(o, d).any(), "a ray of the rule reaches the sphere: move the points"
        rad = np.ones((N * S, 4), np.float32)
        rad[:, :3] = L
        E = gpu.query_irradiance(pts, nrm, samples=S, bounces=BOUNCES, environment=env)
        _, bound = f64.irradiance(rad, N, S)
        err = np.abs(E[:, :3] - math.pi * L64)
        print(f"S {S}: E off by at most {(err / (bound + 6 * f64.U * math.pi * L64)).max():.3f} of the bound")
        assert (err <= bound + 6 * f64.U * math.pi * L64).all(), (S, err.max())
        c = gpu.query_sh_probes(pts, samples=S, bounces=BOUNCES, environment=env)
        want, bound = f64.probes(rad, None, 0, N, S)
        bound = bound + 6 * f64.U * 1.1 * 4 * math.pi * L64
        err = np.abs(c - want)
        print(f"S {S}: c off by at most {(err / bound).max():.3f} of the bound")
        assert (err <= bound).all(), (S, np.argwhere(err > bound)[:3].tolist())
        assert (np.abs(c[:, 0] - 2.0 * math.sqrt(math.pi) * L64) <= bound[:, 0]).all()


# ---------------------------------------------------------------------------------------------------------------- progressive
@pytest.mark.gpu
def test_two_progressive_calls_equal_the_host_blend(gpu):
    """Frames 0 and 1 with progressive = 1, the first result fed back, equal the host's blend (weight 1 / (frameCount + 1), rt_render's
    arithmetic) of the two single results, on host arrays and in device memory."""
    pts, nrm, env = _sky_points(gpu)
    for sphere, width in ((False, 4), (True, 27)):
        S = 65
        singles = [_query(gpu, pts, nrm, S, sphere, frame=f, environment=env) for f in (0, 1)]
        assert not np.array_equal(singles[0], singles[1])
        zero = np.zeros_like(singles[0])
        first = _query(gpu, pts, nrm, S, sphere, frame=0, progressive=True, out=zero, environment=env)
        _same(first, singles[0], "frame 0 on top of anything is frame 0")      # weight 1: old * 0 + new * 1
        second = _query(gpu, pts, nrm, S, sphere, frame=1, progressive=True, out=first, environment=env)
        w = np.float32(1.0) / (np.float32(1.0) + np.float32(1.0))
        want = singles[0] * (np.float32(1.0) - w) + singles[1] * w
        if not sphere:
            want[:, 3] = 1.0
        _same(second, want, f"two progressive calls, sphere {sphere}")
        buf = [devmem.DeviceBuffer(a.nbytes).upload(a) for a in (pts, nrm, np.ascontiguousarray(first))]
        try:
            _query(gpu, buf[0].ptr, buf[1].ptr, S, sphere, frame=1, progressive=True, n=N, out=buf[2].ptr, environment=env)
            _same(buf[2].download((N, width), np.float32).reshape(want.shape), want, f"progressive in device memory, sphere {sphere}")
        finally:
            gpu.sync()
            for b in buf:
                b.free()


# ---------------------------------------------------------------------------------------------------------------- what it leaves alone
@pytest.mark.gpu
def test_query_leaves_rendering_alone(gpu):
    """Two progressive frames into the ctx framebuffer with both queries between them (in chunks and parts) equal the two frames
    without; rt_last_pipeline, rt_last_parts and rt_ray_cost are what they were; rt_get_counters().paths grows by n x S."""
    gpu.upload_scene(fans.scene())
    pcs = [fans.fan_constants(0, 2, 3, frame=f, progressive=1) for f in (0, 1)]
    gpu.set_tuning("pipeline", 0)
    gpu.set_tuning("lanes", 1)
    gpu.clear_framebuffer()
    gpu.render(pcs[0], fans.FW, fans.FH)
    want = gpu.render(pcs[1], fans.FW, fans.FH).copy()
    a = gpu.render_aovs(pcs[0], fans.FW, fans.FH)
    hit = np.flatnonzero(a["hit"].reshape(-1))[:N]
    nrm = np.ascontiguousarray(a["normal"].reshape(-1, 3)[hit], np.float32)
    pts = np.ascontiguousarray(a["position"].reshape(-1, 3)[hit] + np.float32(1e-3) * nrm, np.float32)

    gpu.clear_framebuffer()
    first = gpu.render(pcs[0], fans.FW, fans.FH).copy()
    gpu.sync()
    before = dict(pipeline=gpu.last_pipeline(), parts=gpu.last_parts(), cost=gpu.ray_cost(), counters=gpu.counters())
    gpu.set_tuning("lanes_min_kslots", 0)
    gpu.set_tuning("lanes", 3)
    gpu.set_tuning("radiance_max_kslots", 1)
    E = gpu.query_irradiance(pts, nrm, samples=65, bounces=3)
    c = gpu.query_sh_probes(pts, samples=200, bounces=3)
    after = dict(pipeline=gpu.last_pipeline(), parts=gpu.last_parts(), cost=gpu.ray_cost(), counters=gpu.counters())
    assert after["pipeline"] == before["pipeline"] and after["parts"] == before["parts"] == 1 and after["cost"] == before["cost"], (before, after)
    assert after["counters"]["paths"] - before["counters"]["paths"] == N * (65 + 200)
    assert np.isfinite(E).all() and np.isfinite(c).all() and E[:, :3].max() > 0.0
    _same(gpu.read_rgba().reshape(-1, 4), first.reshape(-1, 4), "the ctx framebuffer after the queries")
    gpu.set_tuning("lanes", 1)
    gpu.set_tuning("radiance_max_kslots", 0)
    _same(gpu.render(pcs[1], fans.FW, fans.FH).reshape(-1, 4), want.reshape(-1, 4), "the second progressive frame with the queries in between")


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals_through_python(gpu):
    gpu.upload_scene(cornell_scene(True))
    p = np.zeros((4, 3), np.float32)
    nrm = np.tile(np.array((0, -1, 0), np.float32), (4, 1))
    for query in (lambda **kw: gpu.query_irradiance(p, nrm, **kw), lambda **kw: gpu.query_sh_probes(p, **kw)):
        with pytest.raises(engine.RtError, match="samples must be in 1 .. 2\\^24 - 1"):
            query(samples=0)
        with pytest.raises(engine.RtError, match="samples must be in 1 .. 2\\^24 - 1"):
            query(samples=1 << 24)
        with pytest.raises(engine.RtError, match="bounceLimit needs more than 28 bits"):
            query(bounces=(1 << 28) - 1)
        gpu.set_tuning("radiance_max_kslots", 1)
        with pytest.raises(engine.RtError, match="the 1025 rays of a point do not fit a piece of 1024 rays"):
            query(samples=1025)
        gpu.set_tuning("radiance_max_kslots", 0)
    for bias in (-1e-5, float("inf"), float("nan")):
        with pytest.raises(engine.RtError, match="bias must be finite and >= 0"):
            gpu.query_irradiance(p, nrm, bias=bias)
    # a NULL normals array: through the C ABI as the renderer calls it; nothing is written
    out = np.zeros((4, 4), np.float32)
    batch = _capi.RtPointNormalBatch(p.ctypes.data, None, 4)
    params = _capi.RtIrradianceParams(4, 8, 0, 0, 1e-5)
    with pytest.raises(engine.RtError, match="points, normals and the output are required"):
        gpu._check(gpu._l.rt_query_irradiance_host(gpu._h, C.byref(batch), None, C.byref(params), None, out.ctypes.data), "rt_query_irradiance_host")
    assert not out.any(), "a refused call writes nothing"
    probes = np.zeros((4, 9, 3), np.float32)
    gpu._check(gpu._l.rt_query_sh_probes_host(gpu._h, C.byref(batch), None, C.byref(params), None, probes.ctypes.data), "rt_query_sh_probes_host")   # the probe form ignores them
    assert gpu.query_irradiance(p[:0], nrm[:0]).shape == (0, 4) and gpu.query_sh_probes(p[:0]).shape == (0, 9, 3)
    fresh = engine.Renderer(0)
    try:
        with pytest.raises(engine.RtError, match="before rt_upload_scene"):
            fresh.query_irradiance(p, nrm)
        with pytest.raises(engine.RtError, match="before rt_upload_scene"):
            fresh.query_sh_probes(p)
    finally:
        fresh.close()


def test_wrong_dtype_or_shape_raises_before_the_library_is_called():
    """(no GPU: the checks run before any entry point)"""
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")
    r = engine.Renderer.__new__(engine.Renderer)
    r._l, r._h = NoLibrary(), None
    p, nrm = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    for bad, err in (((p.astype(np.float64), nrm), TypeError), ((p, nrm.astype(np.float16)), TypeError), ((p.reshape(-1), nrm), ValueError),
                     ((p, nrm[:3]), ValueError), ((p[:, :2], nrm[:, :2]), ValueError)):
        with pytest.raises(err):
            r.query_irradiance(*bad)
    for bad, err in ((p.astype(np.float64), TypeError), (p.reshape(-1), ValueError), (p[:, :2], ValueError)):
        with pytest.raises(err):
            r.query_sh_probes(bad)
    for query, shape in ((lambda **kw: r.query_irradiance(p, nrm, **kw), (4, 4)), (lambda **kw: r.query_sh_probes(p, **kw), (4, 9, 3))):
        with pytest.raises(TypeError):
            query(ids=np.arange(4))                                      # int64
        with pytest.raises(ValueError):
            query(ids=np.arange(5, dtype=np.uint32))
        with pytest.raises(ValueError):
            query(progressive=True)                                      # no previous result
        with pytest.raises(ValueError):
            query(progressive=True, out=np.zeros((4, 5), np.float32))
        with pytest.raises(TypeError):
            query(progressive=True, out=np.zeros(shape, np.float64))
        with pytest.raises(ValueError):
            query(out=np.zeros(shape, np.float32))                       # out= without progressive
        with pytest.raises(ValueError):
            query(sync=False)
        with pytest.raises(ValueError):
            query(samples=-1)
        with pytest.raises(TypeError):
            query(environment=(0, 0, 0))
    with pytest.raises(ValueError):
        r.query_irradiance(p, 12345, n=4)                                # host points, device normals
