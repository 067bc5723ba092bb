"""Per-pixel sample counts: rt_render_sampled and rt_build_sample_map ("Per-pixel sample counts").

A pixel's samples are serial and its RNG seed depends on its global pixel index and frameCount only, so "pixel p rendered with n
samples" is defined, bit for bit, by rt_render at samples = n. That is the oracle of every render test here: the S uniform images
at 1..S samples, rendered into the same prefilled buffer, and pixel p of the sampled render must be pixel p of image
min(map[p], S) — or, for a count of 0, the prefill in all four channels. The sizes are the smallest that cross every boundary:
70 x 33 (2310 pixels: no multiple of 64, 8 or 256, three parts of the multi-kernel pipeline when forced) and its tile row0 = 1,
rowStride = 3 (770 pixels); the map is seeded random in 0..6 (so counts above S = 4 clamp) with a whole 8 x 8 block of zeros, a run
of 64 consecutive zero slots, zero at the first and the last pixel and one full row at S.
rt_build_sample_map is held to a numpy float32 restatement of its rule, written here in the stated operation order and sharing no
code with the kernel: counts and all five statistics equal."""
import concurrent.futures
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import _capi, engine, session

from util import bits, cornell_scene, model_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, S = 70, 33, 4
GEOMETRIES = {"frame": dict(row0=0, rowStride=1), "tile": dict(row0=1, rowStride=3)}
COUNTERS = [n for n, _ in _capi.RtCounters._fields_]
DEFAULTS = (("pipeline", -1), ("lanes", 0), ("lanes_min_kslots", 1024), ("camera_reuse", 1), ("fused_maps", 0), ("pixel_refill", 0),
            ("scatter", -1))
# (pipeline, knobs, parts expected on the whole frame)
CONFIGS = [("multi-kernel, one part", dict(pipeline=0, lanes=1), 1),
           ("multi-kernel, three parts", dict(pipeline=0, lanes=3, lanes_min_kslots=1), 3),
           ("fused", dict(pipeline=1), None),
           ("fused, a block at a time", dict(pipeline=1, pixel_refill=64, scatter=0), None)]


def n_rows(geometry):
    g = GEOMETRIES[geometry]
    return (H - g["row0"] + g["rowStride"] - 1) // g["rowStride"]


def the_map(rows, seed=11):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 7, (rows, W)).astype(np.uint32)
    m[9, :] = S                      # one full row at S
    m[0:8, 8:16] = 0                 # a whole 8 x 8 block
    m.reshape(-1)[200:264] = 0       # 64 consecutive slots
    m[0, 0] = 0
    m[-1, -1] = 0
    assert (m > S).any() and (m == 0).sum() > 130 and ((m > 0) & (m < S)).any()
    return m


def sentinel(rows, seed=3):
    """The prefill: seeded finite values in every channel (the progressive tests blend with them), alpha never 1."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (rows, W, 4)).astype(np.float32)
    p[..., 3] = 0.25
    return p


class DeviceImage:
    """A device buffer of one (rows, W, 4) float32 image, from the HIP runtime the library is bound to."""

    def __init__(self, rows):
        self.hip = C.CDLL(_capi.LIB_PATH)
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.shape = (rows, W, 4)
        self.nbytes = rows * W * 16
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), self.nbytes) == 0

    @property
    def ptr(self):
        return self.p.value

    def put(self, a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.shape == self.shape
        assert self.hip.hipMemcpy(self.p, a.ctypes.data, self.nbytes, 1) == 0   # hipMemcpyHostToDevice

    def get(self):
        out = np.empty(self.shape, np.float32)
        assert self.hip.hipMemcpy(out.ctypes.data, self.p, self.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out

    def close(self):
        if self.p.value:
            self.hip.hipFree(self.p)
            self.p = C.c_void_p()


@pytest.fixture
def tuned(renderer):
    """The renderer; afterwards every knob the cases set, and the texture tables, back to their defaults."""
    try:
        yield renderer
    finally:
        pyoracle.set_textures([])
        renderer.upload_textures([])
        for k, v in DEFAULTS:
            renderer.set_tuning(k, v)


@pytest.fixture
def images():
    made = {}

    def get(rows):
        if rows not in made:
            made[rows] = DeviceImage(rows)
        return made[rows]
    yield get
    for d in made.values():
        d.close()


def tune(r, knobs):
    for k, v in DEFAULTS:
        r.set_tuning(k, v)
    for k, v in knobs.items():
        r.set_tuning(k, v)


def expected(uniform, counts, untouched):
    """Pixel p of image min(counts[p], S), or of `untouched` where the count is 0. uniform[n - 1]: the image at n samples."""
    n = np.minimum(counts, S)
    out = untouched.copy()
    for k in range(1, S + 1):
        out[n == k] = uniform[k - 1][n == k]
    return out


def same(got, want, counts, what):
    d = (bits(got) != bits(want)).any(axis=-1)
    assert not d.any(), (f"{what}: {int(d.sum())} pixels differ, of them {int((d & (counts == 0)).sum())} with a count of 0; first "
                         f"{np.argwhere(d)[:4].tolist()}")


# ---------------------------------------------------------------- scenes
def upload_cornell(r, tmp_path):
    s = cornell_scene(True)
    r.upload_textures([])
    r.upload_scene(s)
    return s


def upload_bunny(r, tmp_path):
    s = model_scene("bunny.obj")
    r.upload_textures([])
    r.upload_scene(s)
    return s


def upload_maps(r, tmp_path):
    """The plane scene with an alpha, a metalness and a bump map bound, as tests/test_fused_maps.py builds it."""
    from texture_cases import _bound, _map_set
    s = _bound(tmp_path / "maps", 1, 2.5, alphaIndex=1, metalnessIndex=2, bumpIndex=3)
    r.upload_scene(s.scene)
    s.push(r, "objects")
    s.push(r, "materials")
    r.upload_textures(_map_set())
    return s


SCENES = {"cornell": upload_cornell, "bunny": upload_bunny, "maps": upload_maps}


def constants(n, **kw):
    return engine.push_constants(W, H, singleRender=1, sampleLimit=n, environmentOn=True, **kw)


# ---------------------------------------------------------------- 1. per-pixel equivalence
@pytest.mark.parametrize("scene", list(SCENES))
def test_every_pixel_is_the_uniform_render_at_its_own_count(tuned, images, tmp_path, scene):
    r = tuned
    s = SCENES[scene](r, tmp_path)
    for geometry, g in GEOMETRIES.items():
        rows = n_rows(geometry)
        counts, fill, buf = the_map(rows), sentinel(rows), images(rows)
        tune(r, {})
        uniform = []
        for n in range(1, S + 1):   # the reference: rt_render at 1..S samples into the same prefill
            buf.put(fill)
            r.render(constants(n), W, H, nRows=rows, out_ptr=buf.ptr, **g)
            uniform.append(buf.get())
            assert not (bits(uniform[-1]) == bits(fill)).all(axis=-1).any()
        assert all(not np.array_equal(uniform[k], uniform[k + 1]) for k in range(S - 1))
        if scene == "cornell":   # ... which does not rest on the GPU alone: the fused pipeline's uniform renders against the oracle
            tune(r, dict(pipeline=1))
            for n in range(1, S + 1):
                buf.put(fill)
                r.render(constants(n), W, H, nRows=rows, out_ptr=buf.ptr, **g)
                assert r.last_pipeline() == 1
                same(buf.get(), uniform[n - 1], counts, f"uniform {n}, {geometry}: fused against the default pipeline")
                ref, _ = pyoracle.render(s, constants(n), W, H, nRows=rows, **g)   # (not progressive: the prefill does not show)
                same(buf.get(), ref, counts, f"uniform {n}, {geometry}: fused against the oracle")
        want = expected(uniform, counts, fill)
        for name, knobs, parts in CONFIGS:
            for reuse in (0, 1):
                tune(r, dict(knobs, camera_reuse=reuse, fused_maps=1 if scene == "maps" else 0))
                buf.put(fill)
                assert r.render_sampled(constants(S), W, H, counts, nRows=rows, out_ptr=buf.ptr, **g) is None
                what = f"{scene}, {geometry}, {name}, camera_reuse {reuse} ({r.last_kernel()})"
                assert r.last_pipeline() == knobs["pipeline"], what
                if parts and geometry == "frame":
                    assert r.last_parts() == parts, what
                if scene == "maps" and knobs["pipeline"] == 1:
                    assert r.last_kernel().startswith("k_render_fused_maps<"), what
                same(buf.get(), want, counts, what)


# ---------------------------------------------------------------- 2. progressive, several frames, the ctx framebuffer
@pytest.mark.parametrize("pipeline", [0, 1])
def test_progressive_frames_and_the_ctx_framebuffer(tuned, images, tmp_path, pipeline):
    r = tuned
    upload_cornell(r, tmp_path)
    knobs = dict(pipeline=pipeline, lanes=3, lanes_min_kslots=1)
    frames = 3

    def pc_of(n, frameCount=3):
        return engine.push_constants(W, H, raysPerPixel=n, progressive=1, frameCount=frameCount, environmentOn=True)

    for geometry, g in GEOMETRIES.items():
        rows = n_rows(geometry)
        counts, fill, buf = the_map(rows), sentinel(rows), images(rows)
        tune(r, knobs)
        uniform = []
        for n in range(1, S + 1):
            buf.put(fill)
            r.render_frames(pc_of(n), W, H, frames, nRows=rows, out_ptr=buf.ptr, **g)
            uniform.append(buf.get())
        buf.put(fill)
        r.render_sampled(pc_of(S), W, H, counts, nFrames=frames, nRows=rows, out_ptr=buf.ptr, **g)
        if pipeline == 0:
            assert r.last_parts() == 3   # 3 frames of 832 or 2368 slots: more than 1024 paths
        same(buf.get(), expected(uniform, counts, fill), counts, f"{geometry}, pipeline {pipeline}: three progressive frames")
        # a call rt_render_frames would split uses the same map for every piece
        r.set_tuning("frames_per_launch", 2)
        try:
            buf.put(fill)
            r.render_sampled(pc_of(S), W, H, counts, nFrames=frames, nRows=rows, out_ptr=buf.ptr, **g)
        finally:
            r.set_tuning("frames_per_launch", 0)
        same(buf.get(), expected(uniform, counts, fill), counts, f"{geometry}, pipeline {pipeline}: three frames in two dispatches")

        # the ctx framebuffer (d_rgba = NULL) and its progressive history over two consecutive calls
        uniform = []
        for n in range(1, S + 1):
            r.clear_framebuffer()
            r.render_frames(pc_of(n, 0), W, H, 2, nRows=rows, **g)
            uniform.append(r.render_frames(pc_of(n, 2), W, H, 2, nRows=rows, **g))
        r.clear_framebuffer()
        r.render_sampled(pc_of(S, 0), W, H, counts, nFrames=2, nRows=rows, **g)
        got = r.render_sampled(pc_of(S, 2), W, H, counts, nFrames=2, nRows=rows, **g)
        same(got, expected(uniform, counts, np.zeros((rows, W, 4), np.float32)), counts, f"{geometry}, pipeline {pipeline}: ctx framebuffer")
    r.clear_framebuffer()


# ---------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("pipeline,bounces", [(0, 1), (1, 8)])
def test_a_map_of_S_and_no_map_are_render_frames(tuned, images, tmp_path, pipeline, bounces):
    """Pixels, every RtCounters field and rt_last_kernel / rt_last_parts / rt_last_pipeline. (The multi-kernel pipeline stops
    enqueuing rounds when a count of active paths that it polls without waiting arrives as zero, so its traceLaunches depends on
    timing from eight rounds on: its case has S * (bounceLimit + 1) = 8 rounds, which are always all enqueued.)"""
    r = tuned
    upload_cornell(r, tmp_path)
    tune(r, dict(pipeline=pipeline, lanes=3, lanes_min_kslots=1))
    g, rows = GEOMETRIES["frame"], n_rows("frame")
    buf, fill = images(rows), sentinel(rows)
    pc = engine.push_constants(W, H, raysPerPixel=S, progressive=1, frameCount=5, bounceLimit=bounces)
    plain = constants(2, bounceLimit=bounces)

    def run(call):
        buf.put(fill)
        r.reset_counters()
        call()
        r.sync()
        c = r.counters()
        return buf.get(), {k: c[k] for k in COUNTERS}, (r.last_kernel(), r.last_parts(), r.last_pipeline())

    before = run(lambda: r.render(plain, W, H, out_ptr=buf.ptr))
    ref = run(lambda: r.render_frames(pc, W, H, 2, out_ptr=buf.ptr, **g))
    full = run(lambda: r.render_sampled(pc, W, H, np.full((rows, W), S, np.uint32), nFrames=2, out_ptr=buf.ptr, **g))
    more = run(lambda: r.render_sampled(pc, W, H, np.full((rows, W), S + 3, np.uint32), nFrames=2, out_ptr=buf.ptr, **g))
    none = run(lambda: r.render_sampled(pc, W, H, None, nFrames=2, out_ptr=buf.ptr, **g))
    after = run(lambda: r.render(plain, W, H, out_ptr=buf.ptr))
    assert ref[1]["paths"] == 2 * S * rows * W and ref[2][2] == pipeline
    for name, got in (("map of S", full), ("map above S", more), ("no map", none)):
        assert np.array_equal(bits(got[0]), bits(ref[0])), name
        assert got[1] == ref[1], (name, got[1], ref[1])
        assert got[2] == ref[2], (name, got[2], ref[2])
    assert np.array_equal(bits(after[0]), bits(before[0])) and after[1] == before[1] and after[2] == before[2]


# ---------------------------------------------------------------- 4. empty, 5. accounting
@pytest.mark.parametrize("pipeline", [0, 1])
def test_an_all_zero_map_touches_nothing(tuned, images, tmp_path, pipeline):
    r = tuned
    upload_cornell(r, tmp_path)
    tune(r, dict(pipeline=pipeline))
    for geometry, g in GEOMETRIES.items():
        rows = n_rows(geometry)
        buf, fill = images(rows), sentinel(rows)
        buf.put(fill)
        r.reset_counters()
        pool = concurrent.futures.ThreadPoolExecutor(1)   # (no `with`: leaving it would wait for a call that hangs)
        try:
            job = pool.submit(lambda: r.render_sampled(constants(S), W, H, np.zeros((rows, W), np.uint32), nFrames=2, nRows=rows, out_ptr=buf.ptr, **g))
            job.result(timeout=30)   # enqueued, run and synchronised
        finally:
            pool.shutdown(wait=False)
        assert np.array_equal(bits(buf.get()), bits(fill)), geometry
        c = r.counters()
        assert c["paths"] == 0 and c["segments"] == 0 and c["raysTraced"] == 0, c


@pytest.mark.parametrize("pipeline", [0, 1])
def test_paths_count_the_samples_of_the_map(tuned, images, tmp_path, pipeline):
    r = tuned
    upload_bunny(r, tmp_path)
    tune(r, dict(pipeline=pipeline, lanes=3, lanes_min_kslots=1))
    for geometry, g in GEOMETRIES.items():
        rows = n_rows(geometry)
        counts, buf = the_map(rows), images(rows)
        for frames in (1, 2):
            r.reset_counters()
            r.render_sampled(constants(S), W, H, counts, nFrames=frames, nRows=rows, out_ptr=buf.ptr, **g)
            assert r.counters()["paths"] == frames * int(np.minimum(counts, S).sum()), (geometry, frames)


# ---------------------------------------------------------------- 6. refusals
def test_heat_maps_with_a_map_are_refused(tuned, images, tmp_path):
    r = tuned
    upload_cornell(r, tmp_path)
    tune(r, {})
    rows = n_rows("frame")
    buf, fill, counts = images(rows), sentinel(rows), the_map(rows)
    buf.put(fill)
    r.render(constants(2), W, H, out_ptr=buf.ptr)
    before = buf.get()
    r.reset_counters()
    buf.put(fill)
    for dbg in (0, 1, 2):
        with pytest.raises(engine.RtError, match="rt_render_sampled: the debug heat maps take no sample map"):
            r.render_sampled(constants(S, debug=dbg), W, H, counts, out_ptr=buf.ptr)
    r.sync()
    assert np.array_equal(bits(buf.get()), bits(fill)) and r.counters()["paths"] == 0
    heat = constants(2, debug=0)
    buf.put(fill)
    r.render_sampled(heat, W, H, None, out_ptr=buf.ptr)   # without a map it is rt_render_frames, heat maps included
    a = buf.get()
    buf.put(fill)
    r.render(heat, W, H, out_ptr=buf.ptr)
    assert np.array_equal(bits(a), bits(buf.get()))
    with pytest.raises(ValueError):
        r.render_sampled(constants(S), W, H, counts[:-1], out_ptr=buf.ptr)   # not the tile's shape
    buf.put(fill)
    r.render(constants(2), W, H, out_ptr=buf.ptr)
    assert np.array_equal(bits(buf.get()), bits(before))


# ---------------------------------------------------------------- 7. rt_build_sample_map against a numpy float32 restatement
PARAMS = dict(base_samples=4, min_samples=1, max_samples=16, target_rel_error=0.0625, luminance_floor=0.01)   # tau = 2^-4: tau * tau is exact


LIBRARY_DEFAULTS = dict(base_samples=4, min_samples=1, max_samples=16, target_rel_error=0.05, luminance_floor=0.01)


def restated(mom, base_samples, min_samples, max_samples, target_rel_error, luminance_floor):
    """The rule of rt_amd.h in numpy float32, in its stated order. Returns (counts, stats)."""
    f = np.float32
    mom = np.asarray(mom, np.float32)
    m1, var, N = mom[..., 0], mom[..., 2], mom[..., 3]
    with np.errstate(all="ignore"):
        d = np.fmax(m1, f(luminance_floor))
        den = (N * (f(target_rel_error) * f(target_rel_error))) * (d * d)
        q = (f(base_samples) * var) / den
        assert d.dtype == den.dtype == q.dtype == np.float32
        below = q < f(max_samples)                                   # false for a NaN q
        c = np.where(below, np.where(q > f(0), np.ceil(np.where(below, q, f(0))), f(0)), f(max_samples)).astype(np.uint32)
    n = np.maximum(np.uint32(min_samples), c)
    unknown = (N > f(0)) & (N < f(2))
    n = np.where(N == f(0), np.uint32(min_samples), np.where(unknown, np.uint32(base_samples), n)).astype(np.uint32)
    stats = dict(samples=int(n.sum(dtype=np.uint64)), pixels=int(n.size), unknown=int(unknown.sum()), aboveMin=int((n > min_samples).sum()),
                 atMax=int((n == max_samples).sum()))
    return n, stats, q


def near_a_step(mom, p):
    """Pixels of the general case whose float64 q lies within 2^-20, relative, of an integer or of maxSamples."""
    m = np.asarray(mom, np.float64)
    with np.errstate(all="ignore"):
        d = np.maximum(m[..., 0], float(np.float32(p["luminance_floor"])))
        tau = float(np.float32(p["target_rel_error"]))
        q = (p["base_samples"] * m[..., 2]) / ((m[..., 3] * (tau * tau)) * (d * d))
        near = (np.abs(q - np.rint(q)) <= 2.0 ** -20 * np.maximum(np.abs(q), 1.0)) & (q < p["max_samples"])   # (beyond it every q clamps)
        near |= np.abs(q - p["max_samples"]) <= 2.0 ** -20 * p["max_samples"]
    return near & (m[..., 3] >= 2.0) & np.isfinite(q) & (q > 0)


def synthetic_moments(w, h, seed):
    """Seeded planes with every case of the rule. Returns (moments, mask of the deliberate exact-integer pixels)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    mom = np.empty((h, w, 4), np.float32)
    mom[..., 0] = rng.uniform(0.02, 2.0, (h, w))                       # m1
    mom[..., 3] = np.floor(rng.uniform(2.0, 33.0, (h, w)))             # N, and a few fractional ones as bilinear taps give them
    frac = rng.uniform(size=(h, w)) < 0.2
    mom[..., 3][frac] += rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)[frac]
    rel = 10.0 ** rng.uniform(-3.0, 0.5, (h, w))                       # relative standard deviation of one frame
    mom[..., 2] = (rel * mom[..., 0]) ** 2
    mom[..., 1] = mom[..., 2] + mom[..., 0] ** 2
    kind = rng.integers(0, 20, (h, w))
    mom[kind == 0] = 0.0                                               # kept pixels: N = 0, moments 0
    mom[..., 3][kind == 1] = 1.0                                       # one frame
    mom[..., 2][kind == 2] = 0.0                                       # no variance
    mom[..., 0][kind == 3] = rng.uniform(0.0, 0.01, (h, w)).astype(np.float32)[kind == 3]   # below the floor
    mom[..., 2][kind == 4] = 1e6                                       # clamps at maxSamples
    mom[..., 2][kind == 5] = np.nan                                    # a NaN variance
    # q exactly an integer k: m1 = 2^a, N = 2^b, tau = 2^-4 and var = k * N * tau^2 * m1^2 / base — every product and the
    # quotient are exact in fp32
    exact = kind == 6
    for p in [tuple(x) for x in np.argwhere(kind == 7)[:2]]:           # ... and q exactly maxSamples
        exact[p] = True
    tau2 = f(PARAMS["target_rel_error"]) * f(PARAMS["target_rel_error"])
    k = rng.integers(1, 17, (h, w)).astype(np.float32)
    k[kind == 7] = 16.0
    a = (2.0 ** rng.integers(-3, 2, (h, w))).astype(np.float32)
    b = (2.0 ** rng.integers(1, 6, (h, w))).astype(np.float32)
    mom[..., 0][exact], mom[..., 3][exact] = a[exact], b[exact]
    mom[..., 2][exact] = ((k * b * a * a / f(PARAMS["base_samples"])) * tau2)[exact]
    # nothing else may sit on a step: nudge such pixels off it, deterministically
    for _ in range(8):
        near = near_a_step(mom, PARAMS) & ~exact
        if not near.any():
            break
        mom[..., 2][near] *= f(1.01)
    assert not (near_a_step(mom, PARAMS) & ~exact).any()
    for v in range(8):
        assert (kind == v).any(), v
    return mom, exact


def build(r, mom, **p):
    counts = r.build_sample_map(mom, **p)
    return counts, r.sample_map_stats()


@pytest.mark.parametrize("w,h", [(37, 23), (70, 33)])
def test_build_sample_map_on_synthetic_moments(renderer, w, h):
    renderer.upload_scene(cornell_scene(True))
    d = _capi.RtSampleMapParams()
    _capi.lib().rt_sample_map_params_default(C.byref(d))
    assert (d.baseSamples, d.minSamples, d.maxSamples, d.targetRelError, d.luminanceFloor) == (4, 1, 16, np.float32(0.05), np.float32(0.01))
    mom, exact = synthetic_moments(w, h, 100 * w + h)
    want, stats, q = restated(mom, **PARAMS)
    # the deliberate cases are what they were built to be: exact in fp32, on the integer
    assert exact.sum() >= 10 and (q[exact] == np.rint(q[exact])).all() and (q[exact] >= 1).all() and (q[exact] == 16).any()
    assert (want[exact] == np.minimum(q[exact], 16).astype(np.uint32)).all()
    N, var = mom[..., 3], mom[..., 2]
    assert (want[N == 0] == 1).all() and (want[N == 1] == 4).all() and (want[np.isnan(var)] == 16).all() and (want[var == 1e6] == 16).all()
    assert (want[(var == 0) & (N >= 2)] == 1).all() and len(np.unique(want)) >= 12
    got, gstats = build(renderer, mom, **PARAMS)
    assert got.dtype == np.uint32 and got.shape == (h, w)
    d = got != want
    assert not d.any(), (int(d.sum()), np.argwhere(d)[:5].tolist(), got[d][:5], want[d][:5], q[d][:5])
    assert gstats == stats, (gstats, stats)
    # other parameters, the defaults among them (no argument at all), and min = base = max
    for p in (dict(), dict(base_samples=1, min_samples=0, max_samples=3, target_rel_error=0.2, luminance_floor=0.5),
              dict(base_samples=7, min_samples=7, max_samples=7), dict(base_samples=8, min_samples=2, max_samples=1000, target_rel_error=0.01)):
        full = dict(LIBRARY_DEFAULTS, **p)   # what the call leaves out is rt_sample_map_params_default's
        want, stats, _ = restated(mom, **full)
        got, gstats = build(renderer, mom, **p)
        assert np.array_equal(got, want) and gstats == stats, (p, int((got != want).sum()), gstats, stats)


def test_build_sample_map_on_rendered_moments_and_the_ctx_plane(renderer):
    """The moments of four accumulated frames of the Cornell box at 96 x 72, from the host plane and from the ctx's own; the map of
    the ctx's own plane renders."""
    r = renderer
    w, h = 96, 72
    r.upload_scene(cornell_scene(True))
    r.temporal_reset()
    for k in range(4):
        pc = engine.push_constants(w, h, raysPerPixel=2, progressive=0, frameCount=k)
        r.render(pc, w, h)
        r.render_aovs(pc, w, h)
        _, mom = r.temporal_accumulate(pc, moments=True)
    N = mom[..., 3]
    assert (N == 0).any() and (N == 4).any()
    want, stats, q = restated(mom, **PARAMS)
    print(f"rendered moments: counts {np.bincount(want.reshape(-1)).tolist()}, {stats}, near a step {int(near_a_step(mom, PARAMS).sum())}")
    assert len(np.unique(want)) >= 4 and 0 < stats["aboveMin"] < stats["pixels"]
    got, gstats = build(r, mom, **PARAMS)
    assert np.array_equal(got, want) and gstats == stats, (int((got != want).sum()), gstats, stats)
    own = r.build_sample_map(**PARAMS)                      # the ctx's own plane of the last temporal_accumulate
    assert np.array_equal(own, want) and r.sample_map_stats() == stats
    d_map = r.build_sample_map(to_host=False, **PARAMS)     # ... left on the device and rendered from there
    pc = engine.push_constants(w, h, raysPerPixel=16, progressive=0, frameCount=4)
    r.reset_counters()
    a = r.render_sampled(pc, w, h, d_map)
    assert r.counters()["paths"] == stats["samples"]
    assert np.array_equal(bits(a), bits(r.render_sampled(pc, w, h, want)))
    # the ctx plane must be this frame
    with pytest.raises(engine.RtError, match="not the whole 72 x 96 frame"):
        r.build_sample_map(width=72, height=96, **PARAMS)
    for bad, what in ((dict(min_samples=5), "minSamples must be <= baseSamples"), (dict(base_samples=17), "baseSamples must be <= maxSamples"),
                      (dict(target_rel_error=0.0), "targetRelError"), (dict(target_rel_error=float("nan")), "targetRelError"),
                      (dict(luminance_floor=-1.0), "luminanceFloor")):
        for m in (mom, None):
            with pytest.raises(engine.RtError, match=what):
                r.build_sample_map(m, **dict(PARAMS, **bad))
    assert r.sample_map_stats() == stats                    # a refused call leaves the last build's statistics


def test_no_ctx_moments_yet():
    r = engine.Renderer(0)
    try:
        r.upload_scene(cornell_scene(True))
        with pytest.raises(engine.RtError, match="no ctx-owned moments"):
            r.build_sample_map(width=8, height=8)
        with pytest.raises(engine.RtError, match="rt_build_sample_map was never called"):
            r.sample_map_stats()
    finally:
        r.close()


# ---------------------------------------------------------------- 8. session
def test_session_renders_with_the_map_of_the_previous_frame(tuned):
    r = tuned
    s = cornell_scene(True)
    w, h = 64, 48
    p = dict(base_samples=2, min_samples=1, max_samples=8, target_rel_error=0.05)
    ses = session.InteractiveSession(r, s, w, h, temporal=True, adaptive=True, adaptive_params=p)
    ses.params.raysPerPixel = 4
    previous = None
    varied = 0
    for k in range(6):
        ses.frame(keys="W", frame_time_ms=2.0)
        image, used, mom = ses.image.copy(), ses.sample_map, ses.moments.copy()
        if k == 0:
            assert used is None
            again = r.render(ses.pc, w, h)
        else:
            assert np.array_equal(used, r.build_sample_map(previous, **p)), k
            assert used.min() >= 1
            varied += len(np.unique(np.minimum(used, 4))) > 1
            again = r.render_sampled(ses.pc, w, h, used)
        assert np.array_equal(bits(image), bits(again)), k
        previous = mom
    assert varied >= 4
    ses.frame()   # the camera rests: progressive accumulation, no map
    assert ses.sample_map is None
    with pytest.raises(ValueError):
        session.InteractiveSession(r, s, w, h, adaptive=True)
    with pytest.raises(ValueError):
        session.InteractiveSession(r, s, w, h, temporal=True, adaptive=True, adaptive_params=dict(min_samples=0, base_samples=2))


def test_session_without_adaptive_is_unchanged(tuned):
    r = tuned
    s = cornell_scene(True)
    w, h = 64, 48
    ses = session.InteractiveSession(r, s, w, h, temporal=True)
    ses.params.raysPerPixel = 2
    for k in range(4):
        ses.frame(keys="W", frame_time_ms=2.0)
        image, filtered = ses.image.copy(), ses.filtered.copy()
        assert ses.sample_map is None
        assert np.array_equal(bits(image), bits(r.render(ses.pc, w, h))), k
        assert filtered.shape == (h, w, 4) and ses.history_length.max() == pytest.approx(k + 1.0, abs=1e-3)


# ---------------------------------------------------------------- does it pay?
def test_adaptive_against_uniform_at_equal_samples(renderer):
    """tools/sample_map_quality.py's comparison (eight frames of Cornell + spheres at 160 x 120 through the temporal pass, still
    camera, against 1024 spp): run A, frame 0 at 4 spp and then the map (1..16), never spends more than run B, eight uniform frames
    at the smallest count whose total reaches A's. The accounting only: as recorded (profiles/sample_map_quality.json), A is
    0.98 x B over the filtered set with 6 % fewer samples but 1.19 x B on the worst 8 x 8 tile, so it is not better where it should
    be and no ratio is held; the figures are printed."""
    spec = importlib.util.spec_from_file_location("sample_map_quality", os.path.join(ROOT, "tools", "sample_map_quality.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    q = tool.measure(renderer)
    print(q)
    assert q["A"]["samples"] <= q["B"]["samples"] and q["B"]["samples"] - q["A"]["samples"] < 8 * 160 * 120
    assert q["A"]["samples_per_frame"][0] == 4 * 160 * 120 and all(160 * 120 <= n <= 16 * 160 * 120 for n in q["A"]["samples_per_frame"][1:])
    assert np.isfinite([q["A"]["mse"], q["B"]["mse"], q["A"]["worst_tile_mse"], q["B"]["worst_tile_mse"]]).all()
