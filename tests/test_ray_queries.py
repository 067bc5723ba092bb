"""Ray queries on batches of the caller's own rays (rt_query_closest, rt_query_occluded and their _host forms; Renderer.query_closest /
query_occluded) and the ambient-occlusion plane built on them (rt_render_ao; Renderer.render_ao, engine.ao_rays).

The contract (include/rt_amd.h, DESIGN.md "Ray queries"): ray i with limit T runs calculateIntersections with its running closest
distance started at T. So the closest-hit query returns the oracle's record where its dst < T and the miss record elsewhere (bit for
bit; boxTests and triTests are 0), and the occlusion query says 1 exactly when that search accepts any primitive, which does not depend
on the visiting order: occluded => didHit && dst < T on every ray, and the converse everywhere but within the box tests' rounding below
T. The cases: every scene of test_closest_hit_float64 with its rays, the two golden ray sets, and the alpha-mapped scene of
test_texture_maps_float64 (k_trace_pw_alpha). The limit sets: none, all RT_MISS_DST, f * dst with f cycling through 0.5, 0.999, 1.001, 2
on the oracle's hits (a random factor in (0.1, 4) on its misses), and the same with a few of 0, -1 and NaN among them.

The CPU half asserts the conditions on the ray sets with the oracle and brute_force alone."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import _capi, engine

import brute_force as bf
import closest_hit_cases as chf
import texture_map_cases as tmf
from util import assert_hits_equal, cornell_scene, model_scene, to_device

MISS_DST = np.float32(99999999.0)   # RT_MISS_DST
FACTORS = np.array([0.5, 0.999, 1.001, 2.0], np.float32)
FRAGILE_WORLD = 0.05      # world units: box_intersect's error is a few ulps of coordinates of magnitude <= 4, about 1e-6; a 1e-3
                          # relative gap of a hit at least this far is at least 50 times that
MAX_EXCLUDED = 0.02
MIN_EACH = 100
GOLDEN = ("cornell", "bunny908")
CASES = list(chf.SCENES) + [f"golden_{g}" for g in GOLDEN] + ["alpha"]
HIT_FIELDS = ("dst", "didHit", "isSphere", "objectHitIndex", "triHitIndex", "materialIndex", "frontFace", "hitPoint", "normal")
NEAR_KEEP = {"surface": 16}   # (its rays start 1e-3 off a surface: an eighth of its hits are that near)

_cases = {}


def _case(name, renderer=None):
    """dict(scene: what upload_scene takes; textures; o, d; oracle: the oracle's records; ref: brute_force's answer; dropped),
    once per session."""
    key = (name, renderer is not None and name == "blob70k")
    if key in _cases:
        return _cases[key]
    textures, dropped = [], 0
    if name in chf.SCENES:
        s, bs, o, d, _, ref, dropped = chf._case(name, renderer if name == "blob70k" else None)   # (only its BVH depends on the device)
        up = s
    elif name.startswith("golden_"):
        g = name[len("golden_"):]
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"hits_{g}_1024.npz"), allow_pickle=False)
        s = up = cornell_scene(True) if g == "cornell" else model_scene("bunny.obj")
        o, d = z["origins"], z["dirs"]
        ref = bf.BruteScene.from_numpy(s.numpy()).closest_hit(o, d)
    else:
        s, up, bs, o, d, ref, dropped = tmf._case("alpha", "aimed")
        textures = bs.textures
    try:
        pyoracle.set_textures(textures)
        oracle = engine.hits_to_numpy(pyoracle.trace_rays(up, o, d))
    finally:
        pyoracle.set_textures([])
    if name.startswith("golden_"):
        assert_hits_equal({k: oracle[k] for k in HIT_FIELDS}, {k: z[k] for k in HIT_FIELDS})
    # The source sets hold more hits within FRAGILE_WORLD of the origin than the conditions on a case's rays allow (test_ray_set_conditions:
    # half of them get f = 0.999 or 1.001 and are fragile, and their dst bound is often above 1e-3 of their dst, which takes them out of
    # (4) as well). The cure is in the rays, not in the cap: of those rays a case keeps every NEAR_KEEP-th in ray order, chosen by the
    # oracle's own dst before any code under test has seen them.
    world = oracle["dst"].astype(np.float64) * np.linalg.norm(np.asarray(d, np.float64), axis=1)
    near = oracle["didHit"].astype(bool) & (world < FRAGILE_WORLD)
    keep = ~near
    keep[np.flatnonzero(near)[::NEAR_KEEP.get(name, 4)]] = True
    o, d, oracle, ref = o[keep], d[keep], {k: v[keep] for k, v in oracle.items()}, tmf._rows(ref, keep)
    _cases[key] = dict(scene=up, textures=textures, o=np.ascontiguousarray(o, np.float32), d=np.ascontiguousarray(d, np.float32),
                       oracle=oracle, ref=ref, dropped=dropped)
    return _cases[key]


def _limits(name, oracle):
    """The limit sets of a case, from the oracle's dst alone: name -> ((n,) float32 or None, the factor index per ray or -1)."""
    n = len(oracle["dst"])
    hit = oracle["didHit"].astype(bool)
    rng = np.random.default_rng(900 + CASES.index(name))
    fi = np.full(n, -1)
    fi[hit] = np.arange(int(hit.sum())) % len(FACTORS)
    scaled = rng.uniform(0.1, 4.0, n).astype(np.float32)
    scaled[hit] = FACTORS[fi[hit]] * oracle["dst"][hit]
    bad = scaled.copy()
    bad[3::41] = np.resize(np.array([0.0, -1.0, np.nan, -0.0], np.float32), len(bad[3::41]))
    return dict(none=(None, np.full(n, -1)), miss=(np.full(n, MISS_DST, np.float32), np.full(n, -1)), scaled=(scaled, fi), bad=(bad, fi))


def _within(oracle, T):
    """didHit && dst < T, in float32 as the kernels compare (a NaN or non-positive limit admits nothing)."""
    if T is None:
        return oracle["didHit"].astype(bool)
    with np.errstate(invalid="ignore"):
        return oracle["didHit"].astype(bool) & (oracle["dst"] < T) & (T > 0)


def _fragile(c, T, fi):
    """Assertion (3)'s exceptions: f in {0.999, 1.001} and the hit nearer than FRAGILE_WORLD."""
    world = c["oracle"]["dst"].astype(np.float64) * np.linalg.norm(c["d"].astype(np.float64), axis=1)
    return ((fi == 1) | (fi == 2)) & c["oracle"]["didHit"].astype(bool) & (world < FRAGILE_WORLD)


def _brute_usable(c, T):
    """Assertion (4)'s rays: not ill, and |dst - T| above the ray's dst bound where the reference hits."""
    ref = c["ref"]
    t64 = np.full(len(ref["ill"]), float(MISS_DST)) if T is None else T.astype(np.float64)
    with np.errstate(invalid="ignore"):
        near = ref["didHit"] & ~(np.abs(ref["dst"] - t64) > ref["dst_bound"])
        expect = ref["didHit"] & (ref["dst"] < t64) & (t64 > 0)
    return ~ref["ill"] & ~near, expect


def _expected_closest(oracle, T):
    """The oracle's record where dst < T, the miss record elsewhere."""
    keep = _within(oracle, T)
    out = {}
    for k in HIT_FIELDS:
        v = oracle[k].copy()
        v[~keep] = MISS_DST if k == "dst" else 0
        out[k] = v
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU half
@pytest.mark.parametrize("name", CASES)
def test_ray_set_conditions(name):
    """Conditions on the ray sets, asserted without the code under test: the fragile set of (3) plus the exclusions of (4) are at most
    2 % of a case's rays, and under the f * dst limits at least 100 rays are occluded and at least 100 are not."""
    c = _case(name)
    n = len(c["o"]) + c["dropped"]
    T, fi = _limits(name, c["oracle"])["scaled"]
    usable, _ = _brute_usable(c, T)
    excluded = _fragile(c, T, fi) | ~usable
    occluded = _within(c["oracle"], T)
    print(f"[{name}] rays {n}  fragile {int(_fragile(c, T, fi).sum())}  excluded from (4) {int((~usable).sum())}  dropped {c['dropped']}  "
          f"together {(int(excluded.sum()) + c['dropped']) / n:.4%}  occluded {int(occluded.sum())}  unoccluded {int((~occluded).sum())}")
    assert (int(excluded.sum()) + c["dropped"]) / n <= MAX_EXCLUDED, name
    assert occluded.sum() >= MIN_EACH and (~occluded).sum() >= MIN_EACH, name
    bad = _limits(name, c["oracle"])["bad"][0]
    assert np.isnan(bad).any() and (bad == 0).any() and (bad == -1).any()
    # the oracle and the float64 reference agree on what is occluded wherever (4) looks
    for T, _ in _limits(name, c["oracle"]).values():
        usable, expect = _brute_usable(c, T)
        assert np.array_equal(_within(c["oracle"], T)[usable], expect[usable]), name


def test_ray_batch_layout_matches_the_header():
    assert [n for n, _ in _capi.RtRayBatch._fields_] == ["origins", "dirs", "tmax", "n"]
    assert C.sizeof(_capi.RtRayBatch) == 3 * C.sizeof(C.c_void_p) + 8 and _capi.RtRayBatch.n.offset == 3 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _capi.RtAoParams._fields_] == ["samples", "radius", "seed"] and C.sizeof(_capi.RtAoParams) == 12


# ---------------------------------------------------------------------------------------------------------------- GPU half
def _device_queries(renderer, o, d, T):
    """Both queries through the device entry points: the rays start as numpy arrays and get there through device buffers."""
    n = len(o)
    renderer.sync()
    po, pd = to_device(renderer, "q_origins", o), to_device(renderer, "q_dirs", d)
    pt = None if T is None else to_device(renderer, "q_tmax", T)
    ph = renderer._device_buffer("q_hits", n * C.sizeof(_capi.RtHit))
    pb = renderer._device_buffer("q_occluded", n)
    renderer.query_closest(po, pd, pt, n=n, out=ph, sync=False)
    kernel = renderer.last_kernel()
    renderer.query_occluded(po, pd, pt, n=n, out=pb, sync=False)
    assert renderer.last_kernel() == kernel
    renderer.sync()
    hits = (_capi.RtHit * n)()
    renderer._owned["q_hits"].download(into=np.frombuffer(hits, np.uint8))
    occ = renderer._owned["q_occluded"].download(n, np.uint8)
    assert set(np.unique(occ)) <= {0, 1}
    return engine.hits_to_numpy(hits), occ.astype(bool), kernel


def _check_case(renderer, name, c, what, host=False, brute=False):
    """Assertions (1) to (3), and with `brute` (4), for every limit set under the knobs as they are."""
    o, d, oracle = c["o"], c["d"], c["oracle"]
    for lname, (T, fi) in _limits(name, oracle).items():
        tag = f"{name} / {what} / limits {lname}"
        got, occ, kernel = _device_queries(renderer, o, d, T)
        assert kernel.startswith("k_trace_pw"), (tag, kernel)
        assert ("alpha" in kernel) == (name == "alpha"), (tag, kernel)
        # (1) the oracle's record where dst < T, the miss record elsewhere; no per-ray counters
        want = _expected_closest(oracle, T)
        assert_hits_equal({k: got[k] for k in HIT_FIELDS}, want)
        assert not got["boxTests"].any() and not got["triTests"].any(), tag
        if host:
            hh = engine.hits_to_numpy(renderer.query_closest(o, d, T))
            assert_hits_equal(hh, got)
            assert np.array_equal(renderer.query_occluded(o, d, T), occ), tag
        # (2) occluded => didHit && dst < T, on every ray
        within = _within(oracle, T)
        wrong = np.flatnonzero(occ & ~within)
        assert len(wrong) == 0, f"{tag}: occluded without a hit below the limit at {wrong[:5].tolist()}"
        # (3) the converse outside the fragile set
        lost = np.flatnonzero(within & ~occ & ~_fragile(c, T, fi))
        assert len(lost) == 0, f"{tag}: a hit below the limit not reported at {lost[:5].tolist()}"
        if brute:   # (4) against the float64 reference
            usable, expect = _brute_usable(c, T)
            off = np.flatnonzero(usable & (occ != expect))
            assert len(off) == 0, f"{tag}: differs from the float64 reference at {off[:5].tolist()}"
        print(f"[{tag}] {kernel}: {int(occ.sum())} of {len(occ)} occluded, fragile {int(_fragile(c, T, fi).sum())}, "
              f"of them unreported {int((within & ~occ).sum())}")


def _upload(renderer, c):
    renderer.upload_scene(c["scene"])
    renderer.upload_textures(c["textures"])


def _run_case(renderer, name, tree_mins=(48,)):
    c = _case(name, renderer)
    try:
        _upload(renderer, c)
        # with no limit: rt_trace_rays' own records
        traced = engine.hits_to_numpy(renderer.trace_rays(c["o"], c["d"]))
        assert_hits_equal({k: traced[k] for k in HIT_FIELDS}, {k: c["oracle"][k] for k in HIT_FIELDS})
        for tree_min in tree_mins:
            renderer.set_tuning("object_tree_min", tree_min)
            _check_case(renderer, name, c, f"defaults tree_min={tree_min}", host=True, brute=True)
            for knobs in chf.KNOBS:   # (5)
                for k, v in knobs.items():
                    renderer.set_tuning(k, v)
                _check_case(renderer, name, c, f"tree_min={tree_min} {knobs}")
            for k, v in chf.DEFAULTS.items():
                renderer.set_tuning(k, v)
            renderer.set_tuning("lanes_min_kslots", 1)
            _check_case(renderer, name, c, f"tree_min={tree_min} lanes_min_kslots=1")
            renderer.set_tuning("lanes_min_kslots", 1024)
    finally:
        for k, v in dict(chf.DEFAULTS, lanes_min_kslots=1024).items():
            renderer.set_tuning(k, v)
        renderer.upload_textures([])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "instances"])
def test_queries_against_the_oracle(renderer, name):
    _run_case(renderer, name)


@pytest.mark.gpu
def test_queries_over_many_placed_objects(renderer):
    """The object hierarchy (off, from 2 objects on, default) and the object-mask window: the skipping code under a caller's bound."""
    _run_case(renderer, "instances", tree_mins=(0, 2, 48))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_batch_sizes(renderer, n):
    c = _case("cornell")
    sub = dict(c, o=c["o"][:n].copy(), d=c["d"][:n].copy(), oracle={k: v[:n] for k, v in c["oracle"].items()},
               ref={k: v[:n] for k, v in c["ref"].items() if isinstance(v, np.ndarray)})
    _upload(renderer, c)
    o, d, oracle = sub["o"], sub["d"], sub["oracle"]
    for lname, (T, fi) in _limits("cornell", c["oracle"]).items():
        T = None if T is None else T[:n].copy()
        got, occ, _ = _device_queries(renderer, o, d, T)
        assert_hits_equal({k: got[k] for k in HIT_FIELDS}, _expected_closest(oracle, T))
        assert_hits_equal(engine.hits_to_numpy(renderer.query_closest(o, d, T)), got)
        assert np.array_equal(renderer.query_occluded(o, d, T), occ)
        within = _within(oracle, T)
        assert not (occ & ~within).any() and not (within & ~occ & ~_fragile(sub, T, fi[:n])).any(), (n, lname)
    # nothing past the batch is written
    guard = np.full(n + 64, 7, np.uint8)
    renderer.sync()
    pb = to_device(renderer, "q_guard", guard)
    renderer.query_occluded(to_device(renderer, "q_origins", o), to_device(renderer, "q_dirs", d), None, n=n, out=pb)
    renderer._owned["q_guard"].download(into=guard)
    assert np.array_equal(guard[:n].astype(bool), oracle["didHit"].astype(bool)) and np.all(guard[n:] == 7)


@pytest.mark.gpu
def test_empty_batch_and_refusals(renderer):
    c = _case("golden_cornell")
    _upload(renderer, c)
    e = np.zeros((0, 3), np.float32)
    assert len(renderer.query_closest(e, e)) == 0 and len(renderer.query_occluded(e, e)) == 0
    b = _capi.RtRayBatch(None, None, None, 5)
    for fn in ("rt_query_closest", "rt_query_occluded", "rt_query_closest_host", "rt_query_occluded_host"):
        assert getattr(renderer._l, fn)(renderer._h, C.byref(b), None) != 0
        assert renderer._l.rt_last_error(renderer._h).decode() == f"{fn}: origins, dirs and the output are required"
        assert getattr(renderer._l, fn)(renderer._h, None, None) != 0
        assert renderer._l.rt_last_error(renderer._h).decode() == f"{fn}: the batch is NULL"
    with pytest.raises(ValueError):
        renderer.query_closest(c["o"], c["d"][:5])
    with pytest.raises(ValueError):
        renderer.query_occluded(1 << 20, 1 << 21, n=4)   # device pointers without out=


@pytest.mark.gpu
def test_a_query_pass_leaves_rendering_alone(renderer):
    """After a query pass, rt_render of the golden Cornell frame is bit-identical to one rendered before it: the framebuffer,
    last_pipeline, last_parts; ray_cost is unchanged."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_c1_64x64_4spp.npz"), allow_pickle=False)
    c = _case("golden_cornell")
    _upload(renderer, c)
    pc = engine.push_constants(64, 64, singleRender=1, sampleLimit=4)
    before = renderer.render(pc, 64, 64)
    assert np.array_equal(before.view(np.uint32), z["rgba"].view(np.uint32))
    state = (renderer.last_pipeline(), renderer.last_parts())
    renderer.sync()
    cost = renderer.ray_cost()
    T = _limits("golden_cornell", c["oracle"])["scaled"][0]
    renderer.query_closest(c["o"], c["d"], T)
    renderer.query_occluded(c["o"], c["d"], T)
    assert renderer.last_kernel().startswith("k_trace_pw")
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state


# ---------------------------------------------------------------------------------------------------------------- AO
AO_W, AO_H = 64, 48


@pytest.mark.gpu
def test_ambient_occlusion_plane(renderer):
    renderer.upload_scene(cornell_scene(True))
    pc = engine.push_constants(AO_W, AO_H)
    a = renderer.render_aovs(pc, AO_W, AO_H)
    hit = a["hit"].reshape(-1)
    assert hit.sum() >= 1000 and (~hit).any()
    ao = renderer.render_ao(samples=4, radius=0.3, seed=1)
    assert ao.shape == (AO_H, AO_W) and ao.dtype == np.float32
    # the mean over the host's rays pushed through query_occluded, bit for bit
    k = np.zeros(AO_W * AO_H, np.uint32)
    for s in range(4):
        o, d, valid = engine.ao_rays(a, s, samples=4, radius=0.3, seed=1)
        assert np.array_equal(valid, hit)
        occ = renderer.query_occluded(o[valid], d[valid], np.full(int(valid.sum()), 0.3, np.float32))
        k[valid] += occ
    want = np.where(hit, (np.float32(4) - k.astype(np.float32)) / np.float32(4), np.float32(1)).astype(np.float32)
    assert np.array_equal(ao.reshape(-1).view(np.uint32), want.view(np.uint32))
    assert np.all(ao.reshape(-1)[~hit] == 1.0)
    assert 0 < k.sum() < 4 * hit.sum()
    # planes handed over equal the context's own
    assert np.array_equal(renderer.render_ao(a, samples=4, radius=0.3, seed=1), ao)
    # the same rays with a smaller bound
    small = renderer.render_ao(samples=4, radius=0.15, seed=1)
    assert np.all(small >= ao) and (small > ao).any()
    one, two = renderer.render_ao(samples=1, radius=0.3, seed=1), renderer.render_ao(samples=1, radius=0.3, seed=2)
    assert set(np.unique(one)) <= {0.0, 1.0} and (one != two).any()
    with pytest.raises(engine.RtError, match="samples must be 1..64"):
        renderer.render_ao(samples=65, radius=0.3)
