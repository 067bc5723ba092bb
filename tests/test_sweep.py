"""Sphere sweeps on the GPU (rt_query_sweep, rt_query_sweep_host; Renderer.query_sweep; DESIGN.md, "Sphere sweeps"): the first contact
of a ball moved along a ray.

The contract (include/rt_amd.h, include/rt_sweep.h): a primitive's contact time is a function of the ray, the radius and the
primitive alone, the key that picks the answer is total and the descent's pruning conservative, so the device (its own node
numbering, its pruned and ordered descent, the two instantiations of k_sweep_spheres) must give what the exhaustive host loop over
the host arrays gives (rt_sweep_exhaustive_host; engine.sweep_exhaustive) in every byte of every record, with and without limits.
The loop itself is held to a float64 reference on the CPU (tests/test_sweep_host.py). The scenes and ray sets are
tests/sweep_cases.py's."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import sweep_cases as sc
import sweep_float64 as sf
from util import _deformed_bunny, kernel_instantiations, to_device

REC = C.sizeof(_capi.RtSweep)
SHALLOW, DEEP = "k_sweep_spheres<24, true>", "k_sweep_spheres<64, false>"

_wants = {}


def raw(recs, n):
    return np.frombuffer(recs, dtype=np.uint8).reshape(n, REC).copy() if n else np.zeros((0, REC), np.uint8)


def is_not_found(rows):
    want = np.zeros(16, np.uint32)
    want[0] = np.float32(99999999.0).view(np.uint32)
    return (rows.view(np.uint32).reshape(-1, 16) == want).all(axis=1)


def fields(rows):
    f, u = rows.view(np.float32).reshape(-1, 16), rows.view(np.uint32).reshape(-1, 16)
    return dict(t=f[:, 0], found=u[:, 1] == 1, gap=f[:, 7])


def _want(name, key, limited):
    """The exhaustive loop's answer, once per session: (bytes [n, 64], the limits or None). The limits are 0.5, 1, 1.5 and 2 times
    the unlimited answer's own t in turn, so that half of them cut it, one of them exactly at t."""
    if (name, key, limited) not in _wants:
        c = sc.case(name)
        s = c["sets"][key]
        n = len(s["o"])
        T = None
        if limited:
            free = fields(_want(name, key, False)[0])
            T = np.where(free["found"], free["t"] * np.resize(np.array([0.5, 1.0, 1.5, 2.0], np.float32), n), np.float32(1.0)).astype(np.float32)
            T[~(T > 0)] = 1.0
        _wants[(name, key, limited)] = (raw(engine.sweep_exhaustive(c["scene"].arrays(), s["o"], s["d"], s["R"], T), n), T)
    return _wants[(name, key, limited)]


def _device(renderer, o, d, R, T=None, guard=0):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own: (bytes [n, 64], the kernel that
    ran, the `guard` bytes behind the records)."""
    n = len(o)
    renderer.sync()
    po, pd, pr = to_device(renderer, "s_o", o), to_device(renderer, "s_d", d), to_device(renderer, "s_r", R)
    pt = None if T is None else to_device(renderer, "s_t", T)
    out = np.full(n * REC + guard, 0xA5, np.uint8)
    pout = to_device(renderer, "s_out", out)
    assert renderer.query_sweep(po, pd, pr, pt, n=n, out=pout, sync=False) is None
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["s_out"].download(into=out)
    return out[:n * REC].reshape(n, REC), kernel, out[n * REC:]


def _assert_equal(got, want, what):
    assert np.array_equal(got, want), f"{what}: records differ at rays {np.unique(np.argwhere(got != want)[:, 0])[:8].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.SCENES)
def test_device_equals_the_exhaustive_loop(renderer, name):
    """All 64 bytes of all records, on every ray set, with and without limits, and through the _host form; the kernel by the
    scene's depth; and with a limit T the unlimited record when its t < T, else the not-found record, exactly."""
    c = sc.case(name)
    renderer.upload_scene(c["scene"])
    for key, s in c["sets"].items():
        n = len(s["o"])
        free = None
        for limited in (False, True):
            want, T = _want(name, key, limited)
            what = f"{name}/{key}/{'limits' if limited else 'no limit'}"
            got, kernel, _ = _device(renderer, s["o"], s["d"], s["R"], T)
            assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
            _assert_equal(got, want, what)
            _assert_equal(raw(renderer.query_sweep(s["o"], s["d"], s["R"], T), n), got, what + " / host form")
            if not limited:
                free = got
                continue
            f = fields(free)
            keep = f["found"] & (f["t"] < T)
            assert np.array_equal(got[keep], free[keep]) and is_not_found(got[~keep]).all(), f"{what}: a limit does more than cut"
            assert keep.any() and ((f["found"] & ~keep).any() or not (f["t"][f["found"]] > 0).any()), f"{what}: the limits do not try both sides"
        print(f"{name}/{key}: {int(fields(free)['found'].sum())} of {n} found, {int((fields(free)['t'] == 0).sum())} start in contact")


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_sweep_spheres") == {SHALLOW, DEEP}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n rays alone equal their rows of the whole set, and the 64 bytes behind the records
    are left as they were."""
    c = sc.case("cornell")
    renderer.upload_scene(c["scene"])
    s = c["sets"]["aimed"]
    for limited in (False, True):
        want, T = _want("cornell", "aimed", limited)
        got, kernel, behind = _device(renderer, s["o"][:n].copy(), s["d"][:n].copy(), s["R"][:n].copy(), None if T is None else T[:n].copy(), guard=64)
        assert kernel == SHALLOW
        _assert_equal(got, want[:n], f"n = {n}")
        assert (behind == 0xA5).all(), f"n = {n}: bytes behind the batch's output were written"
        _assert_equal(raw(renderer.query_sweep(s["o"][:n], s["d"][:n], s["R"][:n], None if T is None else T[:n]), n), got, f"n = {n} / host form")


@pytest.mark.gpu
def test_radii_limits_and_directions_that_mean_no_search(renderer):
    """Radii and limits of 0, -0, -1 and NaN, and a zero direction: the not-found record, and not counted in raysTraced."""
    c = sc.case("cornell")
    renderer.upload_scene(c["scene"])
    s = c["sets"]["contact"]
    n = 120
    o, d, R = s["o"][:n].copy(), s["d"][:n].copy(), s["R"][:n].copy()
    T = np.full(n, 5.0, np.float32)
    bad = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), n)
    kind = np.arange(n) % 4            # 0: sound, 1: a bad radius, 2: a bad limit, 3: no direction
    R[kind == 1] = bad[kind == 1]
    T[kind == 2] = bad[kind == 2]
    d[kind == 3] = 0.0
    renderer.sync()
    before = renderer.counters()
    got, _, _ = _device(renderer, o, d, R, T)
    after = renderer.counters()
    assert is_not_found(got[kind != 0]).all()
    f = fields(got[kind == 0])
    assert f["found"].all() and (f["t"] == 0).all()
    assert after["raysTraced"] - before["raysTraced"] == int((kind == 0).sum()) and after["raysHit"] - before["raysHit"] == int((kind == 0).sum())
    _assert_equal(got, raw(engine.sweep_exhaustive(c["scene"].arrays(), o, d, R, T), n), "degenerate arguments")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.SCENES)
def test_relation_to_the_nearest_and_the_closest_hit_queries(renderer, name):
    """rt_query_nearest over the contact centres fl(o + t d) returns dst <= gap as an fp32 compare, on every found ray: gap is the
    point queries' own distance of one primitive. rt_query_closest over the same rays: wherever it hits a surface, the sweep is
    found and t <= dst within the two float64 bounds of the ray: a ball of any radius touches what its centre's ray crosses no
    later than that, so t <= t64(R - delta) + tau <= dst64 + tau (tests/test_sweep_host.py holds the loop to the first), and the
    ray query's own dst lies within sweep_cases.ray_query_bound of dst64. The sweep's surface set contains the ray query's, but
    for the zeroed sphere slots its arithmetic can report from far away (ray_query_bound says which)."""
    c = sc.case(name)
    renderer.upload_scene(c["scene"])
    for key, s in c["sets"].items():
        n = len(s["o"])
        got, _, _ = _device(renderer, s["o"], s["d"], s["R"])
        f = fields(got)
        centres = (s["o"] + f["t"][:, None] * s["d"]).astype(np.float32)[f["found"]]
        near = engine.nearest_to_numpy(renderer.query_nearest(centres))
        assert near["found"].all() and (near["dst"] <= f["gap"][f["found"]]).all(), f"{name}/{key}: rt_query_nearest at a contact centre is farther than gap"
        hit = engine.hits_to_numpy(renderer.query_closest(s["o"], s["d"]))
        bound, surface = sc.ray_query_bound(c["ns"], s, hit)
        crossed = (hit["didHit"] == 1) & surface
        tol = sf.tau(c["ns"], s["d"], s["R"], hit["dst"]) + bound
        assert f["found"][crossed].all(), f"{name}/{key}: a ray hits where its sweep finds nothing"
        assert (f["t"][crossed] <= hit["dst"][crossed] + tol[crossed]).all(), f"{name}/{key}: a sweep touches later than its centre's ray hits"
        print(f"{name}/{key}: {int(crossed.sum())} of {n} rays hit, {int(f['found'].sum())} sweeps found")


@pytest.mark.gpu
def test_counters_and_what_a_sweep_leaves_alone(renderer):
    """raysTraced and raysHit equal the loop's counts; boxTests and triTests move; nothing else does, and the nearest query after it
    is what it was."""
    c = sc.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    s = c["sets"]["grazing"]
    want, _ = _want("cornell_bunny", "grazing", False)
    renderer.reset_counters()
    zero = renderer.counters()
    cost = renderer.ray_cost()
    state = (renderer.last_pipeline(), renderer.last_parts())
    got, _, _ = _device(renderer, s["o"], s["d"], s["R"])
    _assert_equal(got, want, "cornell_bunny/grazing")
    after = renderer.counters()
    assert after["raysTraced"] - zero["raysTraced"] == len(s["o"])
    assert after["raysHit"] - zero["raysHit"] == int(fields(want)["found"].sum())
    assert after["boxTests"] > zero["boxTests"] and after["triTests"] > zero["triTests"]
    for key in after:
        if key not in ("boxTests", "triTests", "raysTraced", "raysHit"):
            assert after[key] == zero[key], key
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    points = s["o"]
    want_near = engine.nearest_to_numpy(engine.nearest_exhaustive(c["scene"].arrays(), points))
    near = engine.nearest_to_numpy(renderer.query_nearest(points))
    assert np.array_equal(near["dst"].view(np.uint32), want_near["dst"].view(np.uint32)) and np.array_equal(near["found"], want_near["found"])


@pytest.mark.gpu
def test_after_update_objects_the_answers_follow_the_moved_object(renderer):
    """The reference is the exhaustive loop over the host arrays before and after the move: its own answers change, and the device
    equals it each time, so the device read the moved tables."""
    e = sc.pq.build_scene("instances")
    renderer.upload_scene(e)
    s = sc.case("instances")["sets"]["aimed"]
    n = len(s["o"])
    before, _, _ = _device(renderer, s["o"], s["d"], s["R"])
    want_before = raw(engine.sweep_exhaustive(e.arrays(), s["o"], s["d"], s["R"]), n)
    _assert_equal(before, want_before, "instances before the move")
    e.set_transform(1, engine.placement(position=(0.2, -0.4, 0.5), rotation=(15, -40, 70), scale=(0.8, 1.3, 0.5)))
    e.push(renderer, "objects")
    after, kernel, _ = _device(renderer, s["o"], s["d"], s["R"])
    assert kernel == SHALLOW
    want_after = raw(engine.sweep_exhaustive(e.arrays(), s["o"], s["d"], s["R"]), n)
    moved = int((want_after != want_before).any(axis=1).sum())
    print(f"the move changes the reference's record on {moved} of {n} rays")
    assert moved, "the move does not change the reference: the test shows nothing"
    _assert_equal(after, want_after, "instances after the move")


@pytest.mark.gpu
def test_after_update_points_the_answers_follow_the_deformed_mesh(renderer):
    scene, p, first = _deformed_bunny()
    renderer.upload_scene(scene, dynamic=True)
    s = sc.case("cornell_bunny")["sets"]["aimed"]
    n = len(s["o"])
    want_before = raw(engine.sweep_exhaustive(scene.arrays(), s["o"], s["d"], s["R"]), n)
    _assert_equal(_device(renderer, s["o"], s["d"], s["R"])[0], want_before, "the dynamic upload")
    renderer.update_points(p, first)
    scene.update_points(p, first)
    want_after = raw(engine.sweep_exhaustive(scene.arrays(), s["o"], s["d"], s["R"]), n)
    moved = int((want_after != want_before).any(axis=1).sum())
    print(f"the deformation changes the reference's record on {moved} of {n} rays")
    assert moved, "the deformation does not change the reference: the test shows nothing"
    _assert_equal(_device(renderer, s["o"], s["d"], s["R"])[0], want_after, "after rt_update_points")


@pytest.mark.gpu
def test_empty_batch_and_refusals_through_the_c_abi(renderer):
    c = sc.case("cornell")
    renderer.upload_scene(c["scene"])
    z3, z1 = np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    assert len(renderer.query_sweep(z3, z3, z1)) == 0
    l, h = renderer._l, renderer._h
    s = c["sets"]["aimed"]
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    pout = to_device(renderer, "s_out", guard)
    po, pd, pr = to_device(renderer, "s_o", s["o"][:16]), to_device(renderer, "s_d", s["d"][:16]), to_device(renderer, "s_r", s["R"][:16])
    empty = _capi.RtSweepBatch(None, None, None, None, 0)
    assert l.rt_query_sweep(h, C.byref(empty), None) == 0 and l.rt_query_sweep_host(h, C.byref(empty), None) == 0
    for fn in ("rt_query_sweep", "rt_query_sweep_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host = (_capi.RtSweep * 16)()
        out = C.addressof(out_host) if host else pout
        a, b, r = (s["o"][:16].ctypes.data, s["d"][:16].ctypes.data, s["R"][:16].ctypes.data) if host else (po, pd, pr)
        required = "origins, dirs, radius and the output are required"
        for batch, o, message in ((None, out, "the batch is NULL"),
                                  (_capi.RtSweepBatch(None, b, r, None, 5), out, required),
                                  (_capi.RtSweepBatch(a, None, r, None, 5), out, required),
                                  (_capi.RtSweepBatch(a, b, None, None, 5), out, required),
                                  (_capi.RtSweepBatch(a, b, r, None, 5), None, required),
                                  (_capi.RtSweepBatch(a, b, r, None, 1 << 30), out, "a batch of 1073741824 rays does not fit the 30 bits of a slot id"),
                                  (_capi.RtSweepBatch(a, b, None, None, 1 << 30), out, required)):      # the order
            assert call(h, C.byref(batch) if batch is not None else None, o) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {message}", l.rt_last_error(h).decode()
        assert not np.frombuffer(out_host, np.uint8).any()
    renderer.sync()
    renderer._owned["s_out"].download(into=guard)
    assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        batch = _capi.RtSweepBatch(po, pd, pr, None, 16)
        assert fresh._l.rt_query_sweep(fresh._h, C.byref(batch), pout) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_sweep before rt_upload_scene"
        assert fresh._l.rt_query_sweep_host(fresh._h, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_sweep_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_sweep(s["o"], s["d"], s["R"][:5])
    with pytest.raises(ValueError):
        renderer.query_sweep(1 << 20, 1 << 21, 1 << 22, n=4)      # device pointers without out=
