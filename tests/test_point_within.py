"""Radius point queries on the GPU (rt_query_within, rt_query_within_host; Renderer.query_within; DESIGN.md, "Radius point
queries"): every surface within reach of a point, the first k nearest first, and the count.

The contract (include/rt_amd.h, include/rt_point_within.h): the member set of a point is defined with a bound that never shrinks
and the key that orders it is total, so the device (its own node numbering, its pruned descent, the two instantiations of
k_points_within) must give what the exhaustive host loop over the host arrays gives (rt_within_exhaustive_host;
engine.within_exhaustive), bit for bit: every byte of every record and every count, for every k, with and without reaches. The
loop itself is held to a float64 reference on the CPU (tests/test_point_within_host.py). The scenes and point sets are
tests/point_query_cases.py's; the reaches come from the radius rule of tests/within_float64.py at m = 2 and m = 9."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import point_query_cases as pq
import within_float64 as wf
from util import kernel_instantiations, to_device

KS = (0, 1, 2, 8)
TARGETS = (2, 9)
REC = C.sizeof(_capi.RtNearest)
SHALLOW, DEEP = "k_points_within<24, false>", "k_points_within<64, true>"

_wants = {}


def _reach(name, key, m):
    return wf.Reach(wf.case_distances(name, key), m).R


def _want(name, key, m, k):
    """The exhaustive loop's answer, once per session: (bytes [n, k, 48], counts, R)."""
    if (name, key, m, k) not in _wants:
        c = pq.case(name)
        R = None if m is None else _reach(name, key, m)
        recs, counts = engine.within_exhaustive(c["scene"].arrays(), c["sets"][key], R, k)
        _wants[(name, key, m, k)] = (wf.raw(recs, len(counts), k).copy(), counts, R)
    return _wants[(name, key, m, k)]


def _device(renderer, points, R, k, guard=0):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own: (bytes [n, k, 48], counts, the
    kernel that ran, the `guard` bytes behind the records, the `guard` bytes behind the counts)."""
    n = len(points)
    renderer.sync()
    pp = to_device(renderer, "w_points", points)
    pr = None if R is None else to_device(renderer, "w_reach", R)
    out = np.full(n * k * REC + guard, 0xA5, np.uint8)
    cnt = np.full(n * 4 + guard, 0xA5, np.uint8)
    po, pc = to_device(renderer, "w_out", out), to_device(renderer, "w_counts", cnt)
    assert renderer.query_within(pp, pr, k, n=n, out=po if k else None, counts=pc, sync=False) is None
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["w_out"].download(into=out)
    renderer._owned["w_counts"].download(into=cnt)
    return out[:n * k * REC].reshape(n, k, REC), cnt[:n * 4].view(np.uint32).copy(), kernel, out[n * k * REC:], cnt[n * 4:]


def _assert_equal(got, want, what):
    (gb, gc), (wb, wc) = got, want
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.flatnonzero(gc != wc)[:5].tolist()}"
    assert np.array_equal(gb, wb), f"{what}: records differ at points {np.unique(np.argwhere(gb != wb)[:, 0])[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_device_equals_the_exhaustive_loop(renderer, name):
    """All bytes of all records and all counts, on every point set, k in {0, 1, 2, 8}, reaches at m in {2, 9}; and the _host form."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    most = 0
    for key, points in c["sets"].items():
        n = len(points)
        for m in TARGETS:
            for k in KS:
                wb, wc, R = _want(name, key, m, k)
                what = f"{name}/{key}/m={m}/k={k}"
                gb, gc, kernel, _, _ = _device(renderer, points, R, k)
                assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
                _assert_equal((gb, gc), (wb, wc), what)
                hr, hc = renderer.query_within(points, R, k)
                _assert_equal((wf.raw(hr, n, k), hc), (gb, gc), what + " / host form")
                most = max(most, int(wc.max()))
    surfaces = len(c["ns"].sph_c) + len(c["ns"].W)
    assert most > 8 or surfaces <= 8, f"{name}: no point has more members than slots"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spheres", "deep"])
def test_without_a_reach_every_surface_is_a_member(renderer, name):
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    for key, points in c["sets"].items():
        wb, wc, _ = _want(name, key, None, 8)
        gb, gc, _, _, _ = _device(renderer, points, None, 8)
        _assert_equal((gb, gc), (wb, wc), f"{name}/{key}/no reach")
        assert (gc == len(c["ns"].sph_c) + len(c["ns"].W)).all()


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_points_within") == {SHALLOW, DEEP}
    assert kernel_instantiations("k_points_within_resolve") == {"k_points_within_resolve<256>"}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n points alone equal their rows of the whole set, and the 64 bytes behind the
    records and behind the counts are left as they were."""
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    points = c["sets"]["uniform"][:n].copy()
    for k in (1, 8):
        wb, wc, R = _want("cornell", "uniform", 9, k)
        gb, gc, kernel, g_out, g_cnt = _device(renderer, points, R[:n].copy(), k, guard=64)
        assert kernel == SHALLOW
        _assert_equal((gb, gc), (wb[:n], wc[:n]), f"n = {n}, k = {k}")
        assert (g_out == 0xA5).all() and (g_cnt == 0xA5).all(), f"n = {n}, k = {k}: bytes behind the batch's outputs were written"
        hr, hc = renderer.query_within(points, R[:n], k)
        _assert_equal((wf.raw(hr, n, k), hc), (gb, gc), f"n = {n}, k = {k} / host form")


@pytest.mark.gpu
def test_reaches_that_admit_nothing_are_not_searched(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    points = c["sets"]["uniform"][:200]
    R = _reach("cornell", "uniform", 2)[:200].copy()
    bad = np.arange(200) % 5 == 3
    R[bad] = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), int(bad.sum()))
    for k in (0, 8):
        renderer.sync()
        before = renderer.counters()
        gb, gc, _, _, _ = _device(renderer, points, R, k)
        after = renderer.counters()
        assert not gc[bad].any() and wf.is_not_found(gb[bad]).all()
        assert (gc[~bad] >= 2).all()
        assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
        assert after["raysHit"] - before["raysHit"] == int((~bad).sum())
        recs, counts = engine.within_exhaustive(c["scene"].arrays(), points, R, k)
        _assert_equal((gb, gc), (wf.raw(recs, 200, k), counts), f"degenerate reaches, k = {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_relation_to_the_nearest_query(renderer, name):
    """On the device, under the same limits: count > 0 iff rt_query_nearest finds; out[i k].dst has its dst's bits; its primitive
    is listed wherever count <= k, with its record byte for byte; counts do not depend on k; a smaller k is the head of the list."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    for key in ("uniform", "vertices"):
        points = c["sets"][key]
        n = len(points)
        for m in TARGETS:
            R = _reach(name, key, m)
            renderer.sync()
            po = renderer._device_buffer("w_nearest", n * REC)
            renderer.query_nearest(to_device(renderer, "w_points", points), to_device(renderer, "w_reach", R), n=n, out=po)
            nearest = renderer._owned["w_nearest"].download((n, REC), np.uint8)
            eight, counts, _, _, _ = _device(renderer, points, R, 8)
            wf.check_relations(nearest, eight, counts, 8, f"{name}/{key}/m={m}")
            for k in (1, 2):
                gb, gc, _, _, _ = _device(renderer, points, R, k)
                assert np.array_equal(gc, counts) and np.array_equal(gb, eight[:, :k]), (name, key, m, k)
                wf.check_relations(nearest, gb, gc, k, f"{name}/{key}/m={m}/k={k}")
            none, gc, _, _, _ = _device(renderer, points, R, 0)
            assert np.array_equal(gc, counts) and none.size == 0
        # R1 <= R2: the list at R1 is the head of the list at R2
        small, c1, _, _, _ = _device(renderer, points, _reach(name, key, 2), 8)
        large, c2, _, _, _ = _device(renderer, points, _reach(name, key, 9), 8)
        head = np.arange(8)[None, :] < np.minimum(c1, 8)[:, None]
        assert (c1 <= c2).all() and np.array_equal(small[head], large[head]) and wf.is_not_found(small[~head]).all(), (name, key)


@pytest.mark.gpu
def test_a_radius_query_leaves_rendering_alone(renderer):
    """After a pass, rt_render of the golden Cornell frame is bit-identical to one rendered before it; last_pipeline, last_parts
    and the ray cost are unchanged; only the four counters the pass declares have moved."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_c1_64x64_4spp.npz"), allow_pickle=False)
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    pc = engine.push_constants(64, 64, singleRender=1, sampleLimit=4)
    before = renderer.render(pc, 64, 64)
    assert np.array_equal(before.view(np.uint32), z["rgba"].view(np.uint32))
    state = (renderer.last_pipeline(), renderer.last_parts())
    renderer.reset_counters()      # (it waits for the render and takes in what its snapshot says about the ray cost)
    zero = renderer.counters()
    cost = renderer.ray_cost()
    points, R = c["sets"]["uniform"], _reach("cornell", "uniform", 9)
    recs, counts = renderer.query_within(points, R, 8)
    assert renderer.last_kernel() == SHALLOW
    _device(renderer, c["sets"]["surface"], _reach("cornell", "surface", 2), 2)
    assert renderer.ray_cost() == cost
    got = renderer.counters()
    assert got["raysTraced"] - zero["raysTraced"] == len(points) + len(c["sets"]["surface"])
    assert got["raysHit"] - zero["raysHit"] == len(points) + len(c["sets"]["surface"]) and (counts > 0).all()
    assert got["boxTests"] > zero["boxTests"] and got["triTests"] > zero["triTests"]
    for key in got:
        if key not in ("boxTests", "triTests", "raysTraced", "raysHit"):
            assert got[key] == zero[key], key
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state
    # and the nearest query after it is what it was
    want = engine.nearest_to_numpy(engine.nearest_exhaustive(c["scene"].arrays(), points))
    near = engine.nearest_to_numpy(renderer.query_nearest(points))
    assert np.array_equal(near["dst"].view(np.uint32), want["dst"].view(np.uint32)) and np.array_equal(near["found"], want["found"])


@pytest.mark.gpu
def test_after_update_objects_the_answers_follow_the_moved_object(renderer):
    """The reference is the exhaustive loop over the host arrays before and after the move: its own answers change, and the device
    equals it each time, so the device read the moved tables."""
    e = pq.build_scene("instances")
    renderer.upload_scene(e)
    case = pq.case("instances")
    points = np.concatenate([case["sets"]["surface"], case["sets"]["uniform"]])
    n = len(points)
    R = np.full(n, 0.25, np.float32)
    before, cb, _, _, _ = _device(renderer, points, R, 8)
    recs, counts_before = engine.within_exhaustive(e.arrays(), points, R, 8)
    _assert_equal((before, cb), (wf.raw(recs, n, 8), counts_before), "instances before the move")
    e.set_transform(1, engine.placement(position=(0.2, -0.4, 0.5), rotation=(15, -40, 70), scale=(0.8, 1.3, 0.5)))
    e.push(renderer, "objects")
    after, ca, kernel, _, _ = _device(renderer, points, R, 8)
    assert kernel == SHALLOW
    recs, counts_after = engine.within_exhaustive(e.arrays(), points, R, 8)
    print(f"the move changes the reference's count on {int((counts_after != counts_before).sum())} of {n} points")
    assert (counts_after != counts_before).any(), "the move does not change the reference: the test shows nothing"
    _assert_equal((after, ca), (wf.raw(recs, n, 8), counts_after), "instances after the move")


@pytest.mark.gpu
def test_empty_batch_and_refusals_through_the_c_abi(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    recs, counts = renderer.query_within(np.zeros((0, 3), np.float32), None, 8)
    assert len(recs) == 0 and len(counts) == 0
    l, h = renderer._l, renderer._h
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    po, pc = to_device(renderer, "w_out", guard), to_device(renderer, "w_counts", guard)
    pp = to_device(renderer, "w_points", c["sets"]["uniform"][:16])
    empty = _capi.RtPointBatch(None, None, 0)
    assert l.rt_query_within(h, C.byref(empty), 99, None, None) == 0 and l.rt_query_within_host(h, C.byref(empty), 99, None, None) == 0
    for fn in ("rt_query_within", "rt_query_within_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host, cnt_host = (_capi.RtNearest * (16 * 8))(), (C.c_uint32 * 16)()
        out, cnt = (C.addressof(out_host), C.addressof(cnt_host)) if host else (po, pc)
        pts = c["sets"]["uniform"][:16].ctypes.data if host else pp
        ok = _capi.RtPointBatch(pts, None, 5)
        big = _capi.RtPointBatch(pts, None, 1 << 30)
        for batch, k, o, cn, message in ((None, 8, out, cnt, "the batch is NULL"),
                                         (_capi.RtPointBatch(None, None, 5), 8, out, cnt, "points and the output are required"),
                                         (ok, 9, out, cnt, "k = 9 is above RT_WITHIN_MAX_K = 8"),
                                         (ok, 8, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 0, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 1, None, cnt, "counts and, with k > 0, the output are required"),
                                         (big, 8, out, cnt, "a batch of 1073741824 points does not fit the 30 bits of a slot id"),
                                         (_capi.RtPointBatch(None, None, 1 << 30), 9, None, None, "points and the output are required"),   # the order
                                         (big, 9, None, None, "k = 9 is above RT_WITHIN_MAX_K = 8"),
                                         (big, 8, None, cnt, "counts and, with k > 0, the output are required")):
            assert call(h, C.byref(batch) if batch is not None else None, k, o, cn) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {message}", l.rt_last_error(h).decode()
        assert not np.frombuffer(out_host, np.uint8).any() and not np.frombuffer(cnt_host, np.uint8).any()
    renderer.sync()
    for name in ("w_out", "w_counts"):
        renderer._owned[name].download(into=guard)
        assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        b = _capi.RtPointBatch(pp, None, 16)
        assert fresh._l.rt_query_within(fresh._h, C.byref(b), 8, po, pc) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_within before rt_upload_scene"
        assert fresh._l.rt_query_within_host(fresh._h, None, 8, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_within_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_within(c["sets"]["uniform"], np.ones(5, np.float32), 2)
    with pytest.raises(engine.RtError, match="RT_WITHIN_MAX_K"):
        renderer.query_within(c["sets"]["uniform"][:4], None, 9)
    with pytest.raises(ValueError):
        renderer.query_within(1 << 20, None, 2, n=4, out=1 << 21)    # a device pointer without counts=
    with pytest.raises(ValueError):
        renderer.query_within(1 << 20, None, 2, n=4, counts=1 << 21)   # k > 0 without out=
