"""Point queries on the GPU (rt_query_nearest, rt_query_nearest_host; Renderer.query_nearest; DESIGN.md, "Point queries").

The contract (include/rt_amd.h, include/rt_point_query.h): dst and found are the minimum of one fp32 function over one set, so the
device answer equals rt_nearest_exhaustive_host's bit for bit in both, whatever the traversal pruned; which of several equally near
primitives is reported is not specified, so point, uv and the primitive are held to the float64 rules of
tests/point_query_cases.py: check_records instead. The scenes and point sets are that module's (each with its float64 answer,
computed once): Cornell with spheres, spheres only, Cornell + bunny908, four bunny instances (rotation + uniform scale, non-uniform
scale, shear, rotation + translation), 150 placed objects, and the comb-shaped chain whose depth takes the deep instantiation."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import point_query_cases as pq
from util import _deformed_bunny, to_device

pytestmark = pytest.mark.gpu

MISS_DST = np.float32(99999999.0)
FACTORS = (0.5, 0.999, 1.001, 2.0)
REC = C.sizeof(_capi.RtNearest)
SHALLOW, DEEP = "k_nearest_points<24, true>", "k_nearest_points<64, false>"


def _device_query(renderer, points, T=None, guard=0):
    """Through the device entry point: (the records' bytes [n, 48], the kernel that ran, the `guard` bytes behind them)."""
    n = len(points)
    renderer.sync()
    pp = to_device(renderer, "n_points", points)
    pt = None if T is None else to_device(renderer, "n_limits", T)
    raw = np.full(n * REC + guard, 0xA5, np.uint8)
    po = to_device(renderer, "n_out", raw)
    renderer.query_nearest(pp, pt, n=n, out=po, sync=False)
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["n_out"].download(into=raw)
    return raw[:n * REC].reshape(n, REC), kernel, raw[n * REC:]


def _records(raw):
    return engine.nearest_to_numpy((_capi.RtNearest * len(raw)).from_buffer_copy(raw.tobytes()))


def _host_bytes(recs, n):
    return np.frombuffer(recs, np.uint8).reshape(n, REC)


def _same_dst_and_found(got, want, what):
    assert np.array_equal(got["found"], want["found"]), f"{what}: found differs at {np.flatnonzero(got['found'] != want['found'])[:5].tolist()}"
    bad = np.flatnonzero(got["dst"].view(np.uint32) != want["dst"].view(np.uint32))
    assert len(bad) == 0, f"{what}: dst differs from the exhaustive loop's at {bad[:5].tolist()}: {got['dst'][bad[:5]]} against {want['dst'][bad[:5]]}"


@pytest.mark.parametrize("name", pq.SCENES)
def test_device_equals_the_exhaustive_loop_and_float64(renderer, name):
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    arrays = c["scene"].arrays()
    for k, points in c["sets"].items():
        what = f"{name}/{k}"
        raw, kernel, _ = _device_query(renderer, points)
        assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
        got = _records(raw)
        want = engine.nearest_to_numpy(engine.nearest_exhaustive(arrays, points))
        _same_dst_and_found(got, want, what)
        assert not raw[:, 40:].any(), f"{what}: the record's padding is not 0"
        pq.check_records(c, points, got, c["ref"][k], what)
        host = renderer.query_nearest(points)
        assert np.array_equal(_host_bytes(host, len(points)), raw), f"{what}: the _host form's bytes differ from the device form's"


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name", pq.SCENES)
def test_limits_on_the_uniform_set(renderer, name, factor):
    """found iff dst < T: bit for bit against the exhaustive loop, and against float64 with no point exempt."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    points, ref = c["sets"]["uniform"], c["ref"]["uniform"]
    T = (np.float64(factor) * ref["dst"]).astype(np.float32)
    exempt = np.abs(ref["dst"] - T.astype(np.float64)) <= ref["bound"]
    assert not exempt.any()
    raw, _, _ = _device_query(renderer, points, T)
    got = _records(raw)
    want = engine.nearest_to_numpy(engine.nearest_exhaustive(c["scene"].arrays(), points, T))
    _same_dst_and_found(got, want, f"{name} x {factor}")
    assert np.array_equal(got["found"] != 0, ref["dst"] < T.astype(np.float64))
    miss = got["found"] == 0
    assert (got["dst"][miss] == MISS_DST).all() and not raw[miss][:, 4:].any()
    if (~miss).any():
        pq.check_records(c, points[~miss], {k: v[~miss] for k, v in got.items()}, {k: v[~miss] for k, v in ref.items()}, f"{name} x {factor}")
    assert np.array_equal(_host_bytes(renderer.query_nearest(points, T), len(points)), raw)


def test_limits_that_admit_nothing_are_not_searched(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    points = c["sets"]["uniform"][:200]
    T = (2.0 * c["ref"]["uniform"]["dst"][:200]).astype(np.float32)
    bad = np.arange(200) % 5 == 3
    T[bad] = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), int(bad.sum()))
    renderer.sync()
    before = renderer.counters()
    raw, _, _ = _device_query(renderer, points, T)
    after = renderer.counters()
    got = _records(raw)
    assert not got["found"][bad].any() and (got["dst"][bad] == MISS_DST).all() and not raw[bad][:, 4:].any()
    assert got["found"][~bad].all()
    assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
    assert after["raysHit"] - before["raysHit"] == int((~bad).sum())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_batch_sizes(renderer, n):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    points = np.concatenate([c["sets"][k] for k in ("uniform", "surface", "vertices", "far")])[:n].copy()
    assert len(points) == n
    raw, kernel, guard = _device_query(renderer, points, guard=64)
    assert kernel == SHALLOW
    assert (guard == 0xA5).all(), "bytes behind the batch's records were written"
    _same_dst_and_found(_records(raw), engine.nearest_to_numpy(engine.nearest_exhaustive(c["scene"].arrays(), points)), f"n = {n}")
    assert np.array_equal(_host_bytes(renderer.query_nearest(points), n), raw)


def test_empty_batch_and_refusals(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    assert len(renderer.query_nearest(np.zeros((0, 3), np.float32))) == 0
    l, h = renderer._l, renderer._h
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    po = to_device(renderer, "n_out", guard)
    pp = to_device(renderer, "n_points", c["sets"]["uniform"][:16])
    empty = _capi.RtPointBatch(None, None, 0)
    assert l.rt_query_nearest(h, C.byref(empty), None) == 0 and l.rt_query_nearest_host(h, C.byref(empty), None) == 0
    for fn in ("rt_query_nearest", "rt_query_nearest_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host = (_capi.RtNearest * 16)()
        out = C.addressof(out_host) if host else po
        pts = c["sets"]["uniform"][:16].ctypes.data if host else pp
        for batch, o, message in ((None, out, "the batch is NULL"),
                                  (_capi.RtPointBatch(None, None, 5), out, "points and the output are required"),
                                  (_capi.RtPointBatch(pts, None, 5), None, "points and the output are required"),
                                  (_capi.RtPointBatch(pts, None, 1 << 30), out, "a batch of 1073741824 points does not fit the 30 bits of a slot id")):
            assert call(h, C.byref(batch) if batch is not None else None, o) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {message}"
        assert not np.frombuffer(out_host, np.uint8).any()
    renderer.sync()
    renderer._owned["n_out"].download(into=guard)
    assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        b = _capi.RtPointBatch(pp, None, 16)
        assert fresh._l.rt_query_nearest(fresh._h, C.byref(b), po) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_nearest before rt_upload_scene"
        assert fresh._l.rt_query_nearest_host(fresh._h, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_nearest_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_nearest(c["sets"]["uniform"], np.ones(5, np.float32))
    with pytest.raises(ValueError):
        renderer.query_nearest(1 << 20, n=4)   # a device pointer without out=


def test_pruning_works_at_all(renderer):
    """Not a performance figure: a traversal that has degenerated into the exhaustive loop tests every triangle for every point."""
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    points = c["sets"]["surface"]
    renderer.sync()
    before = renderer.counters()
    _device_query(renderer, points)
    after = renderer.counters()
    tri, box = after["triTests"] - before["triTests"], after["boxTests"] - before["boxTests"]
    print(f"cornell_bunny / surface: {tri / len(points):.1f} triangle and {box / len(points):.1f} box evaluations per point of {c['ns'].tri_count} triangles")
    assert 0 < tri < len(points) * c["ns"].tri_count / 4 and box > 0
    assert after["raysTraced"] - before["raysTraced"] == len(points) and after["raysHit"] - before["raysHit"] == len(points)


def test_after_update_points_the_answers_are_a_fresh_uploads(renderer):
    scene, p, first = _deformed_bunny()
    renderer.upload_scene(scene, dynamic=True)
    renderer.update_points(p, first)
    scene.update_points(p, first)
    rng = np.random.default_rng(77)
    points = rng.uniform(-1.5, 1.5, (1024, 3)).astype(np.float32)
    points[:, 1] -= 0.5
    refit, _, _ = _device_query(renderer, points)
    renderer.upload_scene(scene)
    fresh, _, _ = _device_query(renderer, points)
    assert np.array_equal(refit, fresh)
    _same_dst_and_found(_records(refit), engine.nearest_to_numpy(engine.nearest_exhaustive(scene.arrays(), points)), "deformed bunny")


def test_a_point_query_leaves_rendering_alone(renderer):
    """After a pass, rt_render of the golden Cornell frame is bit-identical to one rendered before it: the framebuffer,
    last_pipeline, last_parts; ray_cost is unchanged."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_c1_64x64_4spp.npz"), allow_pickle=False)
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    pc = engine.push_constants(64, 64, singleRender=1, sampleLimit=4)
    before = renderer.render(pc, 64, 64)
    assert np.array_equal(before.view(np.uint32), z["rgba"].view(np.uint32))
    state = (renderer.last_pipeline(), renderer.last_parts())
    renderer.sync()
    cost = renderer.ray_cost()
    renderer.query_nearest(c["sets"]["uniform"])
    _device_query(renderer, c["sets"]["surface"])
    assert renderer.last_kernel() == SHALLOW
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state
