"""Signed point queries on the GPU (rt_upload_topology, rt_query_nearest_signed, rt_query_nearest_signed_host;
Renderer.query_nearest_signed; DESIGN.md, "Signed point queries").

The contract (include/rt_amd.h, include/rt_point_side.h): the records are rt_query_nearest's bit for bit; side is a function of the
point and the reported record alone, so rt_nearest_side_host on the device's own records reproduces it byte for byte, for every
point; and for every point the float64 reference keeps (tests/side_float64.py: the winding number about the reported triangle's
component) it is the reference's sign where that component is signable and 0 where it is not. The scenes and point sets are
tests/side_cases.py's."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import side_cases as sc
from util import EditedScene, to_device

pytestmark = pytest.mark.gpu

MISS_DST = np.float32(99999999.0)
REC = C.sizeof(_capi.RtNearest)
SIDE_KERNEL, SHALLOW = "k_nearest_side<256>", "k_nearest_points<24, true>"


def _signed(renderer, points, T=None, guard=0):
    """Through the device entry point: (the records' bytes [n, 48], side [n] int8, the kernel named, the guard bytes behind both)."""
    n = len(points)
    renderer.sync()
    pp = to_device(renderer, "s_points", points)
    pt = None if T is None else to_device(renderer, "s_limits", T)
    raw = np.full(n * REC + guard, 0xA5, np.uint8)
    sd = np.full(n + guard, 0x5A, np.uint8)
    po, ps = to_device(renderer, "s_out", raw), to_device(renderer, "s_side", sd)
    renderer.query_nearest_signed(pp, pt, n=n, out=po, side=ps, sync=False)
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["s_out"].download(into=raw)
    renderer._owned["s_side"].download(into=sd)
    return raw[:n * REC].reshape(n, REC), sd[:n].view(np.int8).copy(), kernel, (raw[n * REC:], sd[n:])


def _plain(renderer, points, T=None):
    """rt_query_nearest's bytes for the same points (the device entry point)."""
    n = len(points)
    renderer.sync()
    pp = to_device(renderer, "s_points", points)
    pt = None if T is None else to_device(renderer, "s_limits", T)
    raw = np.full(n * REC, 0xA5, np.uint8)
    po = to_device(renderer, "s_plain", raw)
    renderer.query_nearest(pp, pt, n=n, out=po)
    renderer._owned["s_plain"].download(into=raw)
    return raw.reshape(n, REC)


def _records(raw):
    return (_capi.RtNearest * len(raw)).from_buffer_copy(raw.tobytes())


def _upload(renderer, scene, dynamic=False):
    renderer.upload_scene(scene, dynamic=dynamic)
    renderer.upload_topology(scene)


@pytest.mark.parametrize("name", sc.SCENES)
def test_records_host_parity_and_truth(renderer, name):
    c = sc.case(name)
    _upload(renderer, c["scene"])
    arrays = c["scene"].arrays()
    for k, points in c["sets"].items():
        what = f"{name}/{k}"
        raw, side, kernel, _ = _signed(renderer, points)
        assert kernel == SIDE_KERNEL, (what, kernel)
        # 1. the records are rt_query_nearest's, in both forms
        assert np.array_equal(raw, _plain(renderer, points)), f"{what}: the records differ from rt_query_nearest's"
        host_recs, host_side = renderer.query_nearest_signed(points)
        assert np.array_equal(np.frombuffer(host_recs, np.uint8).reshape(len(points), REC), raw), f"{what}: the _host form's records differ"
        assert np.array_equal(host_side, side), f"{what}: the _host form's sides differ"
        # 2. the host rule on the device's own records, every point
        want = engine.nearest_side_host(arrays, points, _records(raw))
        bad = np.flatnonzero(want != side)
        assert len(bad) == 0, f"{what}: side differs from rt_nearest_side_host at {bad[:5].tolist()}: {side[bad[:5]].tolist()} against {want[bad[:5]].tolist()}"
        # 3. the truth
        rec = engine.nearest_to_numpy(_records(raw))
        t = sc.check_sides(c, points, rec, side, c["ref"][k], what)
        print(f"{what}: sides -1/0/+1 {(side == -1).sum()}/{(side == 0).sum()}/{(side == 1).sum()}, excluded {t['excluded'].mean():.2%}")
        tri = (rec["found"] != 0) & (rec["isSphere"] == 0)
        if name == "klein":
            assert not side.any()
        if name == "mixed":
            bunny = tri & (rec["objectIndex"] == c["arrays"]["objects"].shape[0] - 1)
            assert not side[tri & ~t["signable"]].any() and not side[bunny].any() and side[rec["isSphere"] != 0].all()
    if name == "torus_flipped":          # every side equals the unflipped scene's, and the statistics report the flips
        flips = int(sc.flipped(sc.torus_mesh())[1].sum())
        assert c["scene"].scene.topology()[0]["flippedTriangles"] in (flips, 576 - flips)
        sides = {k: _signed(renderer, p)[1] for k, p in c["sets"].items()}
        _upload(renderer, sc.case("torus")["scene"])
        for k, p in c["sets"].items():
            assert np.array_equal(_signed(renderer, p)[1], sides[k]), k


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_batch_sizes(renderer, n):
    c = sc.case("spikes")
    _upload(renderer, c["scene"])
    points = np.concatenate([c["sets"][k] for k in ("features", "uniform", "inside")])[:n].copy()
    assert len(points) == n
    raw, side, kernel, (g_out, g_side) = _signed(renderer, points, guard=64)
    assert kernel == SIDE_KERNEL
    assert (g_out == 0xA5).all() and (g_side == 0x5A).all(), "bytes behind the batch's records or sides were written"
    assert np.array_equal(raw, _plain(renderer, points))
    assert np.array_equal(side, engine.nearest_side_host(c["scene"].arrays(), points, _records(raw)))
    assert set(np.unique(side).tolist()) <= {-1, 1}


def test_limits(renderer):
    """found == 0 gives side == 0, and a NaN or <= 0 limit is not searched; the pass's own count is the points it signed."""
    c = sc.case("cubes")
    _upload(renderer, c["scene"])
    points = c["sets"]["uniform"][:200]
    ref = c["ref"]["uniform"]["dst"][:200]
    T = (2.0 * ref).astype(np.float32)
    T[1::5] = (0.5 * ref[1::5]).astype(np.float32)                         # too short: nothing found
    bad = np.arange(200) % 5 == 3
    T[bad] = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), int(bad.sum()))
    renderer.sync()
    before = renderer.counters()
    raw, side, _, _ = _signed(renderer, points, T)
    after = renderer.counters()
    rec = engine.nearest_to_numpy(_records(raw))
    short = np.arange(200) % 5 == 1
    assert not rec["found"][bad | short].any() and not side[bad | short].any() and not raw[bad | short][:, 4:].any()
    assert rec["found"][~(bad | short)].all() and (side[~(bad | short)] != 0).all()
    assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
    assert after["raysHit"] - before["raysHit"] == int((~(bad | short)).sum())
    assert after["segments"] - before["segments"] == int((side != 0).sum())
    assert np.array_equal(raw, _plain(renderer, points, T))
    host_recs, host_side = renderer.query_nearest_signed(points, T)
    assert np.array_equal(np.frombuffer(host_recs, np.uint8).reshape(200, REC), raw) and np.array_equal(host_side, side)


def test_empty_batch_and_refusals(renderer):
    c, other = sc.case("cubes"), sc.case("spikes")
    l, h = renderer._l, renderer._h
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    po, ps = to_device(renderer, "s_out", guard), to_device(renderer, "s_side", guard)
    pp = to_device(renderer, "s_points", c["sets"]["uniform"][:16])
    host_pts = np.ascontiguousarray(c["sets"]["uniform"][:16])
    out_host, side_host = (_capi.RtNearest * 16)(), np.full(16, 0x5A, np.uint8)

    def refused(fn, batch, o, s, message):
        assert getattr(l, fn)(h, C.byref(batch) if batch is not None else None, o, s) != 0
        assert l.rt_last_error(h).decode() == f"{fn}: {message}"

    def args(fn):
        host = fn.endswith("_host")
        return (host_pts.ctypes.data, C.addressof(out_host), side_host.ctypes.data) if host else (pp, po, ps)

    fresh = engine.Renderer(renderer.device)
    try:
        for fn in ("rt_query_nearest_signed", "rt_query_nearest_signed_host"):
            pts, o, s = args(fn)
            assert getattr(fresh._l, fn)(fresh._h, C.byref(_capi.RtPointBatch(pts, None, 16)), o, s) != 0
            assert fresh._l.rt_last_error(fresh._h).decode() == f"{fn} before rt_upload_scene"
        a = c["scene"].arrays()
        assert fresh._l.rt_upload_topology(fresh._h, C.byref(a)) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_upload_topology before rt_upload_scene"
    finally:
        fresh.close()
    renderer.upload_scene(c["scene"])
    for fn in ("rt_query_nearest_signed", "rt_query_nearest_signed_host"):
        pts, o, s = args(fn)
        ok = _capi.RtPointBatch(pts, None, 16)
        refused(fn, ok, o, s, "no topology uploaded")
        refused(fn, None, o, s, "no topology uploaded")                    # the order: the topology comes before the batch
        renderer.upload_topology(other["scene"])
        refused(fn, ok, o, s, "topology does not match the uploaded scene")
        refused(fn, _capi.RtPointBatch(None, None, 0), None, None, "topology does not match the uploaded scene")
        renderer.upload_topology(c["scene"])
        refused(fn, None, o, s, "the batch is NULL")
        refused(fn, _capi.RtPointBatch(None, None, 5), o, s, "points, the output and side are required")
        refused(fn, _capi.RtPointBatch(pts, None, 5), None, s, "points, the output and side are required")
        refused(fn, _capi.RtPointBatch(pts, None, 5), o, None, "points, the output and side are required")
        refused(fn, _capi.RtPointBatch(pts, None, 1 << 30), o, s, "a batch of 1073741824 points does not fit the 30 bits of a slot id")
        assert getattr(l, fn)(h, C.byref(_capi.RtPointBatch(None, None, 0)), None, None) == 0
        # a new scene drops the table
        renderer.upload_scene(c["scene"])
        refused(fn, ok, o, s, "no topology uploaded")
    assert not np.frombuffer(out_host, np.uint8).any() and (side_host == 0x5A).all()
    renderer.sync()
    for name in ("s_out", "s_side"):
        renderer._owned[name].download(into=guard)
        assert (guard == 0x5A).all(), "a refused call wrote to its output"
    renderer.upload_topology(c["scene"])
    recs, side = renderer.query_nearest_signed(np.zeros((0, 3), np.float32))
    assert len(recs) == 0 and len(side) == 0
    with pytest.raises(ValueError):
        renderer.query_nearest_signed(pp, n=16, out=po)                     # device pointers without side=
    with pytest.raises(ValueError):
        renderer.query_nearest_signed(c["sets"]["uniform"], np.ones(5, np.float32))


def test_after_update_points_the_sides_are_a_fresh_uploads(renderer):
    """The adjacency is kept by contract: a radial scale per grid node moves coincident points alike."""
    scene = sc.build_scene("torus")
    deformed = sc.build_scene("torus", torus=sc.torus_mesh(radial=lambda u, v: 1.0 + 0.3 * np.sin(3 * u) * np.cos(2 * v)))
    before, p = scene.scene.points(), deformed.scene.points()
    assert before.shape == p.shape and not np.array_equal(before[:, :3], p[:, :3])
    _, weld_before = np.unique(before[:, :3] + np.float32(0), axis=0, return_inverse=True)
    _, weld_after = np.unique(p[:, :3] + np.float32(0), axis=0, return_inverse=True)
    assert len(set(zip(weld_before.ravel().tolist(), weld_after.ravel().tolist()))) == weld_before.max() + 1 == weld_after.max() + 1
    _upload(renderer, scene, dynamic=True)
    renderer.update_points(p, 0)
    points = sc.case("torus")["sets"]["uniform"]
    raw, side, _, _ = _signed(renderer, points)
    scene.scene.update_points(p, 0)
    _upload(renderer, scene)
    raw_fresh, side_fresh, _, _ = _signed(renderer, points)
    assert np.array_equal(raw, raw_fresh) and np.array_equal(side, side_fresh)
    assert np.array_equal(side, engine.nearest_side_host(scene.arrays(), points, _records(raw)))
    assert not np.array_equal(side, _signed_on(renderer, sc.case("torus"), points)), "the deformation moved no point across the surface"
    assert set(np.unique(side).tolist()) == {-1, 1}


def _signed_on(renderer, c, points):
    _upload(renderer, c["scene"])
    return _signed(renderer, points)[1]


def test_after_update_objects_mirrors_a_cube_its_sides_follow(renderer):
    """cube.obj is symmetric about its origin, so the mirrored placement covers the same region: inside stays inside only if the
    orientation table followed the objects."""
    c = sc.case("cubes")
    _upload(renderer, c["scene"])
    points = np.concatenate([c["sets"]["inside"], c["sets"]["uniform"]])
    raw, side, _, _ = _signed(renderer, points)
    rec = engine.nearest_to_numpy(_records(raw))
    first = rec["objectIndex"] == 0
    assert (side[first] == -1).any() and (side[first] == 1).any()
    e = EditedScene(c["scene"])
    e.set_transform(0, engine.placement(position=(-3.0, 0.2, 0.1), rotation=(20, 35, 10), scale=(-1.0, 1.0, 1.0)))
    assert engine.scene_topology(e.arrays())[0]["orientation"] == -1 and c["scene"].topology()[0]["orientation"] == 1
    e.push(renderer, "objects")
    raw2, side2, _, _ = _signed(renderer, points)
    assert np.array_equal(side2, engine.nearest_side_host(e.arrays(), points, _records(raw2)))
    rec2 = engine.nearest_to_numpy(_records(raw2))
    assert np.array_equal(rec2["objectIndex"], rec["objectIndex"])
    assert np.array_equal(side2, side), "a mirrored cube's sides did not follow"


def test_a_signed_query_leaves_rendering_alone(renderer):
    """After a pass, rt_render of the golden Cornell frame is bit-identical to one rendered before it: the framebuffer,
    last_pipeline, last_parts; ray_cost is unchanged; a following rt_query_nearest answers as before and names its own kernel."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_c1_64x64_4spp.npz"), allow_pickle=False)
    from util import cornell_scene
    scene = cornell_scene(True)
    _upload(renderer, scene)
    c = sc.case("mixed")
    points = c["sets"]["uniform"]
    pc = engine.push_constants(64, 64, singleRender=1, sampleLimit=4)
    before = renderer.render(pc, 64, 64)
    assert np.array_equal(before.view(np.uint32), z["rgba"].view(np.uint32))
    state = (renderer.last_pipeline(), renderer.last_parts())
    plain_before = _plain(renderer, points)
    assert renderer.last_kernel() == SHALLOW
    renderer.sync()
    cost = renderer.ray_cost()
    renderer.query_nearest_signed(points)
    _, side, kernel, _ = _signed(renderer, points)
    assert kernel == SIDE_KERNEL and renderer.last_kernel() == SIDE_KERNEL and side.any()
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    assert np.array_equal(_plain(renderer, points), plain_before)
    assert renderer.last_kernel() == SHALLOW
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state
