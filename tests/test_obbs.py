"""Oriented box queries on the GPU (rt_query_oriented_boxes, rt_query_oriented_boxes_host; Renderer.query_oriented_boxes,
Renderer.voxelize(frame=...); DESIGN.md, "Oriented box queries"): every surface a closed box placed by a world-to-box frame
touches, the first k in index order, and the count.

The contract (include/rt_amd.h, include/rt_obb_overlap.h): the member set of a box is a function of the box, its frame and the
scene alone and the key that orders it is total, so the device (its own node numbering, its descent through the frame, the two
instantiations of k_obbs_overlap) must give what the exhaustive host loop over the host arrays gives (rt_obbs_exhaustive_host;
engine.obbs_exhaustive), bit for bit: every byte of every record and every count, for every k. The loop itself is held to a
float64 reference on the CPU (tests/test_obbs_host.py). The scenes are tests/point_query_cases.py's, the boxes
tests/obb_float64.py's: about 1.6 k a scene, around the points of its four sets, under four kinds of frame."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import obb_float64 as ob
import overlap_float64 as of
import point_query_cases as pq
from util import kernel_instantiations, to_device

KS = (0, 1, 2, 8)
REC = C.sizeof(_capi.RtOverlap)
SHALLOW, DEEP = "k_obbs_overlap<24, false>", "k_obbs_overlap<64, true>"
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)

_wants = {}


def _raw(recs, n, k):
    return np.frombuffer(recs, np.uint8).reshape(n, k, REC) if n * k else np.zeros((n, k, REC), np.uint8)


def _loop(arrays, frames, lo, hi, k):
    recs, counts = engine.obbs_exhaustive(arrays, frames, lo, hi, k)
    return _raw(recs, len(counts), k).copy(), counts


def _want(name, key, k):
    """The exhaustive loop's answer, once per session: (bytes [n, k, 16], counts)."""
    if (name, key, k) not in _wants:
        _wants[(name, key, k)] = _loop(pq.case(name)["scene"].arrays(), *ob.seed_obbs(name, key), k)
    return _wants[(name, key, k)]


def _device(renderer, frames, lo, hi, k, guard=0, shared=False):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own: (bytes [n, k, 16], counts, the
    kernel that ran, the `guard` bytes behind the records, the `guard` bytes behind the counts). shared: `frames` is one frame."""
    n = len(lo)
    renderer.sync()
    pf, pl, ph = to_device(renderer, "o_frames", frames), to_device(renderer, "o_lo", lo), to_device(renderer, "o_hi", hi)
    out = np.full(n * k * REC + guard, 0xA5, np.uint8)
    cnt = np.full(n * 4 + guard, 0xA5, np.uint8)
    po, pc = to_device(renderer, "o_out", out), to_device(renderer, "o_counts", cnt)
    batch = _capi.RtObbBatch(pf, pl, ph, n, 1 if shared else 0)
    rc = renderer._l.rt_query_oriented_boxes(renderer._h, C.byref(batch), k, C.c_void_p(po) if k else None, C.c_void_p(pc))
    assert rc == 0, renderer._l.rt_last_error(renderer._h).decode()
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["o_out"].download(into=out)
    renderer._owned["o_counts"].download(into=cnt)
    return out[:n * k * REC].reshape(n, k, REC), cnt[:n * 4].view(np.uint32).copy(), kernel, out[n * k * REC:], cnt[n * 4:]


def _assert_equal(got, want, what):
    (gb, gc), (wb, wc) = got, want
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.flatnonzero(gc != wc)[:5].tolist()}"
    assert np.array_equal(gb, wb), f"{what}: records differ at boxes {np.unique(np.argwhere(gb != wb)[:, 0])[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_device_equals_the_exhaustive_loop(renderer, name):
    """All bytes of all records and all counts, on every box set, k in {0, 1, 2, 8}; and the _host form."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    most = 0
    for key in c["sets"]:
        frames, lo, hi = ob.seed_obbs(name, key)
        n = len(lo)
        for k in KS:
            wb, wc = _want(name, key, k)
            what = f"{name}/{key}/k={k}"
            gb, gc, kernel, _, _ = _device(renderer, frames, lo, hi, k)
            assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
            _assert_equal((gb, gc), (wb, wc), what)
            hr, hc = renderer.query_oriented_boxes(frames, lo, hi, k)
            assert renderer.last_kernel() == kernel
            _assert_equal((_raw(hr, n, k), hc), (gb, gc), what + " / host form")
            most = max(most, int(wc.max()))
    os_ = ob.scene(name)
    assert most > 8 or len(os_.sph_c) + len(os_.W) <= 8, f"{name}: no box has more members than slots"


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_obbs_overlap") == {SHALLOW, DEEP}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n boxes alone equal their rows of the whole set, and the 64 bytes behind the
    records and behind the counts are left as they were."""
    c = pq.case("instances")
    renderer.upload_scene(c["scene"])
    frames, lo, hi = (a[:n].copy() for a in ob.seed_obbs("instances", "surface"))
    for k in (1, 8):
        wb, wc = _want("instances", "surface", k)
        gb, gc, kernel, g_out, g_cnt = _device(renderer, frames, lo, hi, k, guard=64)
        assert kernel == SHALLOW
        _assert_equal((gb, gc), (wb[:n], wc[:n]), f"n = {n}, k = {k}")
        assert (g_out == 0xA5).all() and (g_cnt == 0xA5).all(), f"n = {n}, k = {k}: bytes behind the batch's outputs were written"
        hr, hc = renderer.query_oriented_boxes(frames, lo, hi, k)
        _assert_equal((_raw(hr, n, k), hc), (gb, gc), f"n = {n}, k = {k} / host form")


@pytest.mark.gpu
def test_invalid_boxes_and_frames_are_not_searched(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    frames, lo, hi = (a[:240].copy() for a in ob.seed_obbs("cornell", "surface"))
    bad = np.arange(240) % 5 == 3
    which = np.arange(int(bad.sum())) % 6
    rows = np.flatnonzero(bad)
    frames[rows[which == 0], 12] = np.nan                 # the translation
    frames[rows[which == 1], 5] = np.inf                  # the linear part
    frames[rows[which == 2], 2] = -np.inf
    lo[rows[which == 3], 0] = np.nan
    hi[rows[which == 4], 1] = np.inf
    swap = rows[which == 5]
    lo[swap, 1], hi[swap, 1] = hi[swap, 1].copy(), lo[swap, 1].copy()          # inverted (the half-extents are positive)
    frames[~bad, 3], frames[~bad, 15] = np.nan, np.inf                         # never read: still valid
    for k in (0, 8):
        renderer.sync()
        before = renderer.counters()
        gb, gc, _, _, _ = _device(renderer, frames, lo, hi, k)
        after = renderer.counters()
        assert not gc[bad].any() and not gb[bad].any()
        assert (gc[~bad] >= 1).all()
        assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
        assert after["raysHit"] - before["raysHit"] == int((~bad).sum())
        _assert_equal((gb, gc), _loop(c["scene"].arrays(), frames, lo, hi, k), f"invalid boxes, k = {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell", "instances"))
def test_identity_frames_equal_the_box_query(renderer, name):
    """On Cornell and the placed scene: rt_query_boxes' bytes on the same boxes, per-box identity frames and a shared one."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    for key in ("uniform", "vertices"):
        lo, hi = of.seed_boxes(name, key)
        n = len(lo)
        for k in (0, 8):
            br, bc = renderer.query_boxes(lo, hi, k)
            want = (np.frombuffer(br, np.uint8).reshape(n, k, REC) if k else np.zeros((n, 0, REC), np.uint8), bc)
            gb, gc, _, _, _ = _device(renderer, np.tile(IDENTITY, (n, 1)), lo, hi, k)
            _assert_equal((gb, gc), want, f"{name}/{key}/k={k}: identity frames")
            sb, sc, _, _, _ = _device(renderer, IDENTITY, lo, hi, k, shared=True)
            _assert_equal((sb, sc), want, f"{name}/{key}/k={k}: a shared identity frame")
        assert bc.max() > 8


@pytest.mark.gpu
def test_a_shared_frame_equals_the_repeated_frame(renderer):
    c = pq.case("instances")
    renderer.upload_scene(c["scene"])
    frames, lo, hi = ob.seed_obbs("instances", "surface")
    for row in (0, 1, 2, 3):                                                   # one frame of each kind
        one, l, h = frames[row].copy(), lo[row::4].copy(), hi[row::4].copy()
        for k in (0, 8):
            sb, sc, kernel, _, _ = _device(renderer, one, l, h, k, shared=True)
            rb, rc, _, _, _ = _device(renderer, np.tile(one, (len(l), 1)), l, h, k)
            assert kernel == SHALLOW
            _assert_equal((sb, sc), (rb, rc), f"frame {row}, k = {k}")
            _assert_equal((sb, sc), _loop(c["scene"].arrays(), one, l, h, k), f"frame {row}, k = {k} / loop")
            hr, hc = renderer.query_oriented_boxes(one, l, h, k)               # a (16,) frame is passed as shared
            _assert_equal((_raw(hr, len(l), k), hc), (sb, sc), f"frame {row}, k = {k} / host form")
        assert sc.any()


@pytest.mark.gpu
def test_voxelize_in_a_frame(renderer):
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    os_ = ob.scene("cornell_bunny")
    p = np.concatenate([os_.W.reshape(-1, 3), os_.sph_c])
    lo, hi = (p.min(axis=0) - 0.01).astype(np.float32), (p.max(axis=0) + 0.01).astype(np.float32)
    dims = (12, 10, 8)
    plain = renderer.voxelize(lo, hi, dims)
    assert np.array_equal(renderer.voxelize(lo, hi, dims, frame=IDENTITY), plain) and plain.shape == (8, 10, 12)
    # a grid turned by 30 degrees about the vertical through the scene's middle, in its own coordinates
    a = np.radians(30.0)
    R = np.array([[[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]])
    frame = engine.obb_frames(((lo + hi) / 2)[None], R)[0]
    half = ((hi - lo) / 2).astype(np.float32)
    vox = renderer.voxelize(-half, half, dims, frame=frame)
    assert renderer.last_kernel() == SHALLOW and vox.shape == (8, 10, 12) and vox.dtype == np.uint32
    cl, ch = engine.grid_boxes(-half, half, dims)
    _, counts = engine.obbs_exhaustive(c["scene"].arrays(), frame, cl, ch, 0)
    assert np.array_equal(vox.reshape(-1), counts) and counts.any() and not np.array_equal(vox, plain)


@pytest.mark.gpu
def test_after_update_objects_the_answers_follow_the_moved_object(renderer):
    """The reference is the exhaustive loop over the host arrays before and after the move: its own answers change, and the device
    equals it each time, so the device read the moved tables."""
    e = pq.build_scene("instances")
    renderer.upload_scene(e)
    parts = [ob.seed_obbs("instances", key) for key in ("surface", "uniform")]
    frames, lo, hi = (np.concatenate([p[i] for p in parts]) for i in range(3))
    before, cb, _, _, _ = _device(renderer, frames, lo, hi, 8)
    wb, counts_before = _loop(e.arrays(), frames, lo, hi, 8)
    _assert_equal((before, cb), (wb, counts_before), "instances before the move")
    e.set_transform(1, engine.placement(position=(0.2, -0.4, 0.5), rotation=(15, -40, 70), scale=(0.8, 1.3, 0.5)))
    e.push(renderer, "objects")
    after, ca, kernel, _, _ = _device(renderer, frames, lo, hi, 8)
    assert kernel == SHALLOW
    wa, counts_after = _loop(e.arrays(), frames, lo, hi, 8)
    print(f"the move changes the reference's count on {int((counts_after != counts_before).sum())} of {len(lo)} boxes")
    assert (counts_after != counts_before).any(), "the move does not change the reference: the test shows nothing"
    _assert_equal((after, ca), (wa, counts_after), "instances after the move")


@pytest.mark.gpu
def test_an_oriented_box_query_leaves_rendering_alone(renderer):
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
    frames, lo, hi = ob.seed_obbs("cornell", "vertices")
    recs, counts = renderer.query_oriented_boxes(frames, lo, hi, 8)
    assert renderer.last_kernel() == SHALLOW
    sf, slo, shi = ob.seed_obbs("cornell", "surface")
    _device(renderer, sf, slo, shi, 2)
    assert renderer.ray_cost() == cost
    got = renderer.counters()
    assert got["raysTraced"] - zero["raysTraced"] == len(lo) + len(slo)
    assert got["raysHit"] - zero["raysHit"] == len(lo) + len(slo) and (counts > 0).all()
    assert got["boxTests"] > zero["boxTests"] and got["triTests"] > zero["triTests"]
    for key in got:
        if key not in ("boxTests", "triTests", "raysTraced", "raysHit"):
            assert got[key] == zero[key], key
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state
    # and the box query after it is what the loop says
    blo, bhi = of.seed_boxes("cornell", "uniform")
    br, bc = renderer.query_boxes(blo, bhi, 8)
    wr, wc = engine.boxes_exhaustive(c["scene"].arrays(), blo, bhi, 8)
    assert np.array_equal(bc, wc) and bytes(br) == bytes(wr)


@pytest.mark.gpu
def test_empty_batch_and_refusals_through_the_c_abi(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    none = np.zeros((0, 3), np.float32)
    recs, counts = renderer.query_oriented_boxes(np.zeros((0, 16), np.float32), none, none, 8)
    assert len(recs) == 0 and len(counts) == 0
    l, h = renderer._l, renderer._h
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    po, pc = to_device(renderer, "o_out", guard), to_device(renderer, "o_counts", guard)
    bf, blo, bhi = (a[:16].copy() for a in ob.seed_obbs("cornell", "uniform"))
    pf, pl, ph = to_device(renderer, "o_frames", bf), to_device(renderer, "o_lo", blo), to_device(renderer, "o_hi", bhi)
    empty = _capi.RtObbBatch(None, None, None, 0, 5)
    assert l.rt_query_oriented_boxes(h, C.byref(empty), 99, None, None) == 0 and l.rt_query_oriented_boxes_host(h, C.byref(empty), 99, None, None) == 0
    for fn in ("rt_query_oriented_boxes", "rt_query_oriented_boxes_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host, cnt_host = (_capi.RtOverlap * (16 * 8))(), (C.c_uint32 * 16)()
        out, cnt = (C.addressof(out_host), C.addressof(cnt_host)) if host else (po, pc)
        f_, lo_, hi_ = (bf.ctypes.data, blo.ctypes.data, bhi.ctypes.data) if host else (pf, pl, ph)
        ok = _capi.RtObbBatch(f_, lo_, hi_, 5, 0)
        big = _capi.RtObbBatch(f_, lo_, hi_, 1 << 30, 0)
        for batch, k, o, cn, message in ((None, 8, out, cnt, "the batch is NULL"),
                                         (_capi.RtObbBatch(None, lo_, hi_, 5, 0), 8, out, cnt, "frames, lo and hi are required"),
                                         (_capi.RtObbBatch(f_, None, hi_, 5, 0), 8, out, cnt, "frames, lo and hi are required"),
                                         (_capi.RtObbBatch(f_, lo_, None, 5, 1), 8, out, cnt, "frames, lo and hi are required"),
                                         (ok, 9, out, cnt, "k = 9 is above RT_BOXES_MAX_K = 8"),
                                         (_capi.RtObbBatch(f_, lo_, hi_, 5, 2), 8, out, cnt, "sharedFrame = 2 is neither 0 nor 1"),
                                         (ok, 8, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 0, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 1, None, cnt, "counts and, with k > 0, the output are required"),
                                         (big, 8, out, cnt, "a batch of 1073741824 boxes does not fit the 30 bits of a slot id"),
                                         (_capi.RtObbBatch(None, None, None, 1 << 30, 2), 9, None, None, "frames, lo and hi are required"),   # the order
                                         (_capi.RtObbBatch(f_, lo_, hi_, 1 << 30, 2), 9, None, None, "k = 9 is above RT_BOXES_MAX_K = 8"),
                                         (_capi.RtObbBatch(f_, lo_, hi_, 1 << 30, 2), 8, None, None, "sharedFrame = 2 is neither 0 nor 1"),
                                         (big, 8, None, cnt, "counts and, with k > 0, the output are required")):
            assert call(h, C.byref(batch) if batch is not None else None, k, o, cn) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {message}", l.rt_last_error(h).decode()
        assert not np.frombuffer(out_host, np.uint8).any() and not np.frombuffer(cnt_host, np.uint8).any()
    renderer.sync()
    for name in ("o_out", "o_counts"):
        renderer._owned[name].download(into=guard)
        assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        b = _capi.RtObbBatch(pf, pl, ph, 16, 0)
        assert fresh._l.rt_query_oriented_boxes(fresh._h, C.byref(b), 8, po, pc) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_oriented_boxes before rt_upload_scene"
        assert fresh._l.rt_query_oriented_boxes_host(fresh._h, None, 8, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_oriented_boxes_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_oriented_boxes(bf, blo, bhi[:5], 2)
    with pytest.raises(ValueError):
        renderer.query_oriented_boxes(bf[:3], blo, bhi, 2)
    with pytest.raises(engine.RtError, match="RT_BOXES_MAX_K"):
        renderer.query_oriented_boxes(bf[:4], blo[:4], bhi[:4], 9)
    with pytest.raises(ValueError):
        renderer.query_oriented_boxes(1 << 19, 1 << 20, 1 << 22, 2, n=4, out=1 << 21)    # device pointers without counts=
    with pytest.raises(ValueError):
        renderer.query_oriented_boxes(1 << 19, 1 << 20, 1 << 22, 2, n=4, counts=1 << 21)   # k > 0 without out=
    # device memory through the Python method: integer pointers are n frames
    assert renderer.query_oriented_boxes(pf, pl, ph, 8, n=16, out=po, counts=pc) is None
    got = np.zeros(4096, np.uint8)
    renderer._owned["o_counts"].download(into=got)
    assert np.array_equal(got[:64].view(np.uint32), engine.obbs_exhaustive(c["scene"].arrays(), bf, blo, bhi, 0)[1])
