"""Box queries on the GPU (rt_query_boxes, rt_query_boxes_host; Renderer.query_boxes, Renderer.voxelize; DESIGN.md, "Box
queries"): every surface a closed axis-aligned box touches, the first k in index order, and the count.

The contract (include/rt_amd.h, include/rt_box_overlap.h): the member set of a box is a function of the box and the scene alone
and the key that orders it is total, so the device (its own node numbering, its pruned descent, the two instantiations of
k_boxes_overlap) must give what the exhaustive host loop over the host arrays gives (rt_boxes_exhaustive_host;
engine.boxes_exhaustive), bit for bit: every byte of every record and every count, for every k. The loop itself is held to a
float64 reference on the CPU (tests/test_boxes_host.py). The scenes are tests/point_query_cases.py's, the boxes
tests/overlap_float64.py's: about 1.6 k a scene, around the points of its four sets."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import overlap_float64 as of
import point_query_cases as pq
from util import _deformed_bunny, kernel_instantiations, to_device

KS = (0, 1, 2, 8)
REC = C.sizeof(_capi.RtOverlap)
SHALLOW, DEEP = "k_boxes_overlap<24, false>", "k_boxes_overlap<64, true>"

_wants = {}


def _boxes(name, key):
    return of.seed_boxes(name, key)


def _raw(recs, n, k):
    return np.frombuffer(recs, np.uint8).reshape(n, k, REC) if n * k else np.zeros((n, k, REC), np.uint8)


def _loop(arrays, lo, hi, k):
    recs, counts = engine.boxes_exhaustive(arrays, lo, hi, k)
    return _raw(recs, len(counts), k).copy(), counts


def _want(name, key, k):
    """The exhaustive loop's answer, once per session: (bytes [n, k, 16], counts)."""
    if (name, key, k) not in _wants:
        _wants[(name, key, k)] = _loop(pq.case(name)["scene"].arrays(), *_boxes(name, key), k)
    return _wants[(name, key, k)]


def _device(renderer, lo, hi, k, guard=0):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own: (bytes [n, k, 16], counts, the
    kernel that ran, the `guard` bytes behind the records, the `guard` bytes behind the counts)."""
    n = len(lo)
    renderer.sync()
    pl, ph = to_device(renderer, "b_lo", lo), to_device(renderer, "b_hi", hi)
    out = np.full(n * k * REC + guard, 0xA5, np.uint8)
    cnt = np.full(n * 4 + guard, 0xA5, np.uint8)
    po, pc = to_device(renderer, "b_out", out), to_device(renderer, "b_counts", cnt)
    assert renderer.query_boxes(pl, ph, k, n=n, out=po if k else None, counts=pc, sync=False) is None
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["b_out"].download(into=out)
    renderer._owned["b_counts"].download(into=cnt)
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
        lo, hi = _boxes(name, key)
        n = len(lo)
        for k in KS:
            wb, wc = _want(name, key, k)
            what = f"{name}/{key}/k={k}"
            gb, gc, kernel, _, _ = _device(renderer, lo, hi, k)
            assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
            _assert_equal((gb, gc), (wb, wc), what)
            hr, hc = renderer.query_boxes(lo, hi, k)
            _assert_equal((_raw(hr, n, k), hc), (gb, gc), what + " / host form")
            most = max(most, int(wc.max()))
    surfaces = len(c["ns"].sph_c) + len(c["ns"].W)
    assert most > 8 or surfaces <= 8, f"{name}: no box has more members than slots"


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_boxes_overlap") == {SHALLOW, DEEP}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n boxes alone equal their rows of the whole set, and the 64 bytes behind the
    records and behind the counts are left as they were."""
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    lo, hi = (a[:n].copy() for a in _boxes("cornell", "uniform"))
    for k in (1, 8):
        wb, wc = _want("cornell", "uniform", k)
        gb, gc, kernel, g_out, g_cnt = _device(renderer, lo, hi, k, guard=64)
        assert kernel == SHALLOW
        _assert_equal((gb, gc), (wb[:n], wc[:n]), f"n = {n}, k = {k}")
        assert (g_out == 0xA5).all() and (g_cnt == 0xA5).all(), f"n = {n}, k = {k}: bytes behind the batch's outputs were written"
        hr, hc = renderer.query_boxes(lo, hi, k)
        _assert_equal((_raw(hr, n, k), hc), (gb, gc), f"n = {n}, k = {k} / host form")


@pytest.mark.gpu
def test_invalid_boxes_are_not_searched(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    lo, hi = (a[:200].copy() for a in _boxes("cornell", "surface"))
    bad = np.arange(200) % 5 == 3
    which = np.arange(int(bad.sum())) % 4
    lo[bad, 0] = np.where(which == 0, np.nan, lo[bad, 0])
    hi[bad, 1] = np.where(which == 1, np.inf, hi[bad, 1])
    lo[bad, 2] = np.where(which == 2, -np.inf, lo[bad, 2])
    swap = np.flatnonzero(bad)[which == 3]
    lo[swap, 1], hi[swap, 1] = hi[swap, 1].copy(), lo[swap, 1].copy()          # inverted (the half-extents are positive)
    for k in (0, 8):
        renderer.sync()
        before = renderer.counters()
        gb, gc, _, _, _ = _device(renderer, lo, hi, k)
        after = renderer.counters()
        assert not gc[bad].any() and not gb[bad].any()
        assert (gc[~bad] >= 1).all()
        assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
        assert after["raysHit"] - before["raysHit"] == int((~bad).sum())
        _assert_equal((gb, gc), _loop(c["scene"].arrays(), lo, hi, k), f"invalid boxes, k = {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_exact_relations_on_the_device(renderer, name):
    """Counts do not depend on k; the list at a smaller k is the head of the list at a larger one; keys strictly ascend; and a box
    equal to the scene's whole bounds counts every surface the exhaustive loop counts."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    for key in ("uniform", "vertices"):
        lo, hi = _boxes(name, key)
        eight, counts, _, _, _ = _device(renderer, lo, hi, 8)
        for k in (0, 1, 2):
            gb, gc, _, _, _ = _device(renderer, lo, hi, k)
            assert np.array_equal(gc, counts) and np.array_equal(gb, eight[:, :k]), (name, key, k)
        w = eight.copy().view(np.uint32).reshape(len(lo), 8, 4).astype(np.int64)
        have = np.minimum(counts, 8)
        held = np.arange(8)[None, :] < have[:, None]
        assert (w[..., 0] == held).all() and not w[~held].any(), (name, key)
        key64 = ((1 - w[..., 1]) << 62) + (w[..., 2] << 31) + w[..., 3]        # spheres first, then the index, then the triangle
        both = held[:, 1:]
        assert (key64[:, :-1][both] < key64[:, 1:][both]).all(), f"{name}/{key}: keys do not strictly ascend"
    blo, bhi = c["ns"].box()
    whole = (np.floor(blo) - 1).astype(np.float32)[None], (np.ceil(bhi) + 1).astype(np.float32)[None]
    tight = blo.astype(np.float32)[None], bhi.astype(np.float32)[None]
    for lo, hi in (whole, tight):
        _, gc, _, _, _ = _device(renderer, lo, hi, 0)
        _, wc = _loop(c["scene"].arrays(), lo, hi, 0)
        assert np.array_equal(gc, wc), (name, gc, wc)
    assert wc[0] > 0 and _loop(c["scene"].arrays(), *whole, 0)[1][0] == len(c["ns"].sph_c) + len(c["ns"].W)


@pytest.mark.gpu
def test_degenerate_boxes_on_cornell(renderer):
    """Point boxes on mesh vertices and flat boxes in the walls' planes: where an over-eager prune would lose a member. Every one
    is held to the loop byte for byte; those made from the objects whose matrix holds only 0 and +-1 beside its translation (the
    walls: their fp32 world corners are the float64 ones) must also touch the triangle they were made from."""
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    a = c["scene"].arrays()
    plain = np.array([all(abs(a.objects[i].transformMatrix[col * 4 + r]) in (0.0, 1.0) for col in range(3) for r in range(3)) for i in range(a.objectCount)])
    W = c["ns"].W.astype(np.float32)
    walls = W[plain[c["ns"].obj]]
    assert len(walls) >= 10, "the Cornell box has no walls?"
    v = np.concatenate([c["sets"]["vertices"], walls.reshape(-1, 3)])
    flat_lo, flat_hi = [], []
    for t in walls:                                     # every wall triangle's own box: flat in the wall's plane
        lo, hi = t.min(axis=0), t.max(axis=0)
        assert (lo == hi).any()
        flat_lo.append(lo); flat_hi.append(hi)
        flat_lo.append(np.where(lo == hi, lo, (lo + hi) / 2)); flat_hi.append(hi)       # and a quarter of it, from its centre
    lo = np.concatenate([v, np.array(flat_lo, np.float32)])
    hi = np.concatenate([v, np.array(flat_hi, np.float32)])
    for k in (0, 8):
        gb, gc, _, _, _ = _device(renderer, lo, hi, k)
        wb, wc = _loop(a, lo, hi, k)
        _assert_equal((gb, gc), (wb, wc), f"degenerate boxes, k = {k}")
    made = wc[len(c["sets"]["vertices"]):]
    assert (made >= 1).all(), "a point box on a wall's vertex or a flat box in a wall touches nothing"
    assert (made >= 2).any()


@pytest.mark.gpu
def test_after_update_objects_the_answers_follow_the_moved_object(renderer):
    """The reference is the exhaustive loop over the host arrays before and after the move: its own answers change, and the device
    equals it each time, so the device read the moved tables."""
    e = pq.build_scene("instances")
    renderer.upload_scene(e)
    lo = np.concatenate([_boxes("instances", "surface")[0], _boxes("instances", "uniform")[0]])
    hi = np.concatenate([_boxes("instances", "surface")[1], _boxes("instances", "uniform")[1]])
    before, cb, _, _, _ = _device(renderer, lo, hi, 8)
    wb, counts_before = _loop(e.arrays(), lo, hi, 8)
    _assert_equal((before, cb), (wb, counts_before), "instances before the move")
    e.set_transform(1, engine.placement(position=(0.2, -0.4, 0.5), rotation=(15, -40, 70), scale=(0.8, 1.3, 0.5)))
    e.push(renderer, "objects")
    after, ca, kernel, _, _ = _device(renderer, lo, hi, 8)
    assert kernel == SHALLOW
    wa, counts_after = _loop(e.arrays(), lo, hi, 8)
    print(f"the move changes the reference's count on {int((counts_after != counts_before).sum())} of {len(lo)} boxes")
    assert (counts_after != counts_before).any(), "the move does not change the reference: the test shows nothing"
    _assert_equal((after, ca), (wa, counts_after), "instances after the move")


@pytest.mark.gpu
def test_after_update_points_the_answers_follow_the_refit(renderer):
    scene, p, first = _deformed_bunny()
    renderer.upload_scene(scene, dynamic=True)
    rng = np.random.default_rng(78)
    centre = rng.uniform(-1.0, 1.0, (1024, 3)).astype(np.float32)
    centre[:, 1] -= 0.3
    half = rng.uniform(0.02, 0.3, (1024, 3)).astype(np.float32)
    lo, hi = centre - half, centre + half
    _, counts_before = _loop(scene.arrays(), lo, hi, 8)
    gb, gc, _, _, _ = _device(renderer, lo, hi, 8)
    _assert_equal((gb, gc), _loop(scene.arrays(), lo, hi, 8), "before the deformation")
    renderer.update_points(p, first)
    scene.update_points(p, first)
    wb, counts_after = _loop(scene.arrays(), lo, hi, 8)
    assert (counts_after != counts_before).any(), "the deformation does not change the reference: the test shows nothing"
    gb, gc, _, _, _ = _device(renderer, lo, hi, 8)
    _assert_equal((gb, gc), (wb, counts_after), "after the deformation")


@pytest.mark.gpu
def test_voxelize_is_the_box_query_over_the_grid(renderer):
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    blo, bhi = c["ns"].box()
    lo, hi = (blo - 0.01).astype(np.float32), (bhi + 0.01).astype(np.float32)
    dims = (16, 16, 16)
    vox = renderer.voxelize(lo, hi, dims)
    assert vox.shape == (16, 16, 16) and vox.dtype == np.uint32
    cl, ch = engine.grid_boxes(lo, hi, dims)
    _, counts = renderer.query_boxes(cl, ch, 0)
    assert np.array_equal(vox.reshape(-1), counts)
    _, gc, kernel, _, _ = _device(renderer, cl, ch, 0)
    assert kernel == SHALLOW and np.array_equal(gc, counts)
    assert np.array_equal(counts, _loop(c["scene"].arrays(), cl, ch, 0)[1])
    # every triangle whose corners lie inside the grid is a member of at least one cell, by the loop: asked of a scene cut down
    # to that one triangle (one object, one leaf), about the cells that hold its corners
    W = c["ns"].W.astype(np.float32)
    inside = ((W >= lo) & (W <= hi)).all(axis=(1, 2))
    assert inside.sum() >= len(W) - 2
    edges = [np.concatenate([cl[:16, 0], ch[15:16, 0]]), np.concatenate([cl[:256:16, 1], ch[240:256:16, 1]]), np.concatenate([cl[::256, 2], ch[-1:, 2]])]
    a = c["scene"].arrays()
    leaf, one = (_capi.BVHNode * 1)(), (_capi.RenderObject * 1)()
    objects = C.cast(a.objects, C.c_void_p).value            # the address: the field itself is about to change
    a.sphereCount, a.objectCount, a.bvhNodeCount = 0, 1, 1
    a.objects, a.bvhNodes = C.cast(one, C.POINTER(_capi.RenderObject)), C.cast(leaf, C.POINTER(_capi.BVHNode))
    for row in np.flatnonzero(inside):
        C.memmove(one, objects + int(c["ns"].obj[row]) * C.sizeof(_capi.RenderObject), C.sizeof(_capi.RenderObject))
        one[0].bvhIndex = 0
        leaf[0].index, leaf[0].triCount = int(c["ns"].tri[row]), 1
        cell = [np.clip(np.searchsorted(edges[d], W[row, :, d], side="right") - 1, 0, 15) for d in range(3)]
        index = (cell[2] * 16 + cell[1]) * 16 + cell[0]
        _, member = engine.boxes_exhaustive(a, cl[index], ch[index], 0)
        assert member.max() == 1, f"triangle {int(c['ns'].tri[row])} of object {int(c['ns'].obj[row])} is in none of the cells that hold its corners"
        assert (vox.reshape(-1)[index] >= member).all()


@pytest.mark.gpu
def test_a_box_query_leaves_rendering_alone(renderer):
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
    lo, hi = _boxes("cornell", "vertices")
    recs, counts = renderer.query_boxes(lo, hi, 8)
    assert renderer.last_kernel() == SHALLOW
    slo, shi = _boxes("cornell", "surface")
    _device(renderer, slo, shi, 2)
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
    # and the nearest query after it is what it was
    points = c["sets"]["uniform"]
    want = engine.nearest_to_numpy(engine.nearest_exhaustive(c["scene"].arrays(), points))
    near = engine.nearest_to_numpy(renderer.query_nearest(points))
    assert np.array_equal(near["dst"].view(np.uint32), want["dst"].view(np.uint32)) and np.array_equal(near["found"], want["found"])


@pytest.mark.gpu
def test_empty_batch_and_refusals_through_the_c_abi(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    none = np.zeros((0, 3), np.float32)
    recs, counts = renderer.query_boxes(none, none, 8)
    assert len(recs) == 0 and len(counts) == 0
    l, h = renderer._l, renderer._h
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    po, pc = to_device(renderer, "b_out", guard), to_device(renderer, "b_counts", guard)
    blo, bhi = (a[:16].copy() for a in _boxes("cornell", "uniform"))
    pl, ph = to_device(renderer, "b_lo", blo), to_device(renderer, "b_hi", bhi)
    empty = _capi.RtBoxBatch(None, None, 0)
    assert l.rt_query_boxes(h, C.byref(empty), 99, None, None) == 0 and l.rt_query_boxes_host(h, C.byref(empty), 99, None, None) == 0
    for fn in ("rt_query_boxes", "rt_query_boxes_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host, cnt_host = (_capi.RtOverlap * (16 * 8))(), (C.c_uint32 * 16)()
        out, cnt = (C.addressof(out_host), C.addressof(cnt_host)) if host else (po, pc)
        lo_, hi_ = (blo.ctypes.data, bhi.ctypes.data) if host else (pl, ph)
        ok = _capi.RtBoxBatch(lo_, hi_, 5)
        big = _capi.RtBoxBatch(lo_, hi_, 1 << 30)
        for batch, k, o, cn, message in ((None, 8, out, cnt, "the batch is NULL"),
                                         (_capi.RtBoxBatch(None, hi_, 5), 8, out, cnt, "lo and hi are required"),
                                         (_capi.RtBoxBatch(lo_, None, 5), 8, out, cnt, "lo and hi are required"),
                                         (ok, 9, out, cnt, "k = 9 is above RT_BOXES_MAX_K = 8"),
                                         (ok, 8, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 0, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 1, None, cnt, "counts and, with k > 0, the output are required"),
                                         (big, 8, out, cnt, "a batch of 1073741824 boxes does not fit the 30 bits of a slot id"),
                                         (_capi.RtBoxBatch(None, None, 1 << 30), 9, None, None, "lo and hi are required"),   # the order
                                         (big, 9, None, None, "k = 9 is above RT_BOXES_MAX_K = 8"),
                                         (big, 8, None, cnt, "counts and, with k > 0, the output are required")):
            assert call(h, C.byref(batch) if batch is not None else None, k, o, cn) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {message}", l.rt_last_error(h).decode()
        assert not np.frombuffer(out_host, np.uint8).any() and not np.frombuffer(cnt_host, np.uint8).any()
    renderer.sync()
    for name in ("b_out", "b_counts"):
        renderer._owned[name].download(into=guard)
        assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        b = _capi.RtBoxBatch(pl, ph, 16)
        assert fresh._l.rt_query_boxes(fresh._h, C.byref(b), 8, po, pc) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_boxes before rt_upload_scene"
        assert fresh._l.rt_query_boxes_host(fresh._h, None, 8, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_boxes_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_boxes(blo, bhi[:5], 2)
    with pytest.raises(engine.RtError, match="RT_BOXES_MAX_K"):
        renderer.query_boxes(blo[:4], bhi[:4], 9)
    with pytest.raises(ValueError):
        renderer.query_boxes(1 << 20, 1 << 22, 2, n=4, out=1 << 21)    # a device pointer without counts=
    with pytest.raises(ValueError):
        renderer.query_boxes(1 << 20, 1 << 22, 2, n=4, counts=1 << 21)   # k > 0 without out=
