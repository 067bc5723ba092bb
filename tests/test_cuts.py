"""Cut queries on the GPU (rt_query_cuts, rt_query_cuts_host; Renderer.query_cuts, Renderer.query_mesh_cuts; DESIGN.md, "Triangle
cuts"): the segments along which a closed query triangle crosses the scene's triangles, the first k in index order, and the count.

The contract (include/rt_amd.h, include/rt_tri_cut.h): the cut of a pair is a function of the pair and the member set of a query a
function of its corners and the scene alone, under a total key, so the device (its own node numbering, the triangle query's
descent with both prunings, the two instantiations of k_tris_cut, the kept cuts computed a second time after the search) must
give what the exhaustive host loop over the host arrays gives (rt_cuts_exhaustive_host; engine.cuts_exhaustive), bit for bit:
every byte of every 48-byte record and every count, for every k. The loop itself is held to a float64 reference on the CPU
(tests/test_cuts_host.py). The scenes are tests/point_query_cases.py's, the queries tests/cut_float64.py's seeded ones."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import cut_float64 as cf
import point_query_cases as pq
from util import _deformed_bunny, _mesh_triangles, kernel_instantiations, model_scene, to_device

KS = (0, 1, 2, 8)
REC = C.sizeof(_capi.RtCut)
TREC = C.sizeof(_capi.RtOverlap)
SHALLOW, DEEP = "k_tris_cut<24, false>", "k_tris_cut<64, true>"
GUARD = 64

_wants = {}


def _queries(name, key):
    return cf.seed_corners(name, key)


def _raw(recs, n, k):
    return np.frombuffer(recs, np.uint8).reshape(n, k, REC) if n * k else np.zeros((n, k, REC), np.uint8)


def _loop(arrays, corners, k):
    recs, counts = engine.cuts_exhaustive(arrays, corners, k)
    return _raw(recs, len(counts), k).copy(), counts


def _want(name, key, k):
    """The exhaustive loop's answer, once per session: (bytes [n, k, 48], counts)."""
    if (name, key, k) not in _wants:
        _wants[(name, key, k)] = _loop(pq.case(name)["scene"].arrays(), _queries(name, key), k)
    return _wants[(name, key, k)]


def _device(renderer, corners, k, triangles=False):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own with GUARD bytes before and
    after the records and the counts: (bytes [n, k, record], counts, the kernel that ran, the guards of the records (before,
    after), the guards of the counts). triangles: rt_query_triangles instead, over the same path."""
    n, rec = len(corners), TREC if triangles else REC
    renderer.sync()
    pq_ = to_device(renderer, "c_corners", corners)
    out = np.full(GUARD + n * k * rec + GUARD, 0xA5, np.uint8)
    cnt = np.full(GUARD + n * 4 + GUARD, 0xA5, np.uint8)
    po, pc = to_device(renderer, "c_out", out), to_device(renderer, "c_counts", cnt)
    ask = renderer.query_triangles if triangles else renderer.query_cuts
    assert ask(pq_, k, n=n, out=po + GUARD if k else None, counts=pc + GUARD, sync=False) is None
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["c_out"].download(into=out)
    renderer._owned["c_counts"].download(into=cnt)
    guards = (out[:GUARD], out[GUARD + n * k * rec:], cnt[:GUARD], cnt[GUARD + n * 4:])
    return out[GUARD:GUARD + n * k * rec].reshape(n, k, rec), cnt[GUARD:GUARD + n * 4].view(np.uint32).copy(), kernel, guards


def _assert_equal(got, want, what):
    (gb, gc), (wb, wc) = got, want
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.flatnonzero(gc != wc)[:5].tolist()}"
    assert np.array_equal(gb, wb), f"{what}: records differ at queries {np.unique(np.argwhere(gb != wb)[:, 0])[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_device_equals_the_exhaustive_loop(renderer, name):
    """All bytes of all records and all counts, on every query set, k in {0, 1, 2, 8}; the _host form; and never more cuts than
    the triangle query has members."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    for key in c["sets"]:
        q = _queries(name, key)
        n = len(q)
        for k in KS:
            wb, wc = _want(name, key, k)
            what = f"{name}/{key}/k={k}"
            gb, gc, kernel, _ = _device(renderer, q, k)
            assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
            _assert_equal((gb, gc), (wb, wc), what)
            hr, hc = renderer.query_cuts(q, k)
            _assert_equal((_raw(hr, n, k), hc), (gb, gc), what + " / host form")
        _, tc = renderer.query_triangles(q, 0)
        assert (wc <= tc).all(), f"{name}/{key}: more cuts than members of the triangle query"
        print(f"{name:14s} {key:9s} {n} queries, {int(wc.sum())} cuts, the most {int(wc.max())}; {int(tc.sum())} members of the triangle query")


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_the_plane_pruning_changes_no_byte_and_the_descent_is_the_triangle_querys(renderer, name):
    """With "tri_plane" 0 the descent prunes by boxes alone: the same bytes. And with either setting the boxTests and triTests the
    query adds are exactly what rt_query_triangles adds over the same batch: it is the same descent."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    try:
        for key in c["sets"]:
            q = _queries(name, key)
            added = {}
            for plane in (1, 0):
                renderer.set_tuning("tri_plane", plane)
                for what in ("cuts", "triangles"):
                    renderer.sync()
                    before = renderer.counters()
                    gb, gc, _, _ = _device(renderer, q, 8, triangles=what == "triangles")
                    after = renderer.counters()
                    if what == "cuts":
                        _assert_equal((gb, gc), _want(name, key, 8), f"{name}/{key}/tri_plane {plane}")
                    added[(what, plane)] = {x: after[x] - before[x] for x in ("boxTests", "triTests", "raysTraced", "raysHit")}
                    if what == "cuts":
                        assert added[(what, plane)]["raysHit"] == int((gc > 0).sum())
                for x in ("boxTests", "triTests", "raysTraced"):
                    assert added[("cuts", plane)][x] == added[("triangles", plane)][x], (name, key, plane, x, added)
                assert added[("cuts", plane)]["raysTraced"] == len(q)
            assert added[("cuts", 1)]["boxTests"] <= added[("cuts", 0)]["boxTests"]
    finally:
        renderer.set_tuning("tri_plane", 1)


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_tris_cut") == {SHALLOW, DEEP}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n queries alone equal their rows of the whole set, and the 64 bytes before and
    behind the records and the counts are left as they were."""
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    q = _queries("cornell", "uniform")[:n].copy()
    for k in (1, 8):
        wb, wc = _want("cornell", "uniform", k)
        gb, gc, kernel, guards = _device(renderer, q, k)
        assert kernel == SHALLOW
        _assert_equal((gb, gc), (wb[:n], wc[:n]), f"n = {n}, k = {k}")
        assert all((g == 0xA5).all() for g in guards), f"n = {n}, k = {k}: bytes around the batch's outputs were written"
        hr, hc = renderer.query_cuts(q, k)
        _assert_equal((_raw(hr, n, k), hc), (gb, gc), f"n = {n}, k = {k} / host form")


@pytest.mark.gpu
def test_invalid_triangles_are_not_searched(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    q = _queries("cornell", "surface")[:200].copy()
    bad = np.arange(200) % 5 == 3
    which = np.arange(int(bad.sum())) % 3
    rows = np.flatnonzero(bad)
    q[rows, (7 * np.arange(len(rows))) % 9] = np.choose(which, [np.nan, np.inf, -np.inf]).astype(np.float32)
    for k in (0, 8):
        renderer.sync()
        before = renderer.counters()
        gb, gc, _, _ = _device(renderer, q, k)
        after = renderer.counters()
        assert not gc[bad].any() and not gb[bad].any()
        assert gc[~bad].any()
        assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
        assert after["raysHit"] - before["raysHit"] == int((gc > 0).sum())
        _assert_equal((gb, gc), _loop(c["scene"].arrays(), q, k), f"invalid triangles, k = {k}")


@pytest.mark.gpu
def test_degenerate_queries_on_cornell(renderer):
    """Queries with two and with three equal corners (segments between mesh vertices, points on them): no normal, coplanar with
    everything, count 0 and empty records whatever they touch; and the walls' own triangles as queries, coplanar with what they
    were made from and cutting the walls beside it. Every one is held to the loop byte for byte."""
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    a = c["scene"].arrays()
    plain = np.array([all(abs(a.objects[i].transformMatrix[col * 4 + r]) in (0.0, 1.0) for col in range(3) for r in range(3)) for i in range(a.objectCount)])
    walls = c["ns"].W.astype(np.float32)[plain[c["ns"].obj]]
    assert len(walls) >= 10, "the Cornell box has no walls?"
    v = c["sets"]["vertices"]
    points = np.concatenate([np.tile(v, (1, 3)), np.tile(walls.reshape(-1, 3), (1, 3))])
    segments = np.concatenate([v[:-1], v[:-1], v[1:]], axis=1)
    q = np.concatenate([walls.reshape(-1, 9), points, segments]).astype(np.float32)
    for k in (0, 8):
        gb, gc, _, _ = _device(renderer, q, k)
        _assert_equal((gb, gc), _loop(a, q, k), f"degenerate queries, k = {k}")
        assert not gc[len(walls):].any() and not gb[len(walls):].any(), "a query without a normal has a cut"
    _, tc = renderer.query_triangles(q, 0)
    assert (tc[len(walls):len(walls) + len(points)] >= 1).sum() >= len(walls), "the points touch nothing: the case shows nothing"
    assert gc[:len(walls)].any(), "no wall triangle cuts a wall beside it"


def _bunny():
    s = model_scene("bunny.obj")
    faces = _mesh_triangles(s, s.counts()["objects"] - 1)
    points = s.points()[:, :3].copy()
    m = np.array([0.5, 0.0, -0.2, 0.0, 0.35, 0.8, 0.0, 0.0, 0.0, 0.1, 0.6, 0.0, 0.15, 0.4, -0.1, 1.0], np.float32)   # column-major: scale, shear, translation
    return points, faces, m


@pytest.mark.gpu
def test_query_mesh_cuts_equals_query_cuts_over_the_host_corners(renderer):
    """The 908-triangle bunny under a scaled and sheared matrix, placed against cornell_bunny."""
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    points, faces, m = _bunny()
    assert len(faces) == 908
    corners = engine.mesh_corners(points, faces, m)
    for k in (0, 8):
        recs, counts = renderer.query_mesh_cuts(points, faces, k, matrix=m)
        hr, hc = renderer.query_cuts(corners, k)
        _assert_equal((_raw(recs, 908, k), counts), (_raw(hr, 908, k), hc), f"query_mesh_cuts, k = {k}")
        _assert_equal((_raw(recs, 908, k), counts), _loop(c["scene"].arrays(), corners, k), f"query_mesh_cuts against the loop, k = {k}")
    assert (counts > 0).any() and (counts == 0).any()
    recs, counts = renderer.query_mesh_cuts(points, faces, 2)
    _assert_equal((_raw(recs, 908, 2), counts), _loop(c["scene"].arrays(), points[faces].reshape(-1, 9), 2), "query_mesh_cuts without a matrix")


@pytest.mark.gpu
def test_query_mesh_cuts_on_torch_tensors(renderer):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    points, faces, m = _bunny()
    dev = torch.device("cuda:0")
    tp, tfc = torch.from_numpy(points).to(dev), torch.from_numpy(faces.astype(np.int64)).to(dev)
    corners = engine.mesh_corners(points, faces, m)
    for k in (0, 8):
        rec, cnt = renderer.query_mesh_cuts(tp, tfc, k, matrix=m)
        wb, wc = _loop(c["scene"].arrays(), corners, k)
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), wc)
        assert np.array_equal(rec.cpu().numpy().view(np.uint32).reshape(908, k, 12), wb.copy().view(np.uint32).reshape(908, k, 12))


@pytest.mark.gpu
def test_after_update_objects_the_answers_follow_the_moved_object(renderer):
    e = pq.build_scene("instances")
    renderer.upload_scene(e)
    q = np.concatenate([_queries("instances", "surface"), _queries("instances", "uniform")])
    before, cb, _, _ = _device(renderer, q, 8)
    wb, counts_before = _loop(e.arrays(), q, 8)
    _assert_equal((before, cb), (wb, counts_before), "instances before the move")
    e.set_transform(1, engine.placement(position=(0.2, -0.4, 0.5), rotation=(15, -40, 70), scale=(0.8, 1.3, 0.5)))
    e.push(renderer, "objects")
    after, ca, kernel, _ = _device(renderer, q, 8)
    assert kernel == SHALLOW
    wa, counts_after = _loop(e.arrays(), q, 8)
    assert (counts_after != counts_before).any(), "the move does not change the reference: the test shows nothing"
    _assert_equal((after, ca), (wa, counts_after), "instances after the move")


@pytest.mark.gpu
def test_after_update_points_the_answers_follow_the_refit(renderer):
    scene, p, first = _deformed_bunny()
    renderer.upload_scene(scene, dynamic=True)
    rng = np.random.default_rng(79)
    centre = rng.uniform(-1.0, 1.0, (1024, 1, 3))
    centre[:, :, 1] -= 0.3
    q = (centre + rng.uniform(0.02, 0.4, (1024, 1, 1)) * rng.normal(size=(1024, 3, 3))).reshape(-1, 9).astype(np.float32)
    wb, counts_before = _loop(scene.arrays(), q, 8)
    gb, gc, _, _ = _device(renderer, q, 8)
    _assert_equal((gb, gc), (wb, counts_before), "before the deformation")
    renderer.update_points(p, first)
    scene.update_points(p, first)
    wb, counts_after = _loop(scene.arrays(), q, 8)
    assert (counts_after != counts_before).any() or not np.array_equal(wb, gb), "the deformation does not change the reference: the test shows nothing"
    gb, gc, _, _ = _device(renderer, q, 8)
    _assert_equal((gb, gc), (wb, counts_after), "after the deformation")


@pytest.mark.gpu
def test_a_cut_query_leaves_rendering_and_the_triangle_query_alone(renderer):
    """After a pass, rt_render of the golden Cornell frame is bit-identical to one rendered before it, and rt_query_triangles gives
    the bytes it gave before; last_pipeline, last_parts and the ray cost are unchanged; only the four counters the pass declares
    have moved."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_c1_64x64_4spp.npz"), allow_pickle=False)
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    pc = engine.push_constants(64, 64, singleRender=1, sampleLimit=4)
    before = renderer.render(pc, 64, 64)
    assert np.array_equal(before.view(np.uint32), z["rgba"].view(np.uint32))
    q = _queries("cornell", "vertices")
    tr_before, tc_before = renderer.query_triangles(q, 8)
    tr_before = bytes(tr_before)
    want_t, want_tc = engine.tris_exhaustive(c["scene"].arrays(), q, 8)
    assert tr_before == bytes(want_t) and np.array_equal(tc_before, want_tc)
    state = (renderer.last_pipeline(), renderer.last_parts())
    renderer.reset_counters()
    zero = renderer.counters()
    cost = renderer.ray_cost()
    recs, counts = renderer.query_cuts(q, 8)
    assert renderer.last_kernel() == SHALLOW
    sq = _queries("cornell", "surface")
    _, sc, _, _ = _device(renderer, sq, 2)
    assert renderer.ray_cost() == cost
    got = renderer.counters()
    assert got["raysTraced"] - zero["raysTraced"] == len(q) + len(sq)
    assert got["raysHit"] - zero["raysHit"] == int((counts > 0).sum()) + int((sc > 0).sum())
    assert got["boxTests"] > zero["boxTests"] and got["triTests"] > zero["triTests"]
    for key in got:
        if key not in ("boxTests", "triTests", "raysTraced", "raysHit"):
            assert got[key] == zero[key], key
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state
    tr_after, tc_after = renderer.query_triangles(q, 8)
    assert bytes(tr_after) == tr_before and np.array_equal(tc_after, tc_before)


@pytest.mark.gpu
def test_empty_batch_and_refusals_through_the_c_abi(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    recs, counts = renderer.query_cuts(np.zeros((0, 9), np.float32), 8)
    assert len(recs) == 0 and len(counts) == 0
    l, h = renderer._l, renderer._h
    guard = np.full(8192, 0x5A, np.uint8)
    renderer.sync()
    po, pc = to_device(renderer, "c_out", guard), to_device(renderer, "c_counts", guard)
    q = _queries("cornell", "uniform")[:16].copy()
    pq_ = to_device(renderer, "c_corners", q)
    empty = _capi.RtTriangleBatch(None, 0)
    assert l.rt_query_cuts(h, C.byref(empty), 99, None, None) == 0 and l.rt_query_cuts_host(h, C.byref(empty), 99, None, None) == 0
    for fn in ("rt_query_cuts", "rt_query_cuts_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host, cnt_host = (_capi.RtCut * (16 * 8))(), (C.c_uint32 * 16)()
        out, cnt = (C.addressof(out_host), C.addressof(cnt_host)) if host else (po, pc)
        corners = q.ctypes.data if host else pq_
        ok = _capi.RtTriangleBatch(corners, 5)
        big = _capi.RtTriangleBatch(corners, 1 << 30)
        for batch, k, o, cn, message in ((None, 8, out, cnt, "the batch is NULL"),
                                         (_capi.RtTriangleBatch(None, 5), 8, out, cnt, "corners are required"),
                                         (ok, 9, out, cnt, "k = 9 is above RT_BOXES_MAX_K = 8"),
                                         (ok, 8, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 0, out, None, "counts and, with k > 0, the output are required"),
                                         (ok, 1, None, cnt, "counts and, with k > 0, the output are required"),
                                         (big, 8, out, cnt, "a batch of 1073741824 triangles does not fit the 30 bits of a slot id"),
                                         (_capi.RtTriangleBatch(None, 1 << 30), 9, None, None, "corners are required"),   # the order
                                         (big, 9, None, None, "k = 9 is above RT_BOXES_MAX_K = 8"),
                                         (big, 8, None, cnt, "counts and, with k > 0, the output are required")):
            assert call(h, C.byref(batch) if batch is not None else None, k, o, cn) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {message}", l.rt_last_error(h).decode()
        assert not np.frombuffer(out_host, np.uint8).any() and not np.frombuffer(cnt_host, np.uint8).any()
    renderer.sync()
    for name in ("c_out", "c_counts"):
        renderer._owned[name].download(into=guard)
        assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        b = _capi.RtTriangleBatch(pq_, 16)
        assert fresh._l.rt_query_cuts(fresh._h, C.byref(b), 8, po, pc) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_cuts before rt_upload_scene"
        assert fresh._l.rt_query_cuts_host(fresh._h, None, 8, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_cuts_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_cuts(q.reshape(-1)[:10], 2)
    with pytest.raises(engine.RtError, match="RT_BOXES_MAX_K"):
        renderer.query_cuts(q[:4], 9)
    with pytest.raises(ValueError):
        renderer.query_cuts(1 << 20, 2, n=4, out=1 << 21)    # a device pointer without counts=
    with pytest.raises(ValueError):
        renderer.query_cuts(1 << 20, 2, n=4, counts=1 << 21)   # k > 0 without out=
    with pytest.raises(ValueError):
        renderer.query_cuts(1 << 20, 0, counts=1 << 21)   # an integer pointer without n=


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["torus", "cubes"])
def test_cuts_of_a_closed_mesh_close(renderer, name):
    scene, q = cf.closure_queries(name)
    renderer.upload_scene(scene)
    recs, counts = renderer.query_cuts(q, 8)
    _assert_equal((_raw(recs, len(q), 8), counts), _loop(scene.arrays(), q, 8), f"closure queries on {name}")
    looked, shared = cf.check_closure(engine.cuts_to_numpy(recs).reshape(len(q), 8), counts)
    print(f"{name}: {looked} queries with 1 to 8 cuts, {shared} ends shared along scene edges")
    assert looked >= 100 and shared >= 100
