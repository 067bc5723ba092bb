"""Triangle queries on the GPU (rt_query_triangles, rt_query_triangles_host; Renderer.query_triangles, Renderer.query_mesh;
DESIGN.md, "Triangle queries"): every surface a closed query triangle touches, the first k in index order, and the count.

The contract (include/rt_amd.h, include/rt_tri_overlap.h): the member set of a query is a function of its corners and the scene
alone and the key that orders it is total, so the device (its own node numbering, its descent pruned by boxes and by the query's
plane, the two instantiations of k_tris_overlap) must give what the exhaustive host loop over the host arrays gives
(rt_tris_exhaustive_host; engine.tris_exhaustive), bit for bit: every byte of every record and every count, for every k. The loop
itself is held to a float64 reference on the CPU (tests/test_triangles_host.py). The scenes are tests/point_query_cases.py's, the
queries tests/tri_overlap_float64.py's seeded ones: about 1.6 k a scene, around the points of its four sets."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import point_query_cases as pq
import tri_overlap_float64 as tf
from util import _deformed_bunny, _mesh_triangles, kernel_instantiations, model_scene, to_device

KS = (0, 1, 2, 8)
REC = C.sizeof(_capi.RtOverlap)
SHALLOW, DEEP = "k_tris_overlap<24, false>", "k_tris_overlap<64, true>"

_wants = {}


def _queries(name, key):
    return tf.seed_corners(name, key)


def _raw(recs, n, k):
    return np.frombuffer(recs, np.uint8).reshape(n, k, REC) if n * k else np.zeros((n, k, REC), np.uint8)


def _loop(arrays, corners, k):
    recs, counts = engine.tris_exhaustive(arrays, corners, k)
    return _raw(recs, len(counts), k).copy(), counts


def _want(name, key, k):
    """The exhaustive loop's answer, once per session: (bytes [n, k, 16], counts)."""
    if (name, key, k) not in _wants:
        _wants[(name, key, k)] = _loop(pq.case(name)["scene"].arrays(), _queries(name, key), k)
    return _wants[(name, key, k)]


def _device(renderer, corners, k, guard=0):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own: (bytes [n, k, 16], counts, the
    kernel that ran, the `guard` bytes behind the records, the `guard` bytes behind the counts)."""
    n = len(corners)
    renderer.sync()
    pq_ = to_device(renderer, "t_corners", corners)
    out = np.full(n * k * REC + guard, 0xA5, np.uint8)
    cnt = np.full(n * 4 + guard, 0xA5, np.uint8)
    po, pc = to_device(renderer, "t_out", out), to_device(renderer, "t_counts", cnt)
    assert renderer.query_triangles(pq_, k, n=n, out=po if k else None, counts=pc, sync=False) is None
    kernel = renderer.last_kernel()
    renderer.sync()
    renderer._owned["t_out"].download(into=out)
    renderer._owned["t_counts"].download(into=cnt)
    return out[:n * k * REC].reshape(n, k, REC), cnt[:n * 4].view(np.uint32).copy(), kernel, out[n * k * REC:], cnt[n * 4:]


def _device_boxes(renderer, lo, hi, k):
    """rt_query_boxes over the same device path, for the counters."""
    n = len(lo)
    renderer.sync()
    pl, ph = to_device(renderer, "t_lo", lo), to_device(renderer, "t_hi", hi)
    po, pc = renderer._device_buffer("t_bout", max(n * k * REC, 1)), renderer._device_buffer("t_bcounts", n * 4)
    renderer.query_boxes(pl, ph, k, n=n, out=po if k else None, counts=pc, sync=True)


def _assert_equal(got, want, what):
    (gb, gc), (wb, wc) = got, want
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.flatnonzero(gc != wc)[:5].tolist()}"
    assert np.array_equal(gb, wb), f"{what}: records differ at queries {np.unique(np.argwhere(gb != wb)[:, 0])[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_device_equals_the_exhaustive_loop(renderer, name):
    """All bytes of all records and all counts, on every query set, k in {0, 1, 2, 8}; and the _host form."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    most = 0
    for key in c["sets"]:
        q = _queries(name, key)
        n = len(q)
        for k in KS:
            wb, wc = _want(name, key, k)
            what = f"{name}/{key}/k={k}"
            gb, gc, kernel, _, _ = _device(renderer, q, k)
            assert kernel == (DEEP if name == "deep" else SHALLOW), (what, kernel)
            _assert_equal((gb, gc), (wb, wc), what)
            hr, hc = renderer.query_triangles(q, k)
            _assert_equal((_raw(hr, n, k), hc), (gb, gc), what + " / host form")
            most = max(most, int(wc.max()))
    surfaces = len(c["ns"].sph_c) + len(c["ns"].W)
    assert most > 8 or surfaces <= 8, f"{name}: no query has more members than slots"


@pytest.mark.gpu
@pytest.mark.parametrize("name", pq.SCENES)
def test_the_plane_pruning_changes_no_byte_and_no_descent_visits_more_than_the_box_query(renderer, name):
    """With "tri_plane" 0 the descent prunes by boxes alone: the same bytes. And on every set the boxTests and triTests the query
    adds are at most what rt_query_boxes adds over the queries' own boxes (the exact min / max of the corners): the same descent,
    which can only have discarded more; without the plane the two descents are the same and the counters are equal."""
    c = pq.case(name)
    renderer.upload_scene(c["scene"])
    try:
        for key in c["sets"]:
            q = _queries(name, key)
            tri = q.reshape(-1, 3, 3)
            lo, hi = tri.min(axis=1).copy(), tri.max(axis=1).copy()
            added = {}
            for what in ("boxes", "plane", "no plane"):
                renderer.set_tuning("tri_plane", 0 if what == "no plane" else 1)
                renderer.sync()
                before = renderer.counters()
                if what == "boxes":
                    _device_boxes(renderer, lo, hi, 8)
                else:
                    gb, gc, _, _, _ = _device(renderer, q, 8)
                    _assert_equal((gb, gc), _want(name, key, 8), f"{name}/{key}/{what}")
                after = renderer.counters()
                added[what] = {x: after[x] - before[x] for x in ("boxTests", "triTests", "raysTraced")}
            print(f"{name:14s} {key:9s} box tests: boxes {added['boxes']['boxTests']}, triangles {added['plane']['boxTests']} (without the plane {added['no plane']['boxTests']}); "
                  f"triangle tests: {added['boxes']['triTests']}, {added['plane']['triTests']} ({added['no plane']['triTests']})")
            assert added["plane"]["raysTraced"] == added["boxes"]["raysTraced"] == len(q)
            for x in ("boxTests", "triTests"):
                assert added["plane"][x] <= added["no plane"][x] == added["boxes"][x], (name, key, x, added)
    finally:
        renderer.set_tuning("tri_plane", 1)


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_tris_overlap") == {SHALLOW, DEEP}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n queries alone equal their rows of the whole set, and the 64 bytes behind the
    records and behind the counts are left as they were."""
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    q = _queries("cornell", "uniform")[:n].copy()
    for k in (1, 8):
        wb, wc = _want("cornell", "uniform", k)
        gb, gc, kernel, g_out, g_cnt = _device(renderer, q, k, guard=64)
        assert kernel == SHALLOW
        _assert_equal((gb, gc), (wb[:n], wc[:n]), f"n = {n}, k = {k}")
        assert (g_out == 0xA5).all() and (g_cnt == 0xA5).all(), f"n = {n}, k = {k}: bytes behind the batch's outputs were written"
        hr, hc = renderer.query_triangles(q, k)
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
        gb, gc, _, _, _ = _device(renderer, q, k)
        after = renderer.counters()
        assert not gc[bad].any() and not gb[bad].any()
        assert (gc[~bad] >= 1).all()
        assert after["raysTraced"] - before["raysTraced"] == int((~bad).sum())
        assert after["raysHit"] - before["raysHit"] == int((~bad).sum())
        _assert_equal((gb, gc), _loop(c["scene"].arrays(), q, k), f"invalid triangles, k = {k}")


@pytest.mark.gpu
def test_degenerate_queries_on_cornell(renderer):
    """Queries with two and with three equal corners (segments between mesh vertices, points on them) and the walls' own triangles
    as queries, coplanar with what they are asked about: where an over-eager prune would lose a member. Every one is held to the
    loop byte for byte; a wall's own triangle and a point on a wall's vertex must touch the triangle they were made from."""
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
        gb, gc, _, _, _ = _device(renderer, q, k)
        _assert_equal((gb, gc), _loop(a, q, k), f"degenerate queries, k = {k}")
    made = gc[:len(walls)]
    assert (made >= 1).all(), "a wall's own triangle touches nothing"
    on_corner = gc[len(walls) + len(v):len(walls) + len(v) + 3 * len(walls)]
    assert (on_corner >= 1).all(), "a point on a wall's corner touches nothing"


@pytest.mark.gpu
def test_query_mesh_equals_query_triangles_over_the_host_corners(renderer):
    """The 908-triangle bunny under a scaled and sheared matrix, placed against cornell_bunny: the faces' counts and records are
    query_triangles' over the corners computed on the host, which are the loop's."""
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    s = model_scene("bunny.obj")
    faces = _mesh_triangles(s, s.counts()["objects"] - 1)
    points = s.points()[:, :3].copy()
    assert len(faces) == 908
    m = np.array([0.5, 0.0, -0.2, 0.0, 0.35, 0.8, 0.0, 0.0, 0.0, 0.1, 0.6, 0.0, 0.15, 0.4, -0.1, 1.0], np.float32)   # column-major: scale, shear, translation
    corners = engine.mesh_corners(points, faces, m)
    assert corners.shape == (908, 9)
    for k in (0, 8):
        recs, counts = renderer.query_mesh(points, faces, k, matrix=m)
        hr, hc = renderer.query_triangles(corners, k)
        _assert_equal((_raw(recs, 908, k), counts), (_raw(hr, 908, k), hc), f"query_mesh, k = {k}")
        _assert_equal((_raw(recs, 908, k), counts), _loop(c["scene"].arrays(), corners, k), f"query_mesh against the loop, k = {k}")
    assert (counts > 0).any() and (counts == 0).any()
    # without a matrix the mesh lies where the scene's own bunny does not (the scene places it): the gather alone
    recs, counts = renderer.query_mesh(points, faces, 2)
    _assert_equal((_raw(recs, 908, 2), counts), _loop(c["scene"].arrays(), points[faces].reshape(-1, 9), 2), "query_mesh without a matrix")


@pytest.mark.gpu
def test_query_mesh_on_torch_tensors(renderer):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    c = pq.case("cornell_bunny")
    renderer.upload_scene(c["scene"])
    s = model_scene("bunny.obj")
    faces = _mesh_triangles(s, s.counts()["objects"] - 1)
    points = s.points()[:, :3].copy()
    m = np.array([0.5, 0.0, -0.2, 0.0, 0.35, 0.8, 0.0, 0.0, 0.0, 0.1, 0.6, 0.0, 0.15, 0.4, -0.1, 1.0], np.float32)
    dev = torch.device("cuda:0")
    tp, tfc = torch.from_numpy(points).to(dev), torch.from_numpy(faces.astype(np.int64)).to(dev)
    corners = engine.mesh_corners(points, faces, m)
    assert np.array_equal(engine.mesh_corners(tp, tfc, m).cpu().numpy(), corners), "the device gather is not the host's"
    for k in (0, 8):
        rec, cnt = renderer.query_mesh(tp, tfc, k, matrix=m)
        wb, wc = _loop(c["scene"].arrays(), corners, k)
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), wc)
        assert np.array_equal(rec.cpu().numpy().view(np.uint32).reshape(908, k, 4), wb.copy().view(np.uint32).reshape(908, k, 4))


@pytest.mark.gpu
def test_after_update_objects_the_answers_follow_the_moved_object(renderer):
    """The reference is the exhaustive loop over the host arrays before and after the move: its own answers change, and the device
    equals it each time, so the device read the moved tables."""
    e = pq.build_scene("instances")
    renderer.upload_scene(e)
    q = np.concatenate([_queries("instances", "surface"), _queries("instances", "uniform")])
    before, cb, _, _, _ = _device(renderer, q, 8)
    wb, counts_before = _loop(e.arrays(), q, 8)
    _assert_equal((before, cb), (wb, counts_before), "instances before the move")
    e.set_transform(1, engine.placement(position=(0.2, -0.4, 0.5), rotation=(15, -40, 70), scale=(0.8, 1.3, 0.5)))
    e.push(renderer, "objects")
    after, ca, kernel, _, _ = _device(renderer, q, 8)
    assert kernel == SHALLOW
    wa, counts_after = _loop(e.arrays(), q, 8)
    print(f"the move changes the reference's count on {int((counts_after != counts_before).sum())} of {len(q)} queries")
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
    _, counts_before = _loop(scene.arrays(), q, 8)
    gb, gc, _, _, _ = _device(renderer, q, 8)
    _assert_equal((gb, gc), _loop(scene.arrays(), q, 8), "before the deformation")
    renderer.update_points(p, first)
    scene.update_points(p, first)
    wb, counts_after = _loop(scene.arrays(), q, 8)
    assert (counts_after != counts_before).any(), "the deformation does not change the reference: the test shows nothing"
    gb, gc, _, _, _ = _device(renderer, q, 8)
    _assert_equal((gb, gc), (wb, counts_after), "after the deformation")


@pytest.mark.gpu
def test_a_triangle_query_leaves_rendering_alone(renderer):
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
    q = _queries("cornell", "vertices")
    recs, counts = renderer.query_triangles(q, 8)
    assert renderer.last_kernel() == SHALLOW
    sq = _queries("cornell", "surface")
    _, sc, _, _, _ = _device(renderer, sq, 2)
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
    # and the box query after it is what it was
    tri = q.reshape(-1, 3, 3)
    lo, hi = tri.min(axis=1).copy(), tri.max(axis=1).copy()
    hr, hc = renderer.query_boxes(lo, hi, 8)
    wr, wc = engine.boxes_exhaustive(c["scene"].arrays(), lo, hi, 8)
    assert np.array_equal(hc, wc) and bytes(hr) == bytes(wr)


@pytest.mark.gpu
def test_empty_batch_and_refusals_through_the_c_abi(renderer):
    c = pq.case("cornell")
    renderer.upload_scene(c["scene"])
    recs, counts = renderer.query_triangles(np.zeros((0, 9), np.float32), 8)
    assert len(recs) == 0 and len(counts) == 0
    l, h = renderer._l, renderer._h
    guard = np.full(4096, 0x5A, np.uint8)
    renderer.sync()
    po, pc = to_device(renderer, "t_out", guard), to_device(renderer, "t_counts", guard)
    q = _queries("cornell", "uniform")[:16].copy()
    pq_ = to_device(renderer, "t_corners", q)
    empty = _capi.RtTriangleBatch(None, 0)
    assert l.rt_query_triangles(h, C.byref(empty), 99, None, None) == 0 and l.rt_query_triangles_host(h, C.byref(empty), 99, None, None) == 0
    for fn in ("rt_query_triangles", "rt_query_triangles_host"):
        call = getattr(l, fn)
        host = fn.endswith("_host")
        out_host, cnt_host = (_capi.RtOverlap * (16 * 8))(), (C.c_uint32 * 16)()
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
    for name in ("t_out", "t_counts"):
        renderer._owned[name].download(into=guard)
        assert (guard == 0x5A).all(), "a refused call wrote to its output"
    fresh = engine.Renderer(renderer.device)
    try:
        b = _capi.RtTriangleBatch(pq_, 16)
        assert fresh._l.rt_query_triangles(fresh._h, C.byref(b), 8, po, pc) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_triangles before rt_upload_scene"
        assert fresh._l.rt_query_triangles_host(fresh._h, None, 8, None, None) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_triangles_host before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_triangles(q.reshape(-1)[:10], 2)
    with pytest.raises(engine.RtError, match="RT_BOXES_MAX_K"):
        renderer.query_triangles(q[:4], 9)
    with pytest.raises(ValueError):
        renderer.query_triangles(1 << 20, 2, n=4, out=1 << 21)    # a device pointer without counts=
    with pytest.raises(ValueError):
        renderer.query_triangles(1 << 20, 2, n=4, counts=1 << 21)   # k > 0 without out=
    with pytest.raises(ValueError):
        renderer.query_triangles(1 << 20, 0, counts=1 << 21)   # an integer pointer without n=
