"""All-hit ray queries on the GPU (rt_query_hits, rt_query_hits_host; Renderer.query_hits): every surface a ray crosses below its
limit, the first k in order, and the count.

The contract (include/rt_amd.h, DESIGN.md "All-hit ray queries"): the candidate set of a ray is defined with a bound that never
shrinks, so it does not depend on the order of the visits, and the device (its own node numbering, its near-child-first descent, the
two instantiations of k_ray_hits) must give what the host walk over the host arrays gives (rt_hits_walk_host; engine.hits_walk), bit
for bit: every record and every count, for every k, with and without limits, whatever the traversal knobs say. The walk itself is
held to the oracle and to a float64 reference on the CPU (tests/test_ray_hits_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import closest_hit_cases as chf
import point_query_cases as pq
import ray_hits_cases as rh
import texture_cases as tc
from util import cornell_scene, device_buffers, kernel_instantiations, to_device

SCENES = ("cornell", "meshes", "front_only", "instances")
KS = (0, 1, 2, 8)
SHALLOW, DEEP = "k_ray_hits<24, false>", "k_ray_hits<64, true>"
REC = C.sizeof(_capi.RtHit)

_walks = {}


def _limits(name, c):
    """Per-ray limits from the walk's own unlimited lists: 0.5, 0.999, 1.001 and 2 x the second crossing's dst in turn (a random
    limit where there is none), and a few of 0, -0, -1 and NaN among them."""
    w = rh.words(*_walk(name, c, 2, None)[:1], len(c["o"]), 2)
    second = w[:, 1, 0].view(np.float32)
    rng = np.random.default_rng(77)
    T = rng.uniform(0.1, 4.0, len(second)).astype(np.float32)
    has = second < rh.MISS_DST
    T[has] = (np.resize(np.array([0.5, 0.999, 1.001, 2.0], np.float32), int(has.sum())) * second[has]).astype(np.float32)
    T[5::37] = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), len(T[5::37]))
    return T


def _walk(name, c, k, T, textures=None):
    """The host walk's answer for a case, once per session: (hits, counts). T: None, or the string "limits" for _limits."""
    key = (name, k, T is not None)
    if key not in _walks:
        lim = None if T is None else _limits(name, c)
        _walks[key] = engine.hits_walk(c["scene"].arrays(), c["o"], c["d"], k, lim, textures=textures) + (lim,)
    return _walks[key]


def _device(renderer, o, d, k, T=None):
    """The query through the device entry point, asynchronously, on buffers of the renderer's own: (words (n, k, 15), counts, kernel)."""
    n = len(o)
    renderer.sync()
    po, pd = to_device(renderer, "h_origins", o), to_device(renderer, "h_dirs", d)
    pt = None if T is None else to_device(renderer, "h_tmax", T)
    ph = renderer._device_buffer("h_hits", max(n * k, 1) * REC)
    pc = renderer._device_buffer("h_counts", max(n, 1) * 4)
    assert renderer.query_hits(po, pd, k, pt, n=n, out=ph if k else None, counts=pc, sync=False) is None
    kernel = renderer.last_kernel()
    renderer.sync()
    w = renderer._owned["h_hits"].download((n, k, 15), np.uint32) if n * k else np.zeros((n, k, 15), np.uint32)
    counts = renderer._owned["h_counts"].download(n, np.uint32) if n else np.zeros(0, np.uint32)
    return w, counts, kernel


def _assert_equal(got, want, what):
    (gw, gc), (ww, wc) = got, want
    assert np.array_equal(gc, wc), f"{what}: counts differ at {np.flatnonzero(gc != wc)[:5].tolist()}"
    assert np.array_equal(gw, ww), f"{what}: records differ at rays {np.unique(np.argwhere(gw != ww)[:, 0])[:5].tolist()}"


def _check_scene(renderer, name, c, what, ks=KS, host=False, textures=None):
    n = len(c["o"])
    for k in ks:
        for limited in (False, True):
            hits, counts, T = _walk(name, c, k, "limits" if limited else None, textures)
            want = (rh.words(hits, n, k), counts)
            w, cnt, kernel = _device(renderer, c["o"], c["d"], k, T)
            tag = f"{name} / {what} / k = {k} / {'limits' if limited else 'no limit'}"
            assert kernel == SHALLOW, (tag, kernel)
            _assert_equal((w, cnt), want, tag)
            rh.check_shape_of_lists(w, cnt, k, tag)
            if host:
                hh, hc = renderer.query_hits(c["o"], c["d"], k, T)
                _assert_equal((rh.words(hh, n, k), hc), want, tag + " / host form")


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_walk(renderer, name):
    """All records and all counts, k in {0, 1, 2, 8}, with and without limits; again under the knobs: nothing may change."""
    c = rh.case(name)
    assert ((1400 <= len(c["o"])) and (len(c["o"]) <= 5600)), len(c["o"])
    renderer.upload_scene(c["scene"])
    try:
        _check_scene(renderer, name, c, "defaults", host=True)
        assert (_walk(name, c, 8, None)[1] >= 2).sum() >= 500
        for tree_min in (0, 2):
            renderer.set_tuning("object_tree_min", tree_min)
            _check_scene(renderer, name, c, f"object_tree_min={tree_min}", ks=(8,))
        renderer.set_tuning("object_tree_min", chf.DEFAULTS["object_tree_min"])
        for knobs in chf.KNOBS:
            for key, v in knobs.items():
                renderer.set_tuning(key, v)
            _check_scene(renderer, name, c, f"{knobs}", ks=(8,))
    finally:
        for key, v in chf.DEFAULTS.items():
            renderer.set_tuning(key, v)


def test_the_kernel_names_are_instantiations_of_the_library(built):
    assert kernel_instantiations("k_ray_hits") == {SHALLOW, DEEP}
    assert kernel_instantiations("k_ray_hits_resolve") == {"k_ray_hits_resolve<256>"}


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, n):
    """The edges of the launch shape: the first n rays alone equal their rows of the whole batch, and nothing past them is written."""
    c = rh.case("meshes")
    renderer.upload_scene(c["scene"])
    o, d = c["o"][:n].copy(), c["d"][:n].copy()
    for k in (1, 8):
        hits, counts, T = _walk("meshes", c, k, "limits")
        whole = rh.words(hits, len(c["o"]), k)
        with device_buffers(["hits", "counts"], (n + 3) * k * REC, fill=7) as bufs:
            renderer.query_hits(to_device(renderer, "h_origins", o), to_device(renderer, "h_dirs", d), k, to_device(renderer, "h_tmax", T[:n].copy()),
                                n=n, out=bufs["hits"].ptr, counts=bufs["counts"].ptr)
            w = bufs["hits"].download((n + 3, k, 15), np.uint32)
            cnt = bufs["counts"].download((n + 3) * k * REC // 4, np.uint32)
        assert np.array_equal(w[:n], whole[:n]) and np.array_equal(cnt[:n], counts[:n]), (n, k)
        assert (w[n:] == 0x07070707).all() and (cnt[n:] == 0x07070707).all(), (n, k)


@pytest.mark.gpu
def test_empty_batch_writes_nothing(renderer):
    renderer.upload_scene(rh.case("meshes")["scene"])
    e = np.zeros((0, 3), np.float32)
    hits, counts = renderer.query_hits(e, e, 8)
    assert len(hits) == 0 and len(counts) == 0
    with device_buffers(["o", "d", "hits", "counts"], 4096, fill=7) as bufs:
        b = _capi.RtRayBatch(bufs["o"].ptr, bufs["d"].ptr, None, 0)
        assert renderer._l.rt_query_hits(renderer._h, C.byref(b), 8, bufs["hits"].ptr, bufs["counts"].ptr) == 0
        renderer.sync()
        assert (bufs["hits"].download() == 7).all() and (bufs["counts"].download() == 7).all()


# ---------------------------------------------------------------------------------------------------------------- 3, 4
@pytest.mark.gpu
def test_truncation_and_ties(renderer):
    """Twelve quads in a row, two of them at one place: count 12 at k = 8, the eight kept entries the walk's, the coincident pair in
    object order, the near-coincident ones behind them."""
    s, o, d = rh.quad_stack()
    renderer.upload_scene(s)
    n = len(o)
    want_h, want_c = engine.hits_walk(s.arrays(), o, d, 8)
    w, cnt, _ = _device(renderer, o, d, 8)
    assert (cnt == 12).all() and (want_c == 12).all()
    _assert_equal((w, cnt), (rh.words(want_h, n, 8), want_c), "quad stack")
    dst, obj = w[..., 0].view(np.float32), w[..., 3]
    assert (obj == np.arange(8)[None, :]).all()
    assert (dst[:, 0] == dst[:, 1]).all() and (dst[:, 1] < dst[:, 2]).all() and (dst[:, 2] < dst[:, 3]).all()
    for k in (1, 2):
        wk, ck, _ = _device(renderer, o, d, k)
        assert (ck == 12).all() and np.array_equal(wk, w[:, :k])
    hh, hc = renderer.query_hits(o, d, 0)
    assert len(hh) == 0 and (hc == 12).all()


@pytest.mark.gpu
def test_spheres(renderer):
    """From outside: entry then exit; from inside: the exit only; a tangent ray and a radius-0 sphere: the walk's answer."""
    s, o, d, kinds = rh.sphere_scene()
    renderer.upload_scene(s)
    n = len(o)
    want_h, want_c = engine.hits_walk(s.arrays(), o, d, 8)
    w, cnt, _ = _device(renderer, o, d, 8)
    _assert_equal((w, cnt), (rh.words(want_h, n, 8), want_c), "spheres")
    rh.check_shape_of_lists(w, cnt, 8, "spheres")
    r = rh.rows(want_h, n, 8)
    zero = (r["isSphere"] == 1) & (r["objectHitIndex"] == 0)
    front = r["frontFace"] == 1
    out = kinds == "outside"
    assert (cnt[out] >= 2).all() and (cnt[out] % 2 == 0).all()
    assert ((zero & front).sum(axis=1)[out] == 1).all() and ((zero & ~front).sum(axis=1)[out] == 1).all()
    first = np.argmax(zero, axis=1)
    assert front[np.arange(n), first][out].all()                       # the entry comes first
    towards = np.einsum("ijk,ik->ij", r["normal"], d) < 0
    assert towards[zero & out[:, None]].all()                          # both normals face the ray: the exit's is turned round
    inside = kinds == "inside"
    assert ((zero & front).sum(axis=1)[inside] == 0).all() and ((zero & ~front).sum(axis=1)[inside] == 1).all()
    assert (cnt[kinds == "past"] == 0).all()
    assert (cnt[kinds == "tangent"] == want_c[kinds == "tangent"]).all()
    # with a limit between the two roots only the entry is left
    both = out & (cnt == 2)
    T = np.full(n, rh.MISS_DST, np.float32)
    T[both] = (r["dst"][both, 0] + r["dst"][both, 1]) / 2
    w2, c2, _ = _device(renderer, o, d, 8, T)
    assert (c2[both] == 1).all() and np.array_equal(w2[both, 0], w[both, 0]) and rh.is_miss_record(w2[both, 1]).all()


# ---------------------------------------------------------------------------------------------------------------- 5
def _chain_rays(arrays):
    """Rays at the comb scene's chain of triangles: from all round at points of the triangles, and along the chain through many."""
    rng = np.random.default_rng(9)
    n = arrays.triangleCount
    pos = np.array([[list(arrays.triPoints[v].position)[:3] for v in (arrays.triangles[t].v0, arrays.triangles[t].v1, arrays.triangles[t].v2)] for t in range(n)])
    k = rng.integers(0, n, 600)
    target = np.einsum("ij,ijk->ik", rng.dirichlet((1, 1, 1), 600), pos[k])
    o = target + rng.normal(size=(600, 3)) * 0.8
    # (every triangle's plane holds the chain's direction x and the line y = -0.5, z = 0, tilted by k % 3: a ray that climbs in z
    # at a constant small height above that line crosses the three planes one after the other, each inside a triangle or between two)
    x0, y = rng.uniform(-1.6, 1.0, 200), -0.5 + rng.uniform(0.001, 0.009, 200)
    along_o = np.stack([x0, y, np.full(200, -0.02)], 1)
    along_t = np.stack([x0 + rng.uniform(0.3, 1.5, 200), y, np.full(200, 0.05)], 1)
    return (np.concatenate([o, along_o]).astype(np.float32), np.concatenate([target - o, along_t - along_o]).astype(np.float32))


@pytest.mark.gpu
def test_the_deep_instantiation(renderer):
    comb = pq.build_scene("deep")
    assert comb.depth > 24
    renderer.upload_scene(comb)
    o, d = _chain_rays(comb.arrays())
    n = len(o)
    seen = 0
    for k in KS:
        want_h, want_c = engine.hits_walk(comb.arrays(), o, d, k)
        w, cnt, kernel = _device(renderer, o, d, k)
        assert kernel == DEEP, kernel
        _assert_equal((w, cnt), (rh.words(want_h, n, k), want_c), f"comb k = {k}")
        seen = max(seen, int(want_c.max()))
        hh, hc = renderer.query_hits(o, d, k)
        _assert_equal((rh.words(hh, n, k), hc), (rh.words(want_h, n, k), want_c), f"comb k = {k} / host form")
    assert (want_c >= 1).sum() >= 500 and seen >= 2
    renderer.upload_scene(cornell_scene(True))
    _device(renderer, o, d, 1)
    assert renderer.last_kernel() == SHALLOW


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_relation_to_the_other_ray_queries(renderer, name):
    c = rh.case(name)
    renderer.upload_scene(c["scene"])
    n = len(c["o"])
    for limited in (False, True):
        _, _, T = _walk(name, c, 8, "limits" if limited else None)
        w, cnt, _ = _device(renderer, c["o"], c["d"], 8, T)
        closest = renderer.query_closest(c["o"], c["d"], T)
        cw = rh.words(closest, n, 1)[:, 0]
        occluded = renderer.query_occluded(c["o"], c["d"], T)
        first, cdst = w[:, 0, 0].view(np.float32), cw[:, 0].view(np.float32)
        assert (first <= cdst).all(), f"{name}: hits[0].dst above the closest hit's at {np.flatnonzero(~(first <= cdst))[:5].tolist()}"
        print(f"[{name}, limits {limited}] hits[0].dst < closest.dst on {int((first < cdst).sum())} of {n} rays")
        # the closest hit is a member: where it is among the first eight, its record is the closest query's, byte for byte
        hit = cw[:, 1] == 1
        same_prim = (w[:, :, 2:5] == cw[:, None, 2:5]).all(axis=2) & (w[:, :, 1] == 1)
        where = np.argmax(same_prim, axis=1)
        listed = same_prim.any(axis=1)
        assert listed[hit & (cnt <= 8)].all(), f"{name}: the closest hit is not a member of the list"
        rec = w[np.arange(n), where]
        # (a sphere appears twice under one index: the closest query reports the entry, or from inside the exit, which is the first of them)
        assert np.array_equal(rec[listed & hit][:, :rh.COMPARED], cw[listed & hit][:, :rh.COMPARED]), name
        assert (cnt[occluded] >= 1).all(), f"{name}: occluded without a crossing"
        assert (cnt[hit] >= 1).all()


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.gpu
def test_a_hits_pass_leaves_rendering_alone(renderer):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_c1_64x64_4spp.npz"), allow_pickle=False)
    s = cornell_scene(True)
    renderer.upload_scene(s)
    pc = engine.push_constants(64, 64, singleRender=1, sampleLimit=4)
    before = renderer.render(pc, 64, 64)
    assert np.array_equal(before.view(np.uint32), z["rgba"].view(np.uint32))
    state = (renderer.last_pipeline(), renderer.last_parts())
    renderer.reset_counters()      # (it waits for the render and takes in what its snapshot says about the ray cost)
    zero = renderer.counters()
    cost = renderer.ray_cost()
    c = rh.case("cornell")
    T = _walk("cornell", c, 8, "limits")[2]
    hits, counts = renderer.query_hits(c["o"], c["d"], 8, T)
    assert renderer.last_kernel() == SHALLOW
    assert renderer.ray_cost() == cost
    got = renderer.counters()
    with np.errstate(invalid="ignore"):
        searched = int((T > 0).sum())
    assert got["raysTraced"] - zero["raysTraced"] == searched and got["raysHit"] - zero["raysHit"] == int((counts > 0).sum())
    assert got["boxTests"] > zero["boxTests"] and got["triTests"] > zero["triTests"]
    for key in got:
        if key not in ("boxTests", "triTests", "raysTraced", "raysHit"):
            assert got[key] == zero[key], key
    assert (renderer.last_pipeline(), renderer.last_parts()) == state and renderer.ray_cost() == cost
    after = renderer.render(pc, 64, 64)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert (renderer.last_pipeline(), renderer.last_parts()) == state
    # and the other queries after it are what they were
    assert np.array_equal(rh.words(renderer.query_closest(c["o"], c["d"]), len(c["o"]), 1)[:, 0, :rh.COMPARED], c["oracle_raw"][:, :rh.COMPARED])


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.gpu
def test_device_form_on_torch_tensors(renderer):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    c = rh.case("meshes")
    renderer.upload_scene(c["scene"])
    n, k = len(c["o"]), 4
    want_h, want_c, T = _walk("meshes", c, k, "limits")
    dev = torch.device("cuda:0")
    to, td, tt = torch.from_numpy(c["o"]).to(dev), torch.from_numpy(c["d"]).to(dev), torch.from_numpy(T).to(dev)
    out = torch.zeros((n, k, 15), dtype=torch.int32, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert renderer.query_hits(to, td, k, tt, out=out, counts=counts, sync=False) is None
    renderer._check(renderer._l.rt_sync(renderer._h), "rt_sync")
    _assert_equal((out.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)), (rh.words(want_h, n, k), want_c), "torch tensors, sync=False")
    with pytest.raises(ValueError):
        renderer.query_hits(to, td, k, tt, out=out[: n // 2].contiguous(), counts=counts)    # too small
    with pytest.raises(ValueError):
        renderer.query_hits(to, td, k, tt, out=out)                                           # no counts
    with pytest.raises(ValueError):
        renderer.query_hits(to, td, k, tt, counts=counts)                                     # k > 0 without out


@pytest.mark.gpu
def test_refusals_through_the_c_abi(renderer):
    renderer.upload_scene(cornell_scene(True))
    l, h = renderer._l, renderer._h
    P = 1 << 20     # never dereferenced: every call below is refused first
    for fn in ("rt_query_hits", "rt_query_hits_host"):
        f = getattr(l, fn)

        def refused(batch, k, hits, counts, words):
            assert f(h, None if batch is None else C.byref(batch), k, hits, counts) != 0
            assert l.rt_last_error(h).decode() == f"{fn}: {words}", l.rt_last_error(h).decode()

        ok = _capi.RtRayBatch(P, P, None, 5)
        refused(None, 8, P, P, "the batch is NULL")
        refused(_capi.RtRayBatch(None, P, None, 5), 8, P, P, "origins, dirs and the output are required")
        refused(_capi.RtRayBatch(P, None, None, 5), 8, P, P, "origins, dirs and the output are required")
        refused(ok, 9, P, P, "k = 9 is above RT_HITS_MAX_K = 8")
        refused(ok, 8, P, None, "counts and, with k > 0, hits are required")
        refused(ok, 1, None, P, "counts and, with k > 0, hits are required")
        refused(_capi.RtRayBatch(P, P, None, 1 << 30), 8, P, P, "a batch of 1073741824 rays does not fit the 30 bits of a slot id")
        refused(_capi.RtRayBatch(None, P, None, 1 << 30), 9, None, None, "origins, dirs and the output are required")   # the order
        refused(_capi.RtRayBatch(P, P, None, 1 << 30), 9, None, None, "k = 9 is above RT_HITS_MAX_K = 8")
        assert f(h, C.byref(_capi.RtRayBatch(None, None, None, 0)), 99, None, None) == 0
    fresh = engine.Renderer(0)
    try:
        assert fresh._l.rt_query_hits(fresh._h, C.byref(_capi.RtRayBatch(P, P, None, 5)), 8, P, P) != 0
        assert fresh._l.rt_last_error(fresh._h).decode() == "rt_query_hits before rt_upload_scene"
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        renderer.query_hits(np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32), 2)
    with pytest.raises(engine.RtError, match="RT_HITS_MAX_K"):
        renderer.query_hits(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), 9)


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.gpu
def test_alpha_mapped_scene(renderer, tmp_path):
    """A plane with an alpha map (texture_cases), under both samplers: the device equals the walk, and crossings are cut out."""
    tex = tc._map_set()
    for sampler in (0, 1):
        s = tc._bound(tmp_path, sampler, uv_scale=2.5, alphaIndex=1)
        o, d = rh.plane_rays(s)
        renderer.upload_scene(s.scene)
        s.push(renderer, "objects")
        s.push(renderer, "materials")
        try:
            renderer.upload_textures(tex)
            n = len(o)
            want_h, want_c = engine.hits_walk(s.arrays(), o, d, 8, textures=tex)
            w, cnt, kernel = _device(renderer, o, d, 8)
            assert kernel == SHALLOW
            _assert_equal((w, cnt), (rh.words(want_h, n, 8), want_c), f"alpha, sampler {sampler}")
            opaque_h, opaque_c = engine.hits_walk(s.arrays(), o, d, 8)
            assert 100 <= int((opaque_c - want_c).sum()) and (want_c <= opaque_c).all()     # cut-out crossings are gone from the count
            assert (opaque_c > want_c).sum() < (opaque_c > 0).sum()                           # and not every one is cut
            # the closest query sees the same holes
            closest = rh.words(renderer.query_closest(o, d), n, 1)[:, 0]
            assert np.array_equal(closest[:, 0].view(np.float32) < rh.MISS_DST, cnt > 0)
        finally:
            renderer.upload_textures([])
