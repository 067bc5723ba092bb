"""The cut queries on the CPU (rt_query_cuts' host-only unit ray_tracer_amd/csrc/cut_queries.h, the rule include/rt_tri_cut.h,
and the exhaustive host loop rt_cuts_exhaustive_host; engine.cuts_exhaustive, engine.cuts_to_numpy, engine.chain_cuts).

tests/cut_queries_check.cpp, built with plain g++ under the sanitizers as a stand-alone program, provokes every refusal with
made-up addresses, in the stated order, with its message; covers the block and byte arithmetic at n = 0, 1, ... 2^30 - 1 and
k = 0, 1, 8, the stack choice, the part layout of the _host form for 65 triangles, the rule on hand-made cases in small integers
and halves (where every fp32 operation is exact, so end points, features and the a / b order are literals: two triangles
crossing at right angles, in both windings; DESIGN.md's coplanar pair and coplanar members of the triangle query, no cut; a
corner exactly on the other's plane, where equal projections give the end to the query; a point touch, a == b; degenerate
queries, no cut), the bit-equality of the end on an edge that two scene triangles share, under all 36 ways of writing the two
and all rotations of the query, and the loop on a hand-made scene.

The loop is then held to the float64 cuts of tests/cut_float64.py on every scene of tests/point_query_cases.py, with
tri_overlap_float64's seeded queries. No query and no primitive is exempt: each seeded query is moved along its own normal in
fixed small steps until every scene triangle is unambiguous for it; the test asserts that it got there within
cut_float64.MAX_STEPS steps for every query, on the float64 side alone; and on those queries the loop's member set, counts and
order equal the float64 set exactly, featA / featB name the float64 piercing edges, and both end points lie within the counted
position bound of that module."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import cut_float64 as cf
import hostcheck
import point_query_cases as pq

K = 8


def test_refusals_arithmetic_and_the_rule_on_exact_cases(tmp_path, built):
    exe = hostcheck.build(tmp_path, "cut_queries_check", ["cut_queries.cpp", "tri_queries.cpp", "box_queries.cpp", "point_queries.cpp", "host_staging.cpp"], "cut_queries_check.cpp", opt="-O1")
    hostcheck.run(exe, ok="cut queries ok")


@pytest.mark.parametrize("name", pq.SCENES)
def test_the_float64_side_alone_gets_every_query_unambiguous(name):
    """Before anything is asked of the loop or the device: the steering reaches a query without an ambiguous pair within
    MAX_STEPS steps, on every set."""
    assert cf.MAX_STEPS == 8
    for key in pq.case(name)["sets"]:
        c = cf.case_cuts(name, key)
        assert (c.steps <= cf.MAX_STEPS).all() and c.clear.all(), f"{name}/{key}: {int((~c.clear).sum())} queries still have an ambiguous triangle after {cf.MAX_STEPS} steps: none may be exempt"
        assert np.isfinite(c.corners).all()


def _first_cuts(arrays, corners):
    """The loop's first 8 cuts of every query as a structured array [n, 8], and the counts (of all cuts)."""
    recs, counts = engine.cuts_exhaustive(arrays, corners, K)
    return engine.cuts_to_numpy(recs).reshape(len(counts), K), counts


@pytest.mark.parametrize("name", pq.SCENES)
def test_exhaustive_host_equals_the_float64_cuts(name):
    c = pq.case(name)
    ns = c["ns"]
    arrays = c["scene"].arrays()
    most, cuts_seen, long_cuts = 0, 0, 0
    for key in c["sets"]:
        b = cf.case_cuts(name, key)
        assert (b.steps <= cf.MAX_STEPS).all() and b.clear.all(), f"{name}/{key}: {int((~b.clear).sum())} queries still have an ambiguous triangle after {cf.MAX_STEPS} steps: none may be exempt"
        n = len(b.corners)
        got, counts = _first_cuts(arrays, b.corners)
        want_counts = b.member.sum(axis=1)
        assert np.array_equal(counts, want_counts), f"{name}/{key}: counts differ from the float64 sets at {np.flatnonzero(counts != want_counts)[:5].tolist()}"
        keys = cf.expected_keys(ns, b.member, K)
        got_keys = np.stack([got["found"], got["objectIndex"], got["triIndex"]], axis=-1)
        assert np.array_equal(got_keys, keys), f"{name}/{key}: members differ at queries {np.unique(np.argwhere(got_keys != keys)[:, 0])[:5].tolist()}"
        assert not got["reserved"].any()
        # the float64 cuts, in (query, key) order; those beyond a query's first 8 have no record to compare
        cuts = b.cuts
        slot = np.zeros(len(cuts["row"]), np.int64)
        for i in range(1, len(slot)):
            slot[i] = slot[i - 1] + 1 if cuts["row"][i] == cuts["row"][i - 1] else 0
        sel = slot < K
        r = got[cuts["row"][sel], slot[sel]]
        assert (r["found"] == 1).all()
        a32, b32 = r["a"].astype(np.float64), r["b"].astype(np.float64)
        a64, b64, ba, bb = cuts["a"][sel], cuts["b"][sel], cuts["ba"][sel], cuts["bb"][sel]
        fa, fb = cuts["fa"][sel], cuts["fb"][sel]
        dist = lambda x, y: np.sqrt(((x - y) ** 2).sum(axis=1))
        straight = (dist(a32, a64) <= ba) & (dist(b32, b64) <= bb) & (r["featA"] == fa) & (r["featB"] == fb)
        crossed = (dist(a32, b64) <= bb) & (dist(b32, a64) <= ba) & (r["featA"] == fb) & (r["featB"] == fa)
        long = dist(a64, b64) > 2.0 * (ba + bb)
        bad = ~np.where(long, straight, straight | crossed)
        worst = float(np.max(np.minimum(np.maximum(dist(a32, a64) / ba, dist(b32, b64) / bb), np.maximum(dist(a32, b64) / bb, dist(b32, a64) / ba)))) if len(r) else 0.0
        print(f"{name:14s} {key:9s} {int(sel.sum())} cuts compared ({int(long.sum())} longer than twice their bounds), the worst end at {worst:.3f} of its bound; steps up to {int(b.steps.max())}")
        assert not bad.any(), f"{name}/{key}: {int(bad.sum())} cuts outside the bound or on other edges, first at query {int(cuts['row'][sel][bad][0])}"
        for k in (0, 1, 2):
            rk, ck = engine.cuts_exhaustive(arrays, b.corners, k)
            assert np.array_equal(ck, counts)
            assert bytes(engine.cuts_to_numpy(rk).reshape(n, k).tobytes()) == got[:, :k].tobytes(), (name, key, k)
        # every cut member is a member of the triangle query, under the same key, and the keys ascend
        trecs, tcounts = engine.tris_exhaustive(arrays, b.corners, K)
        t = np.frombuffer(trecs, np.uint32).reshape(n, K, 4)
        assert (counts <= tcounts).all()
        for i in np.flatnonzero((tcounts <= K) & (counts > 0)):
            mine = {(int(o), int(tr)) for o, tr in zip(got["objectIndex"][i, :counts[i]], got["triIndex"][i, :counts[i]])}
            theirs = {(int(x[2]), int(x[3])) for x in t[i, :tcounts[i]] if x[1] == 0}
            assert mine <= theirs, (name, key, int(i))
        order = got["objectIndex"].astype(np.int64) * (1 << 32) + got["triIndex"]
        filled = got["found"] == 1
        assert ((np.diff(order, axis=1) > 0) | ~filled[:, 1:]).all(), f"{name}/{key}: keys do not ascend"
        assert (filled[:, :-1] | ~filled[:, 1:]).all(), f"{name}/{key}: a record behind an empty one"
        most = max(most, int(counts.max()) if n else 0)
        cuts_seen += int(sel.sum())
        long_cuts += int(long.sum())
    if len(ns.W):
        assert cuts_seen > 0 and long_cuts > 0, f"{name}: no cut was compared"
        print(f"{name}: the most cuts of a query: {most}")
        # (the 30 thin triangles of `deep` are crossed 8 at a time at the most; its share is the deep kernel, not the full list)
        assert most > K or name == "deep", f"{name}: no query has more cuts than slots"
    else:
        assert most == 0, f"{name}: a scene without triangles has cuts"


def test_coplanar_pairs_the_walls_own_triangles_have_no_cut_with_themselves():
    """Case (iii) of cut_float64: the scene's own axis-aligned triangle as the query is exactly coplanar with itself (every height
    is an exact 0 in float32 as in float64): a member of the triangle query, never of this one."""
    c = pq.case("cornell")
    a = c["scene"].arrays()
    ns = c["ns"]
    plain = np.array([all(abs(a.objects[i].transformMatrix[col * 4 + r]) in (0.0, 1.0) for col in range(3) for r in range(3)) for i in range(a.objectCount)])
    exact = (ns.W.astype(np.float32).astype(np.float64) == ns.W).all(axis=(1, 2))                      # float32 numbers
    rows = np.flatnonzero(plain[ns.obj] & exact & ((ns.W.max(axis=1) - ns.W.min(axis=1)) == 0).any(axis=1))   # flat along an axis
    assert len(rows) >= 10, "the Cornell box has no walls?"
    q = ns.W[rows].astype(np.float32)
    ok, _, _, _, _, _, _, coplanar = cf.cut_pairs(q.astype(np.float64), ns.W[rows], ns.mag[rows])
    assert coplanar.all() and not ok.any()
    recs, counts = engine.cuts_exhaustive(a, q.reshape(-1, 9), K)
    got = engine.cuts_to_numpy(recs).reshape(len(q), K)
    _, tcounts = engine.tris_exhaustive(a, q.reshape(-1, 9), 0)
    assert (tcounts >= 1).all()
    shown = 0
    for i, row in enumerate(rows):
        own = (got["found"][i] == 1) & (got["objectIndex"][i] == ns.obj[row]) & (got["triIndex"][i] == ns.tri[row])
        assert not own.any(), f"wall triangle {int(row)} has a cut with itself"
        # its absence from the first 8 shows it only where the list is whole or already past its key
        last = (int(got["objectIndex"][i, K - 1]), int(got["triIndex"][i, K - 1]))
        shown += counts[i] <= K or last > (int(ns.obj[row]), int(ns.tri[row]))
    assert shown >= 10, f"only {shown} wall triangles show that they have no cut with themselves"


def test_invalid_and_degenerate_triangles_have_no_cut():
    c = pq.case("cornell")
    q = np.tile(np.array([-2, -2, -2, 2, -2, 2, 0, 2, 0], np.float32), (8, 1))
    q[0, 0], q[1, 4], q[2, 8], q[3, 3] = np.nan, np.inf, -np.inf, np.nan
    q[5, 3:6] = q[5, 0:3]                      # two equal corners: a segment through the box
    q[6, 3:6] = q[6, 6:9] = q[6, 0:3]          # three: a point
    q[7, 6:9] = q[7, 3:6]
    for k in (0, 1, K):
        recs, counts = engine.cuts_exhaustive(c["scene"].arrays(), q, k)
        assert not counts[:4].any() and counts[4] > 0 and not counts[5:].any()
        r = np.frombuffer(recs, np.uint8).reshape(8, k, 48) if k else np.zeros((8, 0, 48), np.uint8)
        assert not r[:4].any() and not r[5:].any()
    _, tcounts = engine.tris_exhaustive(c["scene"].arrays(), q, 0)
    assert tcounts[5] > 0, "the segment touches nothing: the case shows nothing"


def test_the_python_side_refuses_what_the_loop_refuses():
    c = pq.case("cornell")
    q = cf.seed_corners("cornell", "uniform")
    with pytest.raises(engine.RtError):
        engine.cuts_exhaustive(c["scene"].arrays(), q, 9)
    with pytest.raises(ValueError):
        engine.cuts_exhaustive(c["scene"].arrays(), q.reshape(-1)[:10], 2)
    recs, counts = engine.cuts_exhaustive(c["scene"].arrays(), np.zeros((0, 9), np.float32), 8)
    assert len(recs) == 0 and len(counts) == 0 and len(engine.cuts_to_numpy(recs)) == 0
    big = np.tile(np.array([-2000, -2000, 0.05, 2000, -2000, 0.05, 0, 2000, 0.05], np.float32), (3, 1))
    o = engine.cuts_to_numpy(engine.cuts_exhaustive(c["scene"].arrays(), big, 2)[0])
    assert o.dtype.names == ("a", "featA", "b", "featB", "found", "objectIndex", "triIndex", "reserved") and o.dtype.itemsize == 48
    assert o.shape == (6,) and o["found"].all() and o["a"].shape == (6, 3)
    assert np.allclose(o["a"][:, 2], 0.05) and np.allclose(o["b"][:, 2], 0.05)   # a horizontal slice: every cut lies in it


@pytest.mark.parametrize("name", ["torus", "cubes"])
def test_cuts_of_a_closed_mesh_close(name):
    """On the closed meshes of tests/side_cases.py, small seeded queries with at most 8 cuts: the ends on scene edges pair up bit
    for bit, and engine.chain_cuts walks them into chains that leave the query through its own edges."""
    scene, q = cf.closure_queries(name)
    recs, counts = engine.cuts_exhaustive(scene.arrays(), q, K)
    looked, shared = cf.check_closure(engine.cuts_to_numpy(recs).reshape(len(q), K), counts)
    print(f"{name}: {looked} queries with 1 to 8 cuts, {shared} ends shared along scene edges")
    assert looked >= 100 and shared >= 100


def _rec(a, b, fa=3, fb=3, found=1):
    r = np.zeros(1, engine.CUT_DTYPE)
    r["a"], r["b"], r["featA"], r["featB"], r["found"] = a, b, fa, fb, found
    return r


def test_chain_cuts_on_hand_made_records():
    """Numpy only. A square loop given out of order and with one cut turned round, an open chain of three, a lone cut, an empty
    record in between, and a point cut hanging on the chain's end."""
    P = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
    recs = np.concatenate([
        _rec(P[0], P[1]), _rec(P[2], P[3]), _rec(P[2], P[1]), _rec(P[3], P[0]),            # 0..3: the loop 0 1 2 3 (cut 2 turned round)
        _rec((0, 0, 0), (0, 0, 0), found=0),                                               # 4: empty
        _rec((5, 0, 0), (6, 0, 0), fa=0), _rec((7, 0, 0), (8, 0, 0), fb=1), _rec((7, 0, 0), (6, 0, 0)),   # 5..7: the chain 5 7 6
        _rec((9, 9, 9), (9, 9, 8), fa=0, fb=2),                                            # 8: alone
        _rec((8, 0, 0), (8, 0, 0)),                                                        # 9: a point on the chain's end
    ])
    loops, chains = engine.chain_cuts(recs)
    assert len(loops) == 1 and sorted(loops[0]) == [0, 1, 2, 3]
    ring = loops[0]
    for x, y in zip(ring, ring[1:] + ring[:1]):   # neighbours in the walk share a point
        ends = lambda i: {tuple(recs["a"][i]), tuple(recs["b"][i])}
        assert ends(x) & ends(y)
    assert sorted(map(sorted, chains)) == [[5, 6, 7, 9], [8]]
    long = [c for c in chains if len(c) == 4][0]
    assert long in ([5, 7, 6, 9], [9, 6, 7, 5])
    # -0.0 and 0.0 are different bits: chains join by bits, as the rule promises them
    two = np.concatenate([_rec((0, 0, 0), (1, 0, 0)), _rec((1, -0.0, 0), (2, 0, 0))])
    loops, chains = engine.chain_cuts(two)
    assert loops == [] and sorted(chains) == [[0], [1]]
    assert engine.chain_cuts(np.zeros(0, engine.CUT_DTYPE)) == ([], [])
