"""The radius point queries on the CPU (rt_query_within's host-only unit ray_tracer_amd/csrc/point_within.h, the rule
include/rt_point_within.h, and the exhaustive host loop rt_within_exhaustive_host; engine.within_exhaustive).

tests/point_within_check.cpp, built with plain g++ under the sanitizers as a stand-alone program, provokes every refusal with
made-up addresses, in the stated order, with its message; covers the block and byte arithmetic at n = 0, 1, ... 2^30 - 1 and
k = 0, 1, 8, the stack choice at depths 24, 25, 64 and 65, the part layout of the _host form for 65 points, the units of the rule
and the loop on a hand-made scene (two coincident triangles in two objects and a sphere at the same distance).

The loop is then held to the float64 member sets of tests/within_float64.py on every scene and point set of
tests/point_query_cases.py, with reaches from that module's radius rule at m in {1, 2, 8, 9, 24}: under the rule no primitive lies
within 4 of its bounds of the reach, so the float64 set is the answer for every point and none is exempt. Counts must equal m'
exactly; every listed record is held to the float64 distance of the primitive it names; order and membership at the cut hold up
to the bounds; and the stated consequences hold bit for bit against rt_nearest_exhaustive_host."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
import point_query_cases as pq
import within_float64 as wf

K = 8
TARGETS = (1, 2, 8, 9, 24)

distances, raw, is_not_found = wf.case_distances, wf.raw, wf.is_not_found


def test_refusals_arithmetic_and_the_units_of_the_rule(tmp_path, built):
    exe = hostcheck.build(tmp_path, "point_within_check", ["point_within.cpp", "point_queries.cpp", "host_staging.cpp"], "point_within_check.cpp", opt="-O1")
    hostcheck.run(exe, ok="point within ok")


def check_against_float64(dist, reach, points, recs, counts, k, what):
    """Counts, distances, and order and membership at the cut."""
    n = len(points)
    assert np.array_equal(counts, reach.count), f"{what}: counts differ from m' at {np.flatnonzero(counts != reach.count)[:5].tolist()}"
    have = np.minimum(counts, k).astype(np.int64)
    col = wf.check_listed(dist, points, engine.nearest_to_numpy(recs), have, k, what)
    assert is_not_found(raw(recs, n, k)[col < 0]).all(), f"{what}: a slot past the count is not the not-found record"
    for i in range(n):
        listed = col[i, :have[i]]
        assert len(set(listed.tolist())) == len(listed), f"{what}: point {i} lists a primitive twice"
        if counts[i] <= k:
            assert set(listed.tolist()) == set(np.flatnonzero(reach.member[i]).tolist()), f"{what}: point {i}'s list is not the float64 member set"
            continue
        lo, hi = dist.d[i] - dist.b[i], dist.d[i] + dist.b[i]
        surely = np.flatnonzero(hi < lo[listed[-1]])                   # surely nearer than the last listed one
        assert np.isin(surely, listed).all(), f"{what}: point {i} misses a primitive that is surely among the first {k}"
        kth = np.partition(hi, k - 1)[k - 1]                          # the k-th smallest d + b
        assert (lo[listed] <= kth).all(), f"{what}: point {i} lists a primitive that is surely not among the first {k}"
    # ascending in dst (sqrt is monotone, so the records are as the key orders them)
    dst = engine.nearest_to_numpy(recs)["dst"].reshape(n, k)
    asc = np.arange(k - 1)[None, :] + 1 < have[:, None]
    assert (dst[:, :-1][asc] <= dst[:, 1:][asc]).all(), f"{what}: a list is not in ascending order"


def check_consequences(arrays, points, R, recs, counts, k, what):
    """Bit for bit against rt_nearest_exhaustive_host under the same limits."""
    n = len(points)
    wf.check_relations(raw(engine.nearest_exhaustive(arrays, points, R), n, 1)[:, 0], raw(recs, n, k), counts, k, what)


@pytest.mark.parametrize("name", pq.SCENES)
def test_exhaustive_host_against_float64_and_the_consequences(name):
    c = pq.case(name)
    arrays = c["scene"].arrays()
    for key, points in c["sets"].items():
        dist = distances(name, key)
        n = len(points)
        lists = {}
        for m in TARGETS:
            what = f"{name}/{key}/m={m}"
            reach = wf.Reach(dist, m)
            assert reach.clear.all(), f"{what}: {int((~reach.clear).sum())} points have a primitive within {wf.MARGIN} bounds of the reach: none may be exempt"
            assert (reach.count >= min(m, dist.d.shape[1])).all() and np.array_equal(reach.member.sum(axis=1), reach.count)
            recs, counts = engine.within_exhaustive(arrays, points, reach.R, K)
            check_against_float64(dist, reach, points, recs, counts, K, what)
            check_consequences(arrays, points, reach.R, recs, counts, K, what)
            lists[m] = (reach, raw(recs, n, K).copy(), counts)
            if m in (2, 9):
                # counts are the same for every k, and a smaller k is the head of the same list
                for k in (0, 1, 2):
                    rk, ck = engine.within_exhaustive(arrays, points, reach.R, k)
                    assert np.array_equal(ck, counts) and np.array_equal(raw(rk, n, k), lists[m][1][:, :k]), (what, k)
                    if k:
                        check_consequences(arrays, points, reach.R, rk, ck, k, f"{what}/k={k}")
        print(f"{name:14s} {key:9s} median m' at m = {TARGETS}: {[int(np.median(lists[m][0].count)) for m in TARGETS]}  largest {int(lists[TARGETS[-1]][0].count.max())}")
        # R1 <= R2: the list at R1 is the prefix of the list at R2 below fl(R1 R1): its first min(count1, k) entries
        for m1, m2 in ((1, 2), (2, 9), (9, 24)):
            (r1, b1, c1), (r2, b2, c2) = lists[m1], lists[m2]
            assert (r1.R <= r2.R).all() and (c1 <= c2).all()
            head = np.arange(K)[None, :] < np.minimum(c1, K)[:, None]
            assert np.array_equal(b1[head], b2[head]) and is_not_found(b1[~head]).all(), f"{name}/{key}: the list at m = {m1} is not the prefix of the list at m = {m2}"


def test_degenerate_reaches_admit_nothing():
    c = pq.case("cornell")
    points = c["sets"]["uniform"][:64]
    R = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), len(points))
    for k in (0, 1, K):
        recs, counts = engine.within_exhaustive(c["scene"].arrays(), points, R, k)
        assert not counts.any() and is_not_found(raw(recs, len(points), k)).all()


@pytest.mark.parametrize("name", ["spheres", "deep"])
def test_without_a_reach_every_surface_counts(name):
    c = pq.case(name)
    surfaces = len(c["ns"].sph_c) + len(c["ns"].W)
    for key, points in c["sets"].items():
        recs, counts = engine.within_exhaustive(c["scene"].arrays(), points, None, K)
        assert (counts == surfaces).all(), (name, key)
        have = np.full(len(points), min(surfaces, K))
        wf.check_listed(distances(name, key), points, engine.nearest_to_numpy(recs), have, K, f"{name}/{key}")
        check_consequences(c["scene"].arrays(), points, None, recs, counts, K, f"{name}/{key}")


def test_the_python_side_refuses_what_the_loop_refuses():
    c = pq.case("spheres")
    with pytest.raises(engine.RtError):
        engine.within_exhaustive(c["scene"].arrays(), c["sets"]["far"], None, 9)
    with pytest.raises(ValueError):
        engine.within_exhaustive(c["scene"].arrays(), c["sets"]["far"], np.ones(5, np.float32), 2)
    recs, counts = engine.within_exhaustive(c["scene"].arrays(), np.zeros((0, 3), np.float32), None, 8)
    assert len(recs) == 0 and len(counts) == 0
