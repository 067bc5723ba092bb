"""The box queries on the CPU (rt_query_boxes' host-only unit ray_tracer_amd/csrc/box_queries.h, the rule
include/rt_box_overlap.h, and the exhaustive host loop rt_boxes_exhaustive_host; engine.boxes_exhaustive).

tests/box_queries_check.cpp, built with plain g++ under the sanitizers as a stand-alone program, provokes every refusal with
made-up addresses, in the stated order, with its message; covers the block and byte arithmetic at n = 0, 1, ... 2^30 - 1 and
k = 0, 1, 8, the stack choice at depths 24, 25, 64 and 65, the part layout of the _host form for 65 boxes, the rule on a table of
cases in small integers and halves (where every fp32 operation is exact, so the rule must give the true answer), the pruning
comparisons, and the loop on a hand-made scene.

The loop is then held to the float64 member sets of tests/overlap_float64.py on every scene of tests/point_query_cases.py, with
boxes about the points of its four point sets in three seeded classes (small cubes, 1 : 4 : 16 boxes, large boxes). No box and
no primitive is exempt: the generator grows each seeded box in fixed small steps until every primitive of the scene is
unambiguous for it (the float64 test gives one answer for the box grown and shrunk by the pair's bound), the test asserts that
it got there within overlap_float64.MAX_STEPS steps for every box and that every half-extent exceeds the bound, and on those
boxes the loop's member set, counts and order equal the float64 set exactly."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
import overlap_float64 as of
import point_query_cases as pq

K = 8


def test_refusals_arithmetic_and_the_rule_on_exact_cases(tmp_path, built):
    exe = hostcheck.build(tmp_path, "box_queries_check", ["box_queries.cpp", "point_queries.cpp", "host_staging.cpp"], "box_queries_check.cpp", opt="-O1")
    hostcheck.run(exe, ok="box queries ok")


@pytest.mark.parametrize("name", pq.SCENES)
def test_exhaustive_host_equals_the_float64_sets(name):
    c = pq.case(name)
    arrays = c["scene"].arrays()
    most = 0
    for key in c["sets"]:
        b = of.case_boxes(name, key)
        assert (b.steps <= of.MAX_STEPS).all() and b.clear.all(), f"{name}/{key}: {int((~b.clear).sum())} boxes still have an ambiguous primitive after {of.MAX_STEPS} steps: none may be exempt"
        assert (b.half > b.beta_max[:, None]).all(), f"{name}/{key}: a half-extent does not exceed the bound"
        n = len(b.lo)
        recs, counts = engine.boxes_exhaustive(arrays, b.lo, b.hi, K)
        want_counts = b.member.sum(axis=1)
        assert np.array_equal(counts, want_counts), f"{name}/{key}: counts differ from the float64 sets at {np.flatnonzero(counts != want_counts)[:5].tolist()}"
        want = of.expected_records(c["ns"], b.member, K)
        got = np.frombuffer(recs, np.uint32).reshape(n, K, 4)
        assert np.array_equal(got, want), f"{name}/{key}: records differ at boxes {np.unique(np.argwhere(got != want)[:, 0])[:5].tolist()}"
        for k in (0, 1, 2):
            rk, ck = engine.boxes_exhaustive(arrays, b.lo, b.hi, k)
            assert np.array_equal(ck, counts)
            assert np.array_equal(np.frombuffer(rk, np.uint32).reshape(n, k, 4) if k else np.zeros((n, 0, 4), np.uint32), want[:, :k]), (name, key, k)
        most = max(most, int(counts.max()))
        for ci, cls in enumerate(of.CLASSES):
            sel = b.cls == ci
            print(f"{name:14s} {key:9s} {cls:6s} median members {int(np.median(counts[sel]))}, largest {int(counts[sel].max())}, steps up to {int(b.steps[sel].max())}")
    surfaces = len(c["ns"].sph_c) + len(c["ns"].W)
    assert most > K or surfaces <= K, f"{name}: no box has more members than slots"


def test_invalid_boxes_have_no_member():
    c = pq.case("cornell")
    lo = np.array([[np.nan, 0, 0], [0, 1, 0], [0, 0, 0], [-np.inf, 0, 0], [-1, -1, -1]], np.float32)
    hi = np.array([[1, 1, 1], [1, 0, 1], [1, np.inf, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    for k in (0, 1, K):
        recs, counts = engine.boxes_exhaustive(c["scene"].arrays(), lo, hi, k)
        assert not counts[:4].any() and counts[4] > 0
        assert not np.frombuffer(recs, np.uint32).reshape(5, k, 4)[:4].any() if k else True


def test_the_python_side_refuses_what_the_loop_refuses():
    c = pq.case("spheres")
    p = c["sets"]["far"]
    with pytest.raises(engine.RtError):
        engine.boxes_exhaustive(c["scene"].arrays(), p, p, 9)
    with pytest.raises(ValueError):
        engine.boxes_exhaustive(c["scene"].arrays(), p, p[:5], 2)
    recs, counts = engine.boxes_exhaustive(c["scene"].arrays(), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 8)
    assert len(recs) == 0 and len(counts) == 0
    o = engine.overlap_to_numpy(engine.boxes_exhaustive(c["scene"].arrays(), p[:3] - 2000, p[:3] + 2000, 2)[0])
    assert set(o) == {"found", "isSphere", "objectIndex", "triIndex"} and o["found"].shape == (6,) and o["found"].all() and o["isSphere"].all()
