"""The triangle queries on the CPU (rt_query_triangles' host-only unit ray_tracer_amd/csrc/tri_queries.h, the rule
include/rt_tri_overlap.h, and the exhaustive host loop rt_tris_exhaustive_host; engine.tris_exhaustive).

tests/tri_queries_check.cpp, built with plain g++ under the sanitizers as a stand-alone program, provokes every refusal with
made-up addresses, in the stated order, with its message; covers the block and byte arithmetic at n = 0, 1, ... 2^30 - 1 and
k = 0, 1, 8, the stack choice at depths 24, 25, 64 and 65, the part layout of the _host form for 65 triangles, the rule on
hand-made cases in small integers and halves (where every fp32 operation is exact, so the rule must give the true answer: a
shared corner, a shared edge, edges crossing in one plane, the coplanar pair that only an in-plane edge normal separates and
that the first eleven axes call touching, one triangle inside another, parallel planes, an edge piercing a face, a corner
resting on a face, queries with two and three equal corners, NaN corners, the sphere's shell from inside, across and outside),
the pruning comparisons, and the loop on a hand-made scene.

The loop is then held to the float64 member sets of tests/tri_overlap_float64.py on every scene of tests/point_query_cases.py,
with query triangles about the points of its four point sets in four seeded classes (small, slivers 1 : 16, large, turned copies
of the scene's own triangles). No query and no primitive is exempt: the generator moves each seeded query along its own normal in
fixed small steps until every primitive of the scene is unambiguous for it (touching by an edge that pierces a face with the
pair's margin, or apart by more than the pair's bound), the test asserts that it got there within
tri_overlap_float64.MAX_STEPS steps for every query, and on those queries the loop's member set, counts and order equal the
float64 set exactly."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
import point_query_cases as pq
import tri_overlap_float64 as tf

K = 8


def test_refusals_arithmetic_and_the_rule_on_exact_cases(tmp_path, built):
    exe = hostcheck.build(tmp_path, "tri_queries_check", ["tri_queries.cpp", "box_queries.cpp", "point_queries.cpp", "host_staging.cpp"], "tri_queries_check.cpp", opt="-O1")
    hostcheck.run(exe, ok="triangle queries ok")


@pytest.mark.parametrize("name", pq.SCENES)
def test_the_float64_side_alone_gets_every_query_unambiguous(name):
    """Before anything is asked of the loop or the device: the steering reaches a query without an ambiguous pair within
    MAX_STEPS steps, on every set."""
    for key in pq.case(name)["sets"]:
        b = tf.case_triangles(name, key)
        assert (b.steps <= tf.MAX_STEPS).all() and b.clear.all(), f"{name}/{key}: {int((~b.clear).sum())} queries still have an ambiguous primitive after {tf.MAX_STEPS} steps: none may be exempt"
        assert np.isfinite(b.corners).all()


@pytest.mark.parametrize("name", pq.SCENES)
def test_exhaustive_host_equals_the_float64_sets(name):
    c = pq.case(name)
    arrays = c["scene"].arrays()
    most = 0
    for key in c["sets"]:
        b = tf.case_triangles(name, key)
        assert (b.steps <= tf.MAX_STEPS).all() and b.clear.all(), f"{name}/{key}: {int((~b.clear).sum())} queries still have an ambiguous primitive after {tf.MAX_STEPS} steps: none may be exempt"
        n = len(b.corners)
        recs, counts = engine.tris_exhaustive(arrays, b.corners, K)
        want_counts = b.member.sum(axis=1)
        assert np.array_equal(counts, want_counts), f"{name}/{key}: counts differ from the float64 sets at {np.flatnonzero(counts != want_counts)[:5].tolist()}"
        want = tf.expected_records(c["ns"], b.member, K)
        got = np.frombuffer(recs, np.uint32).reshape(n, K, 4)
        assert np.array_equal(got, want), f"{name}/{key}: records differ at queries {np.unique(np.argwhere(got != want)[:, 0])[:5].tolist()}"
        for k in (0, 1, 2):
            rk, ck = engine.tris_exhaustive(arrays, b.corners, k)
            assert np.array_equal(ck, counts)
            assert np.array_equal(np.frombuffer(rk, np.uint32).reshape(n, k, 4) if k else np.zeros((n, 0, 4), np.uint32), want[:, :k]), (name, key, k)
        most = max(most, int(counts.max()))
        for ci, cls in enumerate(tf.CLASSES):
            sel = b.cls == ci
            if sel.any():
                print(f"{name:14s} {key:9s} {cls:6s} median members {int(np.median(counts[sel]))}, largest {int(counts[sel].max())}, steps up to {int(b.steps[sel].max())}")
    surfaces = len(c["ns"].sph_c) + len(c["ns"].W)
    assert most > K or surfaces <= K, f"{name}: no query has more members than slots"


def test_invalid_triangles_have_no_member():
    c = pq.case("cornell")
    q = np.tile(np.array([-2, -2, -2, 2, -2, 2, 0, 2, 0], np.float32), (5, 1))
    q[0, 0], q[1, 4], q[2, 8], q[3, 3] = np.nan, np.inf, -np.inf, np.nan
    for k in (0, 1, K):
        recs, counts = engine.tris_exhaustive(c["scene"].arrays(), q, k)
        assert not counts[:4].any() and counts[4] > 0
        assert not np.frombuffer(recs, np.uint32).reshape(5, k, 4)[:4].any() if k else True


def test_the_python_side_refuses_what_the_loop_refuses():
    c = pq.case("spheres")
    q = tf.seed_corners("spheres", "far")
    with pytest.raises(engine.RtError):
        engine.tris_exhaustive(c["scene"].arrays(), q, 9)
    with pytest.raises(ValueError):
        engine.tris_exhaustive(c["scene"].arrays(), q.reshape(-1)[:10], 2)
    recs, counts = engine.tris_exhaustive(c["scene"].arrays(), np.zeros((0, 9), np.float32), 8)
    assert len(recs) == 0 and len(counts) == 0
    big = np.tile(np.array([-2000, -2000, 0.05, 2000, -2000, 0.05, 0, 2000, 0.05], np.float32), (3, 1))   # cuts the first two spheres
    o = engine.overlap_to_numpy(engine.tris_exhaustive(c["scene"].arrays(), big, 2)[0])
    assert set(o) == {"found", "isSphere", "objectIndex", "triIndex"} and o["found"].shape == (6,) and o["found"].all() and o["isSphere"].all()


def test_mesh_corners_restates_rt_xform_point_in_float32():
    """query_mesh's gather: points[faces], each point taken through the matrix in float32, one rounding an operation, in
    rt_xform_point's order; against float64 within the 4 u |M||[v;1]| of that count, and equal to itself without a matrix."""
    rng = np.random.default_rng(5)
    pts = rng.uniform(-2, 2, (50, 3)).astype(np.float32)
    faces = rng.integers(0, 50, (80, 3))
    assert np.array_equal(engine.mesh_corners(pts, faces), pts[faces].reshape(-1, 9))
    ident = np.eye(4, dtype=np.float32).reshape(16)
    assert np.array_equal(engine.mesh_corners(pts, faces, ident), pts[faces].reshape(-1, 9))
    m = rng.uniform(-1.5, 1.5, 16).astype(np.float32)
    got = engine.mesh_corners(pts, faces, m)
    assert got.dtype == np.float32 and got.shape == (80, 9)
    M = m.astype(np.float64).reshape(4, 4).T
    want = (pts.astype(np.float64) @ M[:3, :3].T + M[:3, 3])[faces].reshape(-1, 9)
    mag = (np.abs(pts.astype(np.float64)) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3]))[faces].reshape(-1, 9)
    assert (np.abs(got - want) <= 4 * 2.0 ** -24 * mag).all()
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    first = ((x * m[0] + y * m[4]) + z * m[8]) + m[12]
    assert np.array_equal(got.reshape(80, 3, 3)[:, :, 0], first[faces])
