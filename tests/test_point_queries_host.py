"""The point queries on the CPU (rt_query_nearest's host-only unit ray_tracer_amd/csrc/point_queries.h, the rule
include/rt_point_query.h, and rt_nearest_exhaustive_host).

tests/point_queries_check.cpp, built with plain g++, provokes every refusal with made-up addresses, in the stated order, with its
message; covers the block and byte arithmetic at n = 0, 1, ... and 2^30 - 1 (the staging offsets: tests/test_host_staging_host.py); the stack choice; rt_point_triangle in each of
its seven regions, on the plane (dst exactly 0), at a vertex and on zero-area triangles; rt_point_sphere; and the exhaustive loop
on a hand-made scene. It also prints the pruning record of the matrices this file hands it, and sMin is held against numpy's
singular values: never above the true value, and within the stated margin below it.

rt_nearest_exhaustive_host is then held against the float64 brute force (tests/nearest_float64.py) on every scene and point set of
tests/point_query_cases.py, by the rules of check_records there; the largest |dst - ref| / bound(C = 1) per set is printed, and
C must be at least twice the worst. The limits T = 0.5, 0.999, 1.001 and 2 x the float64 distance run on the uniform sets: found iff
dst < T, no point within the bound of its limit (the exempt share is 0)."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import brute_force as bf
import hostcheck
import nearest_float64 as nf
import point_query_cases as pq

FACTORS = (0.5, 0.999, 1.001, 2.0)
SMIN_MARGIN = 1e-6     # RT_NEAREST_SMIN_MARGIN


def _matrices():
    """name -> 4x4 float64 (as float32 holds it): rotations, uniform and non-uniform scales, shears, and a flat one."""
    shear = np.eye(4)
    shear[0, 1], shear[2, 0] = 0.7, -0.4
    big_shear = np.eye(4)
    big_shear[0, 1], big_shear[1, 2], big_shear[0, 2] = 5.0, -3.0, 2.0
    m = {"rotation": bf.placement_matrix(rotation=(20, 35, 10)),
         "uniform": bf.placement_matrix(position=(1, 2, 3), rotation=(-75, 10, 130), scale=0.6),
         "non_uniform": bf.placement_matrix(position=(0.7, 0.1, -0.3), scale=(1.0, 0.4, 2.5)),
         "rotated_non_uniform": bf.placement_matrix(rotation=(33, -48, 71), scale=(3.0, 0.05, 1.0)),
         "shear": shear @ bf.placement_matrix(position=(0, -0.9, 0.6)),
         "big_shear": big_shear @ bf.placement_matrix(rotation=(10, 20, 30), scale=(2.0, 1.0, 0.25)),
         "flat": bf.placement_matrix(rotation=(5, 5, 5), scale=(1.0, 1e-4, 1.0)),
         "identity_with_translation": bf.placement_matrix(position=(4, 5, 6))}
    return {k: v.astype(np.float32).astype(np.float64) for k, v in m.items()}


@pytest.fixture(scope="module")
def checked(tmp_path_factory, built):
    """The check program built with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they are installed,
    and run once on the matrices: its output."""
    d = tmp_path_factory.mktemp("point_queries")
    exe = hostcheck.build(d, "point_queries_check", ["point_queries.cpp"], "point_queries_check.cpp", opt="-O1")
    mats = _matrices()
    path = d / "matrices.bin"
    np.stack([m.T.reshape(-1) for m in mats.values()]).astype(np.float32).tofile(path)    # column-major
    out = hostcheck.run(exe, [path], ok="point queries ok")
    rows = [tuple(float(x) for x in line.split()[1:]) for line in out.splitlines() if line.startswith("prune ")]
    assert len(rows) == len(mats)
    return dict(zip(mats, rows))


def test_refusals_arithmetic_and_the_units_of_the_rule(checked):
    assert len(checked) == len(_matrices())


@pytest.mark.parametrize("name", list(_matrices()))
def test_smin_is_below_the_smallest_singular_value_by_at_most_the_margin(checked, name):
    M = _matrices()[name]
    true = np.linalg.svd(M[:3, :3], compute_uv=False).min()
    s_min, pad_q = checked[name]
    assert s_min <= true, f"sMin {s_min!r} above the smallest singular value {true!r}"
    assert s_min >= true * (1 - SMIN_MARGIN) * (1 - 2.0 ** -23), f"sMin {s_min!r} more than the margin below {true!r}"
    # padQ bounds what float32 does to inverse(M) q: the inverse's entries (10 u E1) and the row's own roundings (4 u |inv|)
    E = 10 * bf.inverse_error_unit(M)[:3] + 4 * np.abs(np.linalg.inv(M))[:3]
    want = np.sqrt(3) * nf.U32 * E.sum(axis=1).max()
    assert want <= pad_q <= want * (1 + 1e-5), (pad_q, want)
    # and it does bound it, on a few points
    rng = np.random.default_rng(5)
    q = rng.uniform(-3, 3, (64, 3)).astype(np.float32)
    inv32 = np.linalg.inv(M).astype(np.float32)        # (within the 10 u E1 of rt_mat4_inverse's own)
    got = (inv32[:3, :3] @ q.T).T + inv32[:3, 3]
    exact = (np.linalg.inv(M)[:3, :3] @ q.astype(np.float64).T).T + np.linalg.inv(M)[:3, 3]
    err = np.linalg.norm(got.astype(np.float64) - exact, axis=1)
    assert (err <= pad_q * np.maximum(np.abs(q).max(axis=1), 1.0)).all()


@pytest.mark.parametrize("name", pq.SCENES)
def test_exhaustive_host_against_float64(name):
    c = pq.case(name)
    arrays = c["scene"].arrays()
    worst = 0.0
    for k, points in c["sets"].items():
        rec = engine.nearest_to_numpy(engine.nearest_exhaustive(arrays, points))
        ratio = pq.check_records(c, points, rec, c["ref"][k], f"{name}/{k}")
        print(f"{name:14s} {k:9s} largest |dst - ref| / bound(C = 1) = {ratio:.3f}")
        worst = max(worst, ratio)
    assert nf.NEAREST_C >= 2 * worst, f"{name}: C = {nf.NEAREST_C} is not twice the worst observed ratio {worst:.3f}"
    assert worst <= 2 * nf.OBSERVED[name], f"{name}: the ratio {worst:.3f} has left what the docstring of nearest_float64 records"


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name", pq.SCENES)
def test_limits_on_the_uniform_set(name, factor):
    """found iff dst < T. No point of the set lies within its bound of T (so none is exempt), and the record of a found point is
    the unlimited query's, bit for bit."""
    c = pq.case(name)
    points, ref = c["sets"]["uniform"], c["ref"]["uniform"]
    T = (np.float64(factor) * ref["dst"]).astype(np.float32)
    exempt = np.abs(ref["dst"] - T.astype(np.float64)) <= ref["bound"]
    assert not exempt.any(), f"{int(exempt.sum())} points within their bound of the limit: choose another seed"
    arrays = c["scene"].arrays()
    free = engine.nearest_exhaustive(arrays, points)
    lim = engine.nearest_exhaustive(arrays, points, T)
    f, l = engine.nearest_to_numpy(free), engine.nearest_to_numpy(lim)
    assert np.array_equal(l["found"] != 0, ref["dst"] < T.astype(np.float64))
    assert np.array_equal(l["found"] != 0, f["dst"] < T)
    raw_f = np.frombuffer(free, np.uint8).reshape(len(points), -1)
    raw_l = np.frombuffer(lim, np.uint8).reshape(len(points), -1)
    hit = l["found"] != 0
    assert np.array_equal(raw_l[hit], raw_f[hit])
    assert (l["dst"][~hit] == np.float32(99999999.0)).all() and not raw_l[~hit][:, 4:].any()


def test_limits_that_admit_nothing():
    c = pq.case("cornell")
    points = c["sets"]["uniform"][:64]
    T = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), len(points))
    l = engine.nearest_to_numpy(engine.nearest_exhaustive(c["scene"].arrays(), points, T))
    assert not l["found"].any() and (l["dst"] == np.float32(99999999.0)).all() and not l["point"].any()
