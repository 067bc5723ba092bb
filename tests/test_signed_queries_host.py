"""The rule of the signed point queries on the CPU, before any GPU run: rt_nearest_side_host applied to the records of
rt_nearest_exhaustive_host, on every scene and point set of tests/side_cases.py, against the float64 winding number of
tests/side_float64.py (check_sides: every kept point on the side the reference says, 0 where the component is not signable, spheres
exactly, at most 2 % of a set excluded). Also engine.signed_distance and Scene.topology on those scenes."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import side_cases as sc
import side_float64 as sf


def _host_sides(c, points):
    arrays = c["scene"].arrays()
    recs = engine.nearest_exhaustive(arrays, points)
    return recs, engine.nearest_side_host(arrays, points, recs)


@pytest.mark.parametrize("name", sc.SCENES)
def test_side_host_on_exhaustive_records_against_the_winding_number(name):
    c = sc.case(name)
    for k, points in c["sets"].items():
        recs, side = _host_sides(c, points)
        rec = engine.nearest_to_numpy(recs)
        t = sc.check_sides(c, points, rec, side, c["ref"][k], f"{name}/{k}")
        tri = (rec["found"] != 0) & (rec["isSphere"] == 0)
        print(f"{name:14s} {k:9s} sides -1/0/+1: {(side == -1).sum()}/{(side == 0).sum()}/{(side == 1).sum()}, excluded {t['excluded'].mean():.2%}, "
              f"smallest |cos| kept {t['cosine'][t['kept'] & t['signable']].min() if (t['kept'] & t['signable']).any() else float('nan'):.2f}")
        if name in ("cubes", "torus", "torus_flipped", "spikes"):
            assert (side[tri & t["kept"]] != 0).all()
        if name == "klein":
            assert not side.any()
        if name == "mixed":                                    # open walls and the bunny are unsigned (the box's closed blocks are not); the spheres are signed
            bunny = tri & (rec["objectIndex"] == c["arrays"]["objects"].shape[0] - 1)
            assert not side[tri & ~t["signable"]].any() and not side[bunny].any() and side[rec["isSphere"] != 0].all()
            assert k != "uniform" or (bunny.any() and (tri & ~t["signable"] & ~bunny).any())
    if "inside" in c["sets"]:
        assert (_host_sides(c, c["sets"]["inside"])[1] == -1).mean() > 0.9


def test_the_flipped_torus_answers_as_the_torus_does():
    a, b = sc.case("torus"), sc.case("torus_flipped")
    stats = b["scene"].scene.topology()[0]
    _, which = sc.flipped(sc.torus_mesh())
    # the walk starts at the mesh's first triangle: the repair names the reversed third, or, had the volume come out negative, the rest
    assert stats["signableTriangles"] == 576 and stats["flippedTriangles"] in (int(which.sum()), 576 - int(which.sum()))
    assert a["scene"].scene.topology()[0]["flippedTriangles"] == 0
    for k, points in a["sets"].items():
        assert np.array_equal(_host_sides(a, points)[1], _host_sides(b, points)[1]), k


def test_the_spikes_need_the_pseudo_normal():
    assert sc.case("spikes")["face_normal_wrong"] > 0


def test_signed_distance():
    c = sc.case("mixed")
    points = c["sets"]["uniform"]
    T = np.full(len(points), np.inf, np.float32)
    T[::7] = 1e-4                                              # nothing that near
    arrays = c["scene"].arrays()
    recs = engine.nearest_exhaustive(arrays, points, T)
    side = engine.nearest_side_host(arrays, points, recs)
    rec = engine.nearest_to_numpy(recs)
    d = engine.signed_distance(recs, side)
    found = rec["found"] != 0
    assert (~found).sum() >= len(points) // 7 - 1 and (d[~found] == np.float32(99999999.0)).all() and not side[~found].any()
    unknown = found & (side == 0)
    assert unknown.any() and np.isnan(d[unknown]).all()
    known = found & (side != 0)
    assert known.any() and np.array_equal(d[known], rec["dst"][known] * side[known].astype(np.float32))
    assert np.array_equal(engine.signed_distance(rec, side), d, equal_nan=True)


def test_side_host_refuses_what_it_cannot_index():
    c = sc.case("cubes")
    points = c["sets"]["uniform"][:8]
    arrays = c["scene"].arrays()
    recs = engine.nearest_exhaustive(arrays, points)
    recs[3].triIndex = 1 << 20
    with pytest.raises(engine.RtError):
        engine.nearest_side_host(arrays, points, recs)
    with pytest.raises(ValueError):
        engine.nearest_side_host(arrays, points[:4], recs)
    assert len(engine.nearest_side_host(arrays, points[:0], (type(recs[0]) * 0)())) == 0
    assert sf.CAP == 0.02
