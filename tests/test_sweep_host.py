"""The sphere sweeps on the CPU (rt_query_sweep's host-only unit ray_tracer_amd/csrc/sweep_queries.h, the rule include/rt_sweep.h,
and the exhaustive host loop rt_sweep_exhaustive_host; engine.sweep_exhaustive).

tests/sweep_check.cpp, built with plain g++ under the sanitizers as a stand-alone program, provokes every refusal with made-up
addresses, in the stated order, with its message; covers the block and byte arithmetic, the stack choice, the part layout of the
_host form, and the rule on hand cases against their closed forms.

The loop is then pinned to tests/sweep_float64.py, a numpy float64 brute force that shares nothing with the header, on every scene
and ray set of tests/sweep_cases.py, by a bracket with no ray excluded: the contact time never increases with the radius, so with
delta the derived fp32 bound of the ray the fp32 `found` must be 1 where float64 finds a contact at R - delta, 0 where it finds none
at R + delta, and t must lie in [t64(R + delta) - tau, t64(R - delta) + tau]. So that the bracket cannot be vacuous, rays whose
`found` it leaves undecided are at most 2 % of any set, and the median bracket width of decided rays is at most 1e-3 of the median
t: both are properties of the reference and the radii alone. Every found record is held to itself as well: point is w a + u b + v c
of the reported triangle, |centre - point| agrees with gap, normal is unit, gap <= R + delta."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
import nearest_float64 as nf
import sweep_cases as sc
import sweep_float64 as sf

UNDECIDED_CAP = 0.02
WIDTH_CAP = 1e-3


def raw(recs, n):
    return np.frombuffer(recs, dtype=np.uint8).reshape(n, 64) if n else np.zeros((0, 64), np.uint8)


def is_not_found(rows):
    want = np.zeros(16, np.uint32)
    want[0] = np.float32(99999999.0).view(np.uint32)
    return (rows.view(np.uint32).reshape(-1, 16) == want).all(axis=1)


def test_refusals_arithmetic_and_the_rule_on_hand_cases(tmp_path, built):
    exe = hostcheck.build(tmp_path, "sweep_check", ["sweep_queries.cpp", "point_queries.cpp", "host_staging.cpp"], "sweep_check.cpp", opt="-O1")
    hostcheck.run(exe, ok="sweep ok")


def check_records(ns, s, rec, dl, what):
    """Every found record against itself and the float64 scene."""
    f = rec["found"].astype(bool)
    R = s["R"].astype(np.float64)
    centre32 = (s["o"] + rec["t"][:, None] * s["d"]).astype(np.float64)       # fl(o + t d), the product and the sum rounded as the rule rounds them
    p, gap = rec["point"].astype(np.float64), rec["gap"].astype(np.float64)
    assert (np.abs(np.linalg.norm(centre32 - p, axis=1) - gap)[f] <= dl[f]).all(), f"{what}: |centre - point| does not agree with gap"
    assert (np.abs(np.linalg.norm(rec["normal"].astype(np.float64), axis=1) - 1.0)[f] <= 4 * sf.U32).all(), f"{what}: normal is not unit"
    assert (gap[f] <= (R + dl)[f]).all(), f"{what}: gap up to {float(((gap - R) / dl)[f].max()):.3g} delta above R"
    assert (rec["startsInContact"][f] == (rec["t"][f] == 0)).all() and (rec["t"][f] >= 0).all()
    sph = rec["isSphere"].astype(bool) & f
    tri = f & ~sph
    assert (rec["uv"][sph] == 0).all() and (rec["triIndex"][sph] == 0).all()
    # the centre lies within R + delta of the primitive the record names in float64, and point on it
    idx = np.flatnonzero(f)
    d_own, _, W = nf.distance_to_reported(ns, centre32[idx], sph[idx], rec["objectIndex"][idx], rec["triIndex"][idx])
    assert (d_own <= (R + dl)[idx]).all(), f"{what}: the centre at t is up to {float(((d_own - R[idx]) / dl[idx]).max()):.3g} delta from the reported primitive"
    u, v = rec["uv"][idx, 0].astype(np.float64), rec["uv"][idx, 1].astype(np.float64)
    rebuilt = (1 - u - v)[:, None] * W[:, 0] + u[:, None] * W[:, 1] + v[:, None] * W[:, 2]
    mesh = tri[idx]
    assert (np.linalg.norm(rebuilt - p[idx], axis=1)[mesh] <= dl[idx][mesh]).all(), f"{what}: point is not w a + u b + v c of the reported triangle"
    assert (u[mesh] >= 0).all() and (v[mesh] >= 0).all() and ((u + v)[mesh] <= 1 + 4 * sf.U32).all()
    return float(((gap - R) / dl)[f].max()) if f.any() else -np.inf


@pytest.mark.parametrize("name", sc.SCENES)
def test_exhaustive_host_lies_in_the_float64_bracket(name):
    c = sc.case(name)
    arrays, ns = c["scene"].arrays(), c["ns"]
    worst_late = worst_early = worst_gap = -np.inf
    for key, s in c["sets"].items():
        what = f"{name}/{key}"
        n = len(s["o"])
        br = sc.bracket(name, key)
        lo, hi, dl = br["lo"], br["hi"], br["delta"]
        assert (lo <= hi).all(), f"{what}: the reference's contact time increases with the radius"
        rec = engine.sweep_to_numpy(engine.sweep_exhaustive(arrays, s["o"], s["d"], s["R"]))
        found = rec["found"].astype(bool)
        must, never = np.isfinite(hi), ~np.isfinite(lo)
        undecided = ~must & ~never
        decided = must
        width = hi[decided] - lo[decided]
        t64 = hi[decided]
        print(f"{what:24s} found {int(found.sum()):4d}/{n}  undecided {int(undecided.sum()):3d}  median t {np.median(t64) if len(t64) else 0:.4g}  median width {np.median(width) if len(width) else 0:.3g}"
              f"  median delta/R {float(np.median(dl / s['R'])):.2g}")
        assert undecided.sum() <= UNDECIDED_CAP * n, f"{what}: the bracket leaves {int(undecided.sum())} of {n} rays undecided"
        if len(width):
            assert np.median(width) <= WIDTH_CAP * np.median(t64), f"{what}: median bracket width {np.median(width):.3g} against a median t of {np.median(t64):.3g}"
        assert found[must].all(), f"{what}: rays {np.flatnonzero(must & ~found)[:5].tolist()} found nothing where float64 finds a contact at R - delta"
        assert not found[never].any(), f"{what}: rays {np.flatnonzero(never & found)[:5].tolist()} found something where float64 finds none at R + delta"
        assert is_not_found(raw(engine.sweep_exhaustive(arrays, s["o"], s["d"], s["R"]), n)[~found]).all()
        t = rec["t"].astype(np.float64)
        tau_lo = sf.tau(ns, s["d"], s["R"], np.where(np.isfinite(lo), lo, 0.0))
        tau_hi = sf.tau(ns, s["d"], s["R"], np.where(np.isfinite(hi), hi, 0.0))
        early, late = ((lo - t) / tau_lo)[found], ((t - hi) / tau_hi)[found & must]
        print(f"{'':24s} (t64(R + delta) - t) / tau up to {early.max() if len(early) else -np.inf:.3g}, (t - t64(R - delta)) / tau up to {late.max() if len(late) else -np.inf:.3g}")
        assert (early <= 1).all(), f"{what}: t up to {early.max():.3g} tau before t64(R + delta)"
        assert (late <= 1).all(), f"{what}: t up to {late.max():.3g} tau after t64(R - delta)"
        worst_early, worst_late = max(worst_early, early.max() if len(early) else -np.inf), max(worst_late, late.max() if len(late) else -np.inf)
        worst_gap = max(worst_gap, check_records(ns, s, rec, dl, what))
    print(f"{name}: OBSERVED late {worst_late:.3g} tau, early {worst_early:.3g} tau, gap - R {worst_gap:.3g} delta")


def test_a_limit_cuts_the_unlimited_answer():
    for name in ("cornell", "spheres"):
        c = sc.case(name)
        s = c["sets"]["aimed"]
        n = len(s["o"])
        free = raw(engine.sweep_exhaustive(c["scene"].arrays(), s["o"], s["d"], s["R"]), n).copy()
        t = free.view(np.float32).reshape(n, 16)[:, 0]
        found = free.view(np.uint32).reshape(n, 16)[:, 1] == 1
        T = np.where(found, t * np.resize(np.array([0.5, 1.0, 1.5, 2.0], np.float32), n), np.float32(1.0)).astype(np.float32)
        T[T <= 0] = 1.0
        cut = raw(engine.sweep_exhaustive(c["scene"].arrays(), s["o"], s["d"], s["R"], T), n)
        keep = found & (t < T)
        assert np.array_equal(cut[keep], free[keep]) and is_not_found(cut[~keep]).all() and keep.any() and (found & ~keep).any()


def test_degenerate_radii_limits_and_directions_find_nothing():
    c = sc.case("cornell")
    s = c["sets"]["contact"]
    n = 64
    o, d, R = s["o"][:n], s["d"][:n].copy(), s["R"][:n].copy()
    bad = np.resize(np.array([0.0, -0.0, -1.0, np.nan, np.inf], np.float32), n)
    assert is_not_found(raw(engine.sweep_exhaustive(c["scene"].arrays(), o, d, bad), n)).all()
    limits = np.resize(np.array([0.0, -0.0, -1.0, np.nan], np.float32), n)
    assert is_not_found(raw(engine.sweep_exhaustive(c["scene"].arrays(), o, d, R, limits), n)).all()
    assert is_not_found(raw(engine.sweep_exhaustive(c["scene"].arrays(), o, np.zeros_like(d), R), n)).all()
    d[:, 0] = np.inf
    assert is_not_found(raw(engine.sweep_exhaustive(c["scene"].arrays(), o, d, R), n)).all()
    # and the same rays with sound arguments all start in contact
    rec = engine.sweep_to_numpy(engine.sweep_exhaustive(c["scene"].arrays(), o, s["d"][:n], R))
    assert rec["found"].all() and (rec["t"] == 0).all() and rec["startsInContact"].all()


def test_the_python_side_refuses_what_the_loop_refuses():
    c = sc.case("spheres")
    s = c["sets"]["far"]
    with pytest.raises(ValueError):
        engine.sweep_exhaustive(c["scene"].arrays(), s["o"], s["d"], s["R"][:5])
    with pytest.raises(ValueError):
        engine.sweep_exhaustive(c["scene"].arrays(), s["o"], s["d"], None)
    with pytest.raises(ValueError):
        engine.sweep_exhaustive(c["scene"].arrays(), s["o"], s["d"][:5], s["R"])
    assert len(engine.sweep_exhaustive(c["scene"].arrays(), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32))) == 0
