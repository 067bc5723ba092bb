"""The baked-light queries' host-only unit and rule on the CPU (ray_tracer_amd/csrc/irradiance_queries.h, include/rt_irradiance.h):
tests/irradiance_check.cpp provokes every refusal with made-up addresses, in the stated order, with its message, covers the points
with chunks for n x S straddling the piece cap (S equal to the cap; cap + 1 is refused), checks the rays' ids and origins and
the gather's summation order against a fold written out as a tree, for S = 1, 5, 64, 65, 200 with records whose sum depends on
the order. Then the host forms (engine.irradiance_rays, engine.irradiance_gather) are held to the float64 restatement of
tests/irradiance_float64.py within the bounds its docstring derives; the largest fraction of each bound is printed (DESIGN.md,
"Irradiance and SH probes", quotes them)."""
import math

import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
import irradiance_float64 as f64

SAMPLES = (1, 5, 64, 65, 200)
FRAMES = (0, 3)


def test_irradiance_query_checks_on_the_cpu(tmp_path, built):
    """irradiance_queries.cpp + radiance_queries.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan
    and UBSan where they are installed."""
    exe = hostcheck.build(tmp_path, "irradiance_check", ["irradiance_queries.cpp", "radiance_queries.cpp"], "irradiance_check.cpp", rocm=False)
    hostcheck.run(exe, ok="irradiance queries ok")


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _points():
    """Seven points with normals along the axes (both branches of the frame's axis choice) and oblique, and ids that wrap."""
    normals = _unit([(0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0.6, 0, -0.8), (1, 2, 3), (-0.3, 0.9, 0.1)])
    points = np.array([(0.5, -0.25, 2), (-1, 3, 0.125), (7, 8, 9), (0, 0, 0), (-2.5, 0.1, 0.3), (1e-3, 5, -4), (100, -50, 25)], np.float32)
    ids = np.array([0, 1, 7, 0xFFFFFFFF, 0x33333334, 123456789, 42], np.uint32)
    return points, normals, ids


def test_rays_agree_with_the_float64_restatement(built):
    """rt_irradiance_rays_host against irradiance_float64's directions and origins, both forms, within the per-sample bound derived
    there (the roundings of r1, r2, sincos, the square roots and the frame about n): not fitted."""
    points, normals, ids = _points()
    worst = dict(cosine=0.0, sphere=0.0, origin=0.0)
    for S in SAMPLES + (4096,):
        for frame in FRAMES:
            o, d, rid = engine.irradiance_rays(points, normals, samples=S, ids=ids, frame=frame, bias=1e-5)
            os_, ds, rids = engine.irradiance_rays(points, None, samples=S, ids=ids, frame=frame)
            assert d.shape == (len(points) * S, 3) and np.array_equal(rid, rids)
            want_o, bound_o = f64.origins(points, normals, 1e-5)
            for i in range(len(points)):
                rows = slice(i * S, (i + 1) * S)
                assert np.array_equal(rid[rows], ((int(ids[i]) * S + np.arange(S)) & 0xFFFFFFFF).astype(np.uint32))
                assert np.array_equal(os_[rows], np.repeat(points[i][None], S, 0))
                err = np.abs(o[rows].astype(np.float64) - want_o[i][None])
                assert (err <= bound_o[i][None]).all()
                worst["origin"] = max(worst["origin"], float((err / bound_o[i][None]).max()))
                for form, got, (want, bound) in (("cosine", d[rows], f64.cosine_dirs(normals[i], ids[i], frame, S)),
                                                 ("sphere", ds[rows], f64.sphere_dirs(ids[i], frame, S))):
                    err = np.abs(got.astype(np.float64) - want).max(axis=1)
                    bad = np.flatnonzero(err > bound)
                    assert not len(bad), f"{form}, S {S}, frame {frame}, point {i}: sample {bad[:3].tolist()} off by {err[bad[:3]].tolist()}, bound {bound[bad[:3]].tolist()}"
                    worst[form] = max(worst[form], float((err / bound).max()))
    print("largest fraction of the bound:", worst)
    assert all(0.0 < w <= 1.0 for w in worst.values())


def _records(n, S, seed):
    """fp32 radiance records of mixed magnitude, with the magenta of a NaN path among them."""
    rng = np.random.default_rng(seed)
    rad = np.ones((n * S, 4), np.float32)
    rad[:, :3] = (rng.random((n * S, 3)) ** 4 * 50.0).astype(np.float32)
    rad[::17, :3] = (1.0, 0.0, 1.0)
    return rad


def test_gather_agrees_with_a_float64_sum(built):
    """rt_irradiance_gather_host against float64 sums of the same fp32 records: within (fold depth 6 + ceil(S / 64) + the scale's 3
    roundings) u sum |term| for the irradiance; the probes' terms carry their directions' bound as well."""
    _, _, ids = _points()
    n = len(ids)
    worst = dict(irradiance=0.0, probes=0.0)
    for S in SAMPLES:
        rad = _records(n, S, S)
        E = engine.irradiance_gather(rad, n, samples=S, ids=ids, frame=3)
        want, bound = f64.irradiance(rad, n, S)
        assert E.shape == (n, 4) and E.dtype == np.float32 and (E[:, 3] == 1.0).all()
        err = np.abs(E[:, :3].astype(np.float64) - want)
        assert (err <= bound).all(), (S, err.max(), bound.min())
        worst["irradiance"] = max(worst["irradiance"], float((err / bound).max()))
        c = engine.irradiance_gather(rad, n, samples=S, ids=ids, frame=3, sphere=True)
        want, bound = f64.probes(rad, ids, 3, n, S)
        assert c.shape == (n, 9, 3)
        err = np.abs(c.astype(np.float64) - want)
        assert (err <= bound).all(), (S, np.argwhere(err > bound)[:3].tolist())
        worst["probes"] = max(worst["probes"], float((err / bound).max()))
    print("largest fraction of the bound:", worst)
    assert all(0.0 < w <= 1.0 for w in worst.values())


def test_constant_radiance_pins_the_densities(built):
    """S = 4096 and a constant L: the cosine form gives E = pi L and the sphere form c_0 = 2 sqrt(pi) L within the derived bounds
    (no statistical tolerance: a constant has no variance), and c_1..c_8 equal the restatement's projection of its own directions,
    which are small (the set is stratified) but not zero."""
    S, n = 4096, 2
    L = np.array((0.75, 2.0, 0.125), np.float32)
    rad = np.ones((n * S, 4), np.float32)
    rad[:, :3] = L
    ids = np.array([5, 0xFFFFFFF0], np.uint32)
    E = engine.irradiance_gather(rad, n, samples=S, ids=ids)
    _, bound = f64.irradiance(rad, n, S)
    assert (np.abs(E[:, :3] - math.pi * L.astype(np.float64)) <= bound).all()
    c = engine.irradiance_gather(rad, n, samples=S, ids=ids, sphere=True)
    want, bound = f64.probes(rad, ids, 0, n, S)
    assert (np.abs(c - want) <= bound).all()
    assert (np.abs(c[:, 0] - 2.0 * math.sqrt(math.pi) * L.astype(np.float64)) <= bound[:, 0]).all()
    assert (np.abs(want[:, 0] - 2.0 * math.sqrt(math.pi) * L.astype(np.float64)) < 1e-12).all()
    assert (np.abs(want[:, 1:]) < 0.02 * L.max()).all() and np.abs(want[:, 1:]).max() > 0.0


def test_progressive_gather_blends_with_the_previous_result(built):
    n, S = 3, 65
    a, b = _records(n, S, 1), _records(n, S, 2)
    for sphere in (False, True):
        first = engine.irradiance_gather(a, n, samples=S, frame=0, sphere=sphere)
        assert np.array_equal(engine.irradiance_gather(a, n, samples=S, frame=0, sphere=sphere, progressive=True, out=np.full_like(first, 9.0))[..., :3], first[..., :3])
        second = engine.irradiance_gather(b, n, samples=S, frame=1, sphere=sphere)
        got = engine.irradiance_gather(b, n, samples=S, frame=1, sphere=sphere, progressive=True, out=first)
        w = np.float32(1.0) / (np.float32(1.0) + np.float32(1.0))
        want = first * (np.float32(1.0) - w) + second * w
        if not sphere:
            want[:, 3] = 1.0
        assert np.array_equal(got, want)


def test_sh9_irradiance_convolves_with_the_cosine_lobe():
    """L(w) = 1 + 0.5 a.w has the coefficients (2 sqrt(pi), 0.5 a / k1, 0...) and the irradiance pi + 0.5 (2 pi / 3) a.n."""
    a = _unit((0.2, -0.7, 0.4)).astype(np.float64)
    k1 = math.sqrt(3.0 / (4.0 * math.pi))
    c = np.zeros((4, 9, 3))
    c[:, 0] = 2.0 * math.sqrt(math.pi)
    c[:, 1], c[:, 2], c[:, 3] = 0.5 * a[1] / k1, 0.5 * a[2] / k1, 0.5 * a[0] / k1
    normals = _unit([(0, -1, 0), (1, 0, 0), (1, 2, 3), (-0.2, 0.7, -0.4)]).astype(np.float64)
    E = engine.sh9_irradiance(c, normals)
    want = math.pi + 0.5 * (2.0 * math.pi / 3.0) * (normals @ a)
    assert E.shape == (4, 3) and np.allclose(E, want[:, None], rtol=3e-6, atol=0)   # (the six-digit constants)
    with pytest.raises(ValueError):
        engine.sh9_irradiance(np.zeros((4, 27)), normals)


def test_host_forms_refuse_what_the_rule_cannot_take(built):
    p, nrm, _ = _points()
    with pytest.raises(engine.RtError):
        engine.irradiance_rays(p, nrm, samples=0)
    with pytest.raises(engine.RtError):
        engine.irradiance_rays(p, nrm, samples=1 << 24, count=0)
    with pytest.raises(engine.RtError):
        engine.irradiance_rays(p, nrm, samples=4, bias=-1.0)
    with pytest.raises(engine.RtError):
        engine.irradiance_rays(p, nrm, samples=4, first=5, count=3)
    with pytest.raises(ValueError):
        engine.irradiance_rays(p, nrm[:3], samples=4)
    with pytest.raises(ValueError):
        engine.irradiance_gather(np.zeros((7, 4), np.float32), 2, samples=4)
