"""The ambient-occlusion plane (rt_render_ao: k_ao_rays, k_ao_count, k_ao_resolve; include/rt_ao_rays.h) against tests/ao_float64.py,
the numpy float64 restatement of the rule that shares nothing with the header, the kernels or the oracle and asks
tests/brute_force.py for the first hit and for every occlusion query. tests/test_ray_queries.py and tests/test_ao_rays_host.py hold
the plane to the header's own rays pushed through the device's own occlusion query, and the rays to their distribution's mean: a
wrong sample or seed mix that stays a bijection, a reach ignored or applied to the wrong quantity, or a round dropped from the sum
would pass all of that. Here the CPU half holds the composition "engine.ao_rays on the oracle's first-hit planes ->
pyoracle.trace_rays -> dst < radius" to the restatement, and its directions to the float64 directions within T in angle; the GPU half
holds Renderer.render_ao to it, from the context's own planes and from planes handed over.

A pixel is compared where it is not fragile (ao_float64's docstring). The plane must equal float32(S - k) / float32(S) exactly, and
1.0 exactly where the camera ray misses.

T_MEASURED is the largest angle between the rounded and the exact run's directions of the restatement over the compared pixels of
all cases (the restatement alone; the header's angle is printed and never sets it); T is four times that, rounded up to one
significant figure. The rounded run moves the first hit's normal to the edge of brute_force's worst-case bound.

Measured on the restatement (64 x 48; "excluded" is the fragile share, at most 5 % allowed; the counts are compared hit pixels):

    case              samples  radius  seed  excluded  compared  by k                                           rounded   engine.ao_rays
                                                         hits                                                     angle     (printed only)
    cornell_s1        1        0.3     1     2.15 %    1631      0: 1336, 1: 295                                6.4e-4    2.8e-5
    cornell_s4        4        0.3     1     2.44 %    1622      0: 958, 1: 314, 2: 214, 3: 109, 4: 27          7.6e-4    3.5e-5
    cornell_s4_seed2  4        0.3     2     2.34 %    1625      0: 980, 1: 290, 2: 213, 3: 114, 4: 28          7.3e-4    3.4e-5
    cornell_s8        8        0.15    1     2.57 %    1618      0: 1231, 1: 116, 2: 107, 3: 83, 4: 42, 5: 21,  7.6e-4    3.5e-5
                                                                 6: 6, 7: 9, 8: 3
    bunny_s4          4        0.3     1     2.47 %    1621      0: 1007, 1: 312, 2: 209, 3: 79, 4: 14          6.0e-6    4.2e-7

T_MEASURED = 7.65e-4 rad, T = 4e-3 rad. 1697 of the 3072 camera rays hit. Nearly all of the fragile share is brute_force's verdict on
a query (a sample's ray that grazes a wall's edge or starts in a corner); one pixel has a sample within 1e-4 of the reach and none
has a fragile axis choice (the walls' normals are exact). The oracle's composition and, on the MI355X, both routes of
Renderer.render_ao agree with the float64 plane on every pixel, the fragile ones included. DESIGN.md, "Ambient-occlusion plane",
lists the mutations these cases catch.
"""
import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine
import ao_float64 as ao
import brute_force as bf
from ao_cases import oracle_planes
from util import cornell_scene, model_scene

W, H = 64, 48
MAX_FRAGILE = 0.05
MIN_COMPARED_HITS = 1000
T_MEASURED = 7.65e-4    # radians: largest rounded-to-exact angle of the restatement over the compared pixels of all cases
T = 4e-3                # 4 x T_MEASURED, rounded up to one significant figure
#        name              scene      samples radius seed
CASES = {"cornell_s1": ("cornell", 1, 0.3, 1), "cornell_s4": ("cornell", 4, 0.3, 1), "cornell_s4_seed2": ("cornell", 4, 0.3, 2),
         "cornell_s8": ("cornell", 8, 0.15, 1), "bunny_s4": ("bunny", 4, 0.3, 1)}
_scenes, _cache = {}, {}


def _scene(which):
    if which not in _scenes:
        s = cornell_scene(True) if which == "cornell" else model_scene("bunny.obj")
        _scenes[which] = (s, bf.BruteScene.from_numpy(s.numpy()))
    return _scenes[which]


def _case(name):
    """The scene, the constants and the restatement's Study, once per session."""
    if name not in _cache:
        which, samples, radius, seed = CASES[name]
        s, bs = _scene(which)
        pc = engine.push_constants(W, H)
        _cache[name] = dict(scene=s, which=which, pc=pc, samples=samples, radius=radius, seed=seed,
                            study=ao.Study(ao.AmbientOcclusion(bs, pc, W, H, samples, radius, seed)))
    return _cache[name]


def _conditions(name):
    """The conditions on the restatement alone: the cap on fragile pixels, the floor on compared hits, every count present."""
    c = _case(name)
    st = c["study"]
    why = {k: float(getattr(st.exact, k).mean()) for k in ("ill", "near_radius", "axis")}
    compared_hits = int((st.compared & st.hit).sum())
    print(f"[{name}] pixels {W * H}  hits {int(st.hit.sum())}  fragile {st.excluded:.2%} (own: " + ", ".join(f"{k} {v:.2%}" for k, v in why.items()) +
          f")  compared hits {compared_hits}  per k {st.per_k()}  rounded angle {st.rounded_angle:.2e}")
    assert st.excluded <= MAX_FRAGILE, (name, st.excluded)
    assert compared_hits >= MIN_COMPARED_HITS and (st.compared & ~st.hit).any(), (name, compared_hits)
    if c["samples"] <= 4:
        assert all(v > 0 for v in st.per_k().values()), (name, st.per_k())
    assert st.rounded_angle <= T / 4, (name, st.rounded_angle)
    return c


def _check_plane(name, what, plane, st):
    got = np.asarray(plane).reshape(-1)
    assert got.dtype == np.float32 and got.shape == st.plane.shape
    wrong = st.compared & (got != st.plane)
    everywhere = int((got != st.plane).sum())
    print(f"[{name}] {what}: compared {int(st.compared.sum())} of {st.compared.size}, {int(wrong.sum())} differ (fragile pixels included: {everywhere})")
    assert np.all(got[st.compared & ~st.hit] == 1.0), f"{name} {what}: a miss is not 1"
    assert not wrong.any(), f"{name} {what}: {int(wrong.sum())} compared pixels differ from float32(S - k) / float32(S), the first at {np.flatnonzero(wrong)[:5].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- CPU half
@pytest.mark.parametrize("name", CASES)
def test_conditions_on_the_restatement(name):
    _conditions(name)


def test_T_is_four_times_the_measured_angle():
    own = {n: _case(n)["study"].rounded_angle for n in CASES}
    worst = max(own.values())
    print(f"largest rounded angle {worst:.3e}; T_MEASURED {T_MEASURED}, T {T}; " + "  ".join(f"{n} {v:.2e}" for n, v in own.items()))
    # the recorded figure is this measurement (to the few per cent another numpy's float32 sin, cos and sqrt may move it) ...
    assert 0.9 * T_MEASURED <= worst <= 1.1 * T_MEASURED, "T_MEASURED is out of date: measure again and set T to four times it"
    # ... and T is four times the record, rounded up to one significant figure: at most twice that
    assert 4 * T_MEASURED <= T <= 8 * T_MEASURED and 4 * worst <= T


def test_the_state_by_hand():
    """rt_ao_state for one (record, sample, seed) from the formula by hand in Python's integers, and what it must tell apart."""
    i, s, seed = 1234, 3, 2
    h = (i * 747796405 + 2891336453) % 2 ** 32
    h ^= s
    h = (h * 747796405 + 2891336453) % 2 ** 32
    h ^= (seed * 2654435769) % 2 ** 32
    assert int(ao.ao_state(np.array([i]), s, seed)[0]) == h
    idx = np.arange(W * H)
    states = np.stack([ao.ao_state(idx, s, seed) for s in range(4) for seed in (1, 2)])
    assert len(np.unique(states)) == states.size


_planes = {}


@pytest.mark.parametrize("name", CASES)
def test_ao_rays_through_the_oracle_against_float64(name):
    """engine.ao_rays on the oracle's first-hit planes -> pyoracle.trace_rays -> dst < radius, summed over the samples."""
    c = _conditions(name)
    st, S, radius = c["study"], c["samples"], np.float32(c["radius"])
    if c["which"] not in _planes:
        _planes[c["which"]] = oracle_planes(c["scene"], c["pc"], W, H)
    planes = _planes[c["which"]]
    hit = planes["hit"].reshape(-1)
    assert np.array_equal(hit[st.compared], st.hit[st.compared])
    k = np.zeros(W * H, np.uint32)
    worst = 0.0
    for s in range(S):
        o, d, valid = engine.ao_rays(planes, s, samples=S, radius=c["radius"], seed=c["seed"])
        assert np.array_equal(valid, hit)
        r = engine.hits_to_numpy(pyoracle.trace_rays(c["scene"], o[valid], d[valid]))
        k[valid] += (r["didHit"] == 1) & (r["dst"] < radius)
        m = st.compared & st.hit & hit
        worst = max(worst, ao.angle(d[m][:, None], st.exact.dirs[m, s][:, None], np.ones(int(m.sum()), bool)))
    print(f"[{name}] engine.ao_rays: largest angle to the float64 direction {worst:.2e} (T = {T:.0e})")
    assert worst <= T, f"{name}: a direction of engine.ao_rays is {worst:.3e} rad from the float64 rule's, {T} allowed"
    plane = np.where(hit, (np.float32(S) - k.astype(np.float32)) / np.float32(S), np.float32(1)).astype(np.float32)
    _check_plane(name, "ao_rays through the oracle", plane, st)


# ---------------------------------------------------------------------------------------------------------------- GPU half
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_render_ao_against_float64(renderer, name):
    c = _conditions(name)
    renderer.upload_textures([])
    renderer.upload_scene(c["scene"])
    a = renderer.render_aovs(c["pc"], W, H)
    kw = dict(samples=c["samples"], radius=c["radius"], seed=c["seed"])
    own = renderer.render_ao(**kw)
    assert own.shape == (H, W)
    _check_plane(name, "render_ao, the context's planes", own, c["study"])
    _check_plane(name, "render_ao, planes handed over", renderer.render_ao(a, **kw), c["study"])
