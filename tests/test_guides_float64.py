"""The mirror-following guide planes (rt_render_guides, k_guide_follow) against tests/guides_float64.py, the numpy float64
restatement of the contract that shares nothing with the oracle, with `follow` or with the kernels and asks tests/brute_force.py for
every closest hit. tests/test_guides.py holds the kernel to `follow` bit for bit; that would pass if contract, `follow` and kernel
shared a mistake. Here the CPU half holds `follow` (tests/guides_cases.py, over pyoracle.trace_rays) to the restatement and the GPU
half holds Renderer.render_guides to it, its first_hit planes against segment 0 of the float64 chain.

A pixel is compared where it is not fragile (guides_float64's docstring). hit, sphere, front_face, object, material, the triangle
(by its nine corners), bounces and cut must match exactly, a final miss carries RT_MISS_DST exactly, and depth, position, normal,
ray_dir and albedo are held to |got - ref| <= T * max(|ref|, 1e-3) per component.

T_MEASURED, per plane, is the largest distance between the rounded and the exact run of the restatement over the compared pixels
of the cases that share it (the restatement alone: the distances of `follow` and of the kernel are printed and never set it); T is
four times that, rounded up to one significant figure. The hall of mirrors compounds up to eight reflections and has a T of its
own by the same rule rather than loosening the rest. The rounded run moves every hit to the edge of brute_force's worst-case
bounds, a hundred times what a float32 hit is off by, so `follow` and the kernel sit far nearer to the exact run than T.

Measured on the restatement (all 64 x 48 but `tile`; "excluded" is the fragile share, at most 5 % allowed; the counts are compared
pixels), and `follow`'s largest distance over all planes, printed only:

    case          max      excluded  compared, by L                          cut  rounded distance                             follow (largest
                  bounces                                                         depth    position  normal   ray_dir         of the four)
    cornell_0     0        0.13 %    0: 3068                                 75   7.7e-5   2.7e-4    3.9e-4   1.5e-7          2.5e-5
    cornell_1     1        0.13 %    0: 2993, 1: 75                          0    1.8e-4   6.4e-4    3.9e-4   9.2e-4          4.5e-5
    cornell_4     4        0.13 %    0: 2993, 1: 75                          0    1.8e-4   6.4e-4    3.9e-4   9.2e-4          4.5e-5
    hall          8        0.65 %    0: 672, 1: 1306, 2: 568, 3: 297, 4: 89, 33   9.1e-4   9.1e-3    1.0e-2   3.8e-3          4.6e-5
                                     5: 41, 6: 24, 7: 10, 8: 45
    bunny         4        0.16 %    0: 2932, 1: 129, 2: 5, 3: 1             0    3.8e-4   8.5e-4    2.7e-3   6.5e-6          5.2e-4
    metal_map     4        0.16 %    0: 2968, 1: 99                          0    6.6e-5   3.4e-4    2.2e-6   1.5e-7          1.7e-6
    metal_no_map  4        0.16 %    0: 3067                                 0    6.6e-5   3.4e-4    2.2e-6   1.5e-7          1.7e-6
    placed        4        1.40 %    0: 2718, 1: 295, 2: 11, 3: 1, 4: 4      3    9.0e-5   3.6e-4    2.2e-6   9.3e-6          1.3e-6
    tile          4        0.11 %    0: 893, 1: 21 (of 15 rows x 61)         0    1.2e-4   3.4e-4    2.0e-4   4.6e-4          4.5e-5
    dim_mirror    4        0.13 %    0: 2993, 1: 75                          0    1.8e-4   6.4e-4    3.9e-4   9.2e-4          4.5e-5

The albedo's distance is 0 everywhere (no run rounds a material's constant), so its T is 0: an exact match. T_MEASURED and T:

              depth              position           normal             ray_dir            albedo
    shared    3.77e-4 -> 2e-3    8.47e-4 -> 4e-3    2.71e-3 -> 2e-2    9.23e-4 -> 4e-3    0 -> 0
    hall      9.14e-4 -> 4e-3    9.07e-3 -> 4e-2    1.03e-2 -> 5e-2    3.81e-3 -> 2e-2    0 -> 0

Of the hall's 45 compared chains with L = 8, 33 are cut and 12 end on their ninth segment; no chain is cut with L < 8. The `placed`
case looks from (0, -0.3, -2.2), nearer than the default camera, chosen on the restatement alone so that the placed bunny gives
more than 100 chains. dim_mirror is not in the list the work started from: the mirror's reflectance is 0.25 there, which tells
`reflectance != 0` from a threshold. DESIGN.md, "Mirror-following guide planes", lists the mutations of `follow` these cases catch.
On the MI355X the kernel's largest distance is 1.8e-4 (the bunny's normal), the hall's 1.0e-4.
"""
import os

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine
import brute_force as bf
import guides_float64 as gf
from aov_cases import _upload
from closest_hit_cases import _corners_of
from guides_cases import HALL_CAMERA, MIRROR, as_guides, camera_rays, follow, hall_of_mirrors, metal_quad
from util import EditedScene, cornell_scene, model_scene

MAX_FRAGILE = 0.05
# largest rounded-to-exact distance of the restatement per plane (the table above); the albedo of these scenes is a material's constant,
# which no run rounds: distance 0, T = 0, an exact match
T_MEASURED = dict(shared=dict(depth=3.77e-4, position=8.47e-4, normal=2.71e-3, ray_dir=9.23e-4, albedo=0.0),
                  hall=dict(depth=9.14e-4, position=9.07e-3, normal=1.03e-2, ray_dir=3.81e-3, albedo=0.0))
T = dict(shared=dict(depth=2e-3, position=4e-3, normal=2e-2, ray_dir=4e-3, albedo=0.0),
         hall=dict(depth=4e-3, position=4e-2, normal=5e-2, ray_dir=2e-2, albedo=0.0))
CASES = ("cornell_0", "cornell_1", "cornell_4", "hall", "bunny", "metal_map", "metal_no_map", "placed", "tile", "dim_mirror")
OWN_T = ("hall",)
PLACED_CAMERA = dict(pos=(0.0, -0.3, -2.2))   # nearer than the default: the placed bunny fills a tenth of the frame (chosen on the restatement alone)


def _placed_mirror():
    """The placement of tests/test_shade_coresident.py's _placed_mesh (a rotation about all three axes and an uneven scale), with
    the mirror material: the normal goes through the forward matrix, and dst is the world parameter under a matrix that scales."""
    s = cornell_scene(False)
    s.read_obj(os.path.join(engine.ASSET_DIR, "bunny.obj"),
               engine.placement(position=(0.1, 0.5, 0.0), rotation=(20.0, 35.0, 10.0), scale=(0.5, 0.7, 0.6), samplerIndex=1), MIRROR)
    return s


def _dim_mirror():
    """cornell_scene(True) with the mirror material's reflectance turned down to 0.25: still a mirror (reflectance != 0). Not in the
    list the work started from: without it no case tells `reflectance != 0` from a threshold (every other mirror has reflectance 1)."""
    ed = EditedScene(cornell_scene(True))
    ed.materials[MIRROR].reflectance = 0.25
    return ed


def _constants(name):
    """(scene, textures or None, push-constant keywords, W, H, max_bounces, tile keywords)."""
    if name.startswith("cornell_"):
        return cornell_scene(True), None, {}, 64, 48, int(name[-1]), {}
    if name == "hall":
        return hall_of_mirrors(), None, HALL_CAMERA, 64, 48, 8, {}
    if name == "bunny":
        return model_scene("bunny.obj", material=MIRROR, spheres=True), None, {}, 64, 48, 4, {}
    if name == "metal_map":
        s, _, tex = metal_quad()
        return s, tex, {}, 64, 48, 4, {}
    if name == "metal_no_map":
        return metal_quad()[0], None, {}, 64, 48, 4, {}
    if name == "placed":
        return _placed_mirror(), None, PLACED_CAMERA, 64, 48, 4, {}
    if name == "tile":
        return cornell_scene(True), None, {}, 61, 45, 4, dict(row0=1, rowStride=3)
    if name == "dim_mirror":
        return _dim_mirror(), None, {}, 64, 48, 4, {}
    raise KeyError(name)


def _brute(s, tex):
    """The BruteScene of a Scene or of an EditedScene (whose objects' materials and materials' reflectances were edited)."""
    plain = s.scene if isinstance(s, EditedScene) else s
    bs = bf.BruteScene.from_numpy(plain.numpy())
    if isinstance(s, EditedScene):
        for i in range(s.nObjects):
            bs.objects[i][2] = int(s.objects[i].materialIndex)
        for i in range(s.nMaterials):
            bs.material_table["reflectance"][i] = bs.materials[i]["reflectance"] = float(s.materials[i].reflectance)
    if tex is not None:
        bs.set_textures(tex)
    return bs


_cache = {}


def _case(name):
    """The scene, its constants and the restatement's Study, once per session."""
    if name not in _cache:
        s, tex, kw, W, H, mb, tile = _constants(name)
        pc = engine.push_constants(W, H, **kw)
        rows = np.arange(H)[tile["row0"]::tile["rowStride"]] if tile else None
        study = gf.Study(gf.GuideEstimator(_brute(s, tex), pc, W, H, mb, maps=tex is not None, rows=rows))
        plain = s.scene if isinstance(s, EditedScene) else s
        _cache[name] = dict(scene=s, textures=tex, pc=pc, W=W, H=H, mb=mb, tile=tile, rows=rows, study=study, corners_of=_corners_of(plain),
                            shape=(H if rows is None else len(rows), W))
    return _cache[name]


def _group(name):
    return name if name in OWN_T else "shared"


def _conditions(name):
    """The conditions on the restatement alone: the cap on fragile pixels and the floors the case is there for."""
    c = _case(name)
    st = c["study"]
    L, cut, n = st.bounces, st.cut, st.count
    print(f"[{name}] pixels {len(L)}  fragile {st.excluded:.2%}  compared per L {st.per_L()}  cut {n(cut)}  rounded distance " +
          "  ".join(f"{k} {v:.2e}" for k, v in st.rounded_distance.items()))
    assert st.excluded <= MAX_FRAGILE, (name, st.excluded)
    mirror0 = st.exact.first["hit"] & (st.exact.codes[:, 0] >> 4 & 1).astype(bool)
    if name == "cornell_0":
        assert not L.any() and np.array_equal(cut, mirror0) and n(cut) >= 50, "max_bounces = 0: L = 0 and cut on every mirror hit"
    if name in ("cornell_1", "cornell_4", "tile", "dim_mirror"):
        assert n(L >= 1) >= (50 if name != "tile" else 15), (name, n(L >= 1))
    if name == "hall":
        assert n(L >= 1) >= 1000 and n(L >= 2) >= 500 and n(cut & (L == 8)) >= 20 and not (cut & (L < 8)).any(), st.per_L()
    if name in ("bunny", "placed"):
        assert n(L >= 1) >= 100, (name, n(L >= 1))
    if name.startswith("metal"):
        quad = st.exact.first["hit"] & (st.exact.first["material"] == metal_quad()[1])
        if name == "metal_map":
            assert n(quad & (L == 1)) >= 80 and n(quad & (L == 0)) >= 80, (n(quad & (L == 1)), n(quad & (L == 0)))
        else:
            assert n(quad) >= 160 and not L.any() and not cut.any()
    for k, v in st.rounded_distance.items():
        assert v <= T[_group(name)][k] / 4, (name, k, v)
    return c


def _check(name, what, got, record, chain=None):
    """One set of planes (render_guides' dict) against a record of the exact run."""
    c = _case(name)
    st = c["study"]
    bad, dist = gf.disagreements(gf.flat(got), record, st.compared, c["corners_of"], chain)
    print(f"[{name}] {what}: compared {int(st.compared.sum())} of {st.compared.size}  " + "  ".join(f"{k} {v:.2e}" for k, v in dist.items()))
    assert not bad, f"{name} {what}: {bad} differ on compared pixels"
    for k, v in dist.items():
        assert v <= T[_group(name)][k], f"{name} {what}: {k} is {v:.3e} from the float64 chain, {T[_group(name)][k]} allowed"
    return dist


# ---------------------------------------------------------------------------------------------------------------- CPU half
@pytest.mark.parametrize("name", CASES)
def test_conditions_on_the_restatement(name):
    _conditions(name)


def test_T_is_four_times_the_measured_distance():
    own = {n: _case(n)["study"].rounded_distance for n in CASES}
    for group in T:
        worst = {k: max(own[n][k] for n in CASES if _group(n) == group) for k in gf.TOLERANCED}
        print(f"[{group}] largest rounded distances " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
        for k, v in worst.items():
            m, t = T_MEASURED[group][k], T[group][k]
            # the recorded figure is this measurement (to the few per cent another numpy's float32 functions may move it) ...
            assert 0.9 * m <= v <= 1.1 * m, f"T_MEASURED[{group}][{k}] is out of date: {v:.3e}"
            # ... and T is four times the record, rounded up to one significant figure: at most twice that
            assert 4 * m <= t <= 8 * m and 4 * v <= t, (group, k)
    assert any(4 * own["hall"][k] > T["shared"][k] for k in gf.TOLERANCED), "the hall no longer needs a T of its own"


@pytest.mark.parametrize("name", CASES)
def test_follow_against_float64(name):
    """`follow` over the oracle's calculateIntersections, on the float64 camera's rays rounded to float32."""
    c = _conditions(name)
    o, d = camera_rays(c["pc"], c["W"], c["H"])
    if c["rows"] is not None:
        keep = (c["rows"][:, None] * c["W"] + np.arange(c["W"])[None, :]).reshape(-1)
        o, d = o[keep], d[keep]
    try:
        pyoracle.set_textures(c["textures"] or [])
        ref = follow(c["scene"], o, d, c["mb"], c["textures"] or ())
    finally:
        pyoracle.set_textures([])
    _check(name, "follow", as_guides(ref, c["shape"], c["scene"]), c["study"].exact.final, c["study"].exact)


# ---------------------------------------------------------------------------------------------------------------- GPU half
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_render_guides_against_float64(renderer, name):
    c = _conditions(name)
    try:
        _upload(renderer, c["scene"])
        renderer.upload_textures(c["textures"] or [])
        g, first = renderer.render_guides(c["pc"], c["W"], c["H"], c["mb"], first_hit=True, **c["tile"])
    finally:
        renderer.upload_textures([])
    assert g["depth"].shape == c["shape"]
    _check(name, "render_guides", g, c["study"].exact.final, c["study"].exact)
    _check(name, "render_guides' first-hit planes", first, c["study"].exact.first)
