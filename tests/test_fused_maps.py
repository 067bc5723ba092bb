"""The fused pipeline with the alpha, metalness and bump maps (k_render_fused_maps<PIX>, rt_set_tuning "fused_maps" 1).

A scene that binds one of the three maps takes the multi-kernel pipeline by default (k_trace_pw_alpha, k_shade_maps;
tests/test_textures.py pins that). With "fused_maps" 1 it picks its pipeline like any other scene, and the fused one runs
k_render_fused_maps: the fused kernel's loop with the alpha look-up in the traversal's leaf step and the maps' shading, in one
configuration for every map scene (24 LDS stack entries + the overflow buffer, object culling, no top-level table). Every case
here is HIP == oracle bit for bit, pixels and the eight counters, on the kernel the case names, with pixels replaced a block at
a time (pixel_refill 64) and at 8 free lanes."""
import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine

from texture_cases import KEYS, _bound, _grey, _map_set, _plane_material, _same_as_oracle
from util import kernel_instantiations

pytestmark = pytest.mark.gpu

FULL = dict(alphaIndex=1, metalnessIndex=2, bumpIndex=3)
DEFAULTS = {"fused_maps": 0, "pipeline": -1, "pixel_refill": 0, "blocks_per_cu": 0}
LAUNCHED = set()   # k_render_fused_maps<...> instantiations the cases below ran (test_every_maps_instantiation_was_launched)


def maps_instantiations():
    return kernel_instantiations("k_render_fused_maps")


@pytest.fixture
def fused(renderer):
    """fused_maps 1, pipeline 1; afterwards every knob and both texture tables back to their defaults."""
    renderer.set_tuning("fused_maps", 1)
    renderer.set_tuning("pipeline", 1)
    try:
        yield renderer
    finally:
        pyoracle.set_textures([])
        renderer.upload_textures([])
        for k, v in DEFAULTS.items():
            renderer.set_tuning(k, v)


def _fused_same(renderer, s, tex, pc, W, H, what, kernel="k_render_fused_maps<false>"):
    img = _same_as_oracle(renderer, s, tex, pc, W, H, what, kernel, maps=False)
    assert renderer.last_pipeline() == 1, what
    if kernel.startswith("k_render_fused_maps"):
        LAUNCHED.add(kernel)
    return img


REFILL = pytest.mark.parametrize("refill", [64, 8])


@REFILL
def test_each_map_and_all_three_on_the_fused_pipeline(fused, tmp_path, refill):
    """Each map alone and all three, the permuted slots, both samplers, uvs inside and beyond the unit square; and the maps are
    really in the picture."""
    fused.set_tuning("pixel_refill", refill)
    tex = _map_set()
    W, H = 112, 84
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=3, environmentOn=True)
    n = 0
    for sampler in (0, 1):
        for uvs in (1.0, 2.5):
            for slots in (dict(alphaIndex=1), dict(metalnessIndex=2), dict(bumpIndex=3), FULL,
                          dict(alphaIndex=3, metalnessIndex=1, bumpIndex=2, albedoIndex=-1)):
                n += 1
                s = _bound(tmp_path / f"c{n}", sampler, uvs, **slots)
                img = _fused_same(fused, s, tex, pc, W, H, f"sampler {sampler} uv x{uvs} {slots}")
                if n <= 5:
                    fused.upload_textures(tex[:1])
                    assert not np.array_equal(fused.render(pc, W, H), img), slots


@REFILL
def test_fused_maps_edge_cases(fused, tmp_path, refill):
    """One-texel maps under both samplers; slots beyond the table (nothing bound: the ordinary fused kernel); an emissive
    material with holes (it leaves the emitter list) and one without its alpha map."""
    fused.set_tuning("pixel_refill", refill)
    tex = _map_set()
    W, H = 112, 84
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=3, environmentOn=True)
    tiny = [tex[0], _grey(1, 1, 200), _grey(1, 1, 90), _grey(1, 3, np.array([[10], [120], [250]]))]
    _fused_same(fused, _bound(tmp_path / "t0", 0, 2.5, **FULL), tiny, pc, W, H, "one-texel maps, repeat")
    _fused_same(fused, _bound(tmp_path / "t1", 1, 2.5, **FULL), tiny, pc, W, H, "one-texel maps, clamp")
    s = _bound(tmp_path / "x", 1, 2.5, alphaIndex=7, metalnessIndex=5, bumpIndex=63)
    _same_as_oracle(fused, s, tex, pc, W, H, "slots beyond the table", maps=False)
    assert fused.last_pipeline() == 1 and fused.last_kernel().startswith("k_render_fused<"), fused.last_kernel()
    for slots in (dict(FULL, emissionStrength=1.5), dict(metalnessIndex=2, bumpIndex=3, emissionStrength=1.5)):
        s = _bound(tmp_path / f"e{len(slots)}", 0, 1.0, **slots)
        s.materials[_plane_material(s)].emissionColor[:] = [1.0, 0.8, 0.6]
        _fused_same(fused, s, tex, pc, W, H, f"emissive {slots}")


@REFILL
def test_fused_maps_heat_maps(fused, tmp_path, refill):
    fused.set_tuning("pixel_refill", refill)
    tex = _map_set()
    W, H = 112, 84
    for dbg in (0, 1, 2):
        pcd = engine.push_constants(W, H, singleRender=1, sampleLimit=2, environmentOn=True, debug=dbg, boxCap=300, triangleCap=40)
        _fused_same(fused, _bound(tmp_path / f"d{dbg}", 1, 2.5, **FULL), tex, pcd, W, H, f"heat map {dbg}", "k_render_fused_maps<true>")


def _deep_scene():
    """A lopsided mesh of BVH depth > 24 with uvs and all three maps, beside two placed copies of a small mesh under general
    transforms (test_textures.test_alpha_map_on_a_deep_bvh_with_placed_objects): the overflow buffer and object culling."""
    from instantiation_scenes import skewed, soup
    rng = np.random.default_rng(9)
    s = engine.Scene()
    glow = s.add_material(engine.default_material(albedo=(0, 0, 0), emissionColor=(1, 0.9, 0.8), emissionStrength=3.0))
    mapped = engine.default_material(albedo=(0.8, 0.7, 0.6))
    mapped.albedoIndex, mapped.alphaIndex, mapped.metalnessIndex, mapped.bumpIndex = 0, 1, 2, 3
    mapped = s.add_material(mapped)
    holes = engine.default_material(albedo=(0.3, 0.7, 0.4))
    holes.alphaIndex = 1
    holes = s.add_material(holes)
    tri, nrm = skewed(100000, 4, 5)
    s.add_mesh("deep", tri, nrm, engine.placement(), mapped, uvs=rng.uniform(-1.5, 2.5, (tri.shape[0], 6)).astype(np.float32))
    assert s.last_bvh_stats()["maxDepth"] > 24
    quad = np.array([[[-0.3, -1.5, -0.3], [0.3, -1.5, -0.3], [0.3, -1.5, 0.3]], [[-0.3, -1.5, -0.3], [0.3, -1.5, 0.3], [-0.3, -1.5, 0.3]]], np.float32)
    s.add_mesh("light", quad, np.tile(np.array([0, 1, 0], np.float32), (2, 3, 1)), engine.placement(), glow)
    t2, n2 = soup(60, 77, 0.15)
    uv2 = rng.uniform(0, 1, (60, 6)).astype(np.float32)
    s.add_mesh("placed_a", t2, n2, engine.placement(position=(0.5, 0.1, 0.2), rotation=(20, 35, 10), scale=(0.4, 0.5, 0.4), samplerIndex=1), holes, uvs=uv2)
    s.add_mesh("placed_b", t2, n2, engine.placement(position=(-0.5, 0.0, -0.1), rotation=(-15, 70, 5), scale=(0.5, 0.4, 0.6)), mapped, uvs=uv2)
    return s


def _render_same(renderer, s, tex, pc, W, H, what, threads=None):
    renderer.upload_scene(s)
    renderer.upload_textures(tex)
    pyoracle.set_textures(tex)
    renderer.reset_counters()
    img = renderer.render(pc, W, H)
    cnt = renderer.counters()
    ref, rc = pyoracle.render(s, pc, W, H, threads=threads)
    assert renderer.last_pipeline() == 1 and renderer.last_kernel() == "k_render_fused_maps<false>", (what, renderer.last_kernel())
    LAUNCHED.add(renderer.last_kernel())
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{what}: pixels differ from the oracle's"
    assert {k: cnt[k] for k in KEYS} == {k: rc[k] for k in KEYS}, what
    assert rc["lightQueryMismatch"] == 0
    return img


@REFILL
def test_fused_maps_on_a_deep_bvh_with_placed_objects(fused, refill):
    fused.set_tuning("pixel_refill", refill)
    tex = _map_set(11)
    s = _deep_scene()
    W, H = 96, 72
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=5, environmentOn=True)
    img = _render_same(fused, s, tex, pc, W, H, "deep BVH")
    fused.upload_textures([])
    assert not np.array_equal(fused.render(pc, W, H), img)


def test_fused_maps_with_several_blocks_per_wave(fused):
    """One work-group per CU and pixels replaced at 8 free lanes on a 512 x 384 tile: every wave works through several hand-outs
    while its other lanes are in flight (the case that exposed round 3's wrong binary of k_render_fused)."""
    for k, v in (("blocks_per_cu", 1), ("pixel_refill", 8)):
        fused.set_tuning(k, v)
    W, H = 512, 384
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=4, environmentOn=True)
    _render_same(fused, _deep_scene(), _map_set(11), pc, W, H, "several blocks per wave", threads=pyoracle.effective_cpus())


@REFILL
def test_fused_maps_three_frames_in_one_dispatch(fused, tmp_path, refill):
    """render_frames: three progressive frames share the launch (k_blend_frames afterwards) == the oracle's frame sequence."""
    fused.set_tuning("pixel_refill", refill)
    tex = _map_set()
    W, H = 112, 84
    s = _bound(tmp_path / "p", 1, 2.5, **FULL)
    fused.upload_scene(s.scene); s.push(fused, "objects"); s.push(fused, "materials"); fused.upload_textures(tex)
    pyoracle.set_textures(tex)
    pcp = engine.push_constants(W, H, raysPerPixel=2, progressive=1, environmentOn=True)
    fused.clear_framebuffer()
    pcp.frameCount = 0
    img = fused.render_frames(pcp, W, H, 3)
    assert fused.last_pipeline() == 1 and fused.last_kernel() == "k_render_fused_maps<false>", fused.last_kernel()
    LAUNCHED.add(fused.last_kernel())
    prev = None
    for f in range(3):
        pcp.frameCount = f
        prev, _ = pyoracle.render(s, pcp, W, H, prev=prev)
    assert np.array_equal(img.view(np.uint32), prev.view(np.uint32)), "fused frames with maps differ from the oracle's"


def test_fused_maps_selection(renderer, tmp_path):
    """fused_maps 0 keeps map scenes on the multi-kernel pipeline even under pipeline 1; 1 with pipeline -1 lets a small map scene
    go fused; pipeline 0 still runs k_trace_pw_alpha; values other than 0 and 1 are refused."""
    tex = _map_set()
    W, H = 64, 48
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2, environmentOn=True)
    try:
        renderer.set_tuning("pipeline", 1)
        s = _bound(tmp_path / "a", 0, 2.5, **FULL)
        _same_as_oracle(renderer, s, tex, pc, W, H, "fused_maps 0, pipeline 1", "k_trace_pw_alpha<false>")   # asserts pipeline 0
        renderer.set_tuning("fused_maps", 1)
        renderer.set_tuning("pipeline", -1)
        _fused_same(renderer, _bound(tmp_path / "b", 0, 2.5, **FULL), tex, pc, W, H, "fused_maps 1, pipeline -1")
        renderer.set_tuning("pipeline", 0)
        _same_as_oracle(renderer, _bound(tmp_path / "c", 0, 2.5, **FULL), tex, pc, W, H, "fused_maps 1, pipeline 0", "k_trace_pw_alpha<false>")
        for bad in (2, -1):
            with pytest.raises(engine.RtError):
                renderer.set_tuning("fused_maps", bad)
    finally:
        pyoracle.set_textures([])
        renderer.upload_textures([])
        for k, v in DEFAULTS.items():
            renderer.set_tuning(k, v)


def test_every_maps_instantiation_was_launched():
    """Runs after the cases above (file order): every k_render_fused_maps instantiation in the library was launched by them."""
    in_library = maps_instantiations()
    assert in_library, "no k_render_fused_maps instantiation in the library's symbol table"
    assert not (LAUNCHED - in_library), f"launched kernels the symbol table does not hold: {sorted(LAUNCHED - in_library)}"
    assert in_library <= LAUNCHED, f"never launched: {sorted(in_library - LAUNCHED)}"
