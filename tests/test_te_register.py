"""A light query's tE in a register in every k_trace_pw instantiation (trace_wave<ROOMY>, rt_kernels.hip.h).

A light query (the NEE ray or the cosine probe of a diffuse bounce) carries tE, the distance of the nearest emissive primitive on
its line. The leaf step that finds a triangle nearer than tE ends the query with "no hit"; one that finds none runs to the end
and reports the emitter. Until the device code was built without the SLP vectorizer only the kernels for five work-groups per CU
held tE in a register; the six-work-group ones re-read it from the hit record. Now all of them hold it, and this test sends both
kinds of query through every table mode ("hot_pairs" 0 / 1 / 2), both stack sizes the klein bottle's depth can be given
("lds_stack" 16: the overflow stack behind 16 entries; the default: all in LDS) and both pipelines (the fused kernel keeps
re-reading tE: the same pixels either way).

The scene is the Cornell box with its ceiling emitter, the klein bottle as a placed object (general transform: the set-up step
runs) under the emitter, and one sphere. Queries from the floor under the bottle end at one of its triangles; queries from the
open floor and the walls reach the emitter. That both are there is asserted, not assumed: a query that ends at an occluder
reports no hit, so the same frame without the bottle and the sphere — every light query of which reaches the emitter or a wall —
has another `raysHit` per traced ray, and in the occluded frame fewer rays hit than were traced."""
import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine

from util import cornell_scene, model_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
COUNTERS = ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests")


def _pc():
    return engine.push_constants(W, H, singleRender=1, sampleLimit=4, bounceLimit=8)


@pytest.fixture(scope="module")
def occluded():
    """The scene and the oracle's frame and counters, computed once."""
    s = model_scene("klein_bottle.obj", material=4, scale=0.5, position=(0.0, -0.2, 0.0))
    s.set_sphere(0, (0.55, 0.2, -0.5), 0.25, 5)
    ref, rc = pyoracle.render(s, _pc(), W, H)
    return s, ref, rc


def test_both_kinds_of_light_query_are_in_the_image(occluded):
    _, ref, rc = occluded
    _, open_rc = pyoracle.render(cornell_scene(False), _pc(), W, H)
    assert rc["lightQueryMismatch"] == 0 and open_rc["lightQueryMismatch"] == 0 and rc["stackOverflow"] == 0
    # queries that ended at an occluder report no hit ...
    assert rc["raysHit"] < rc["raysTraced"]
    # ... and the frame without occluders has none of them: another number of hits, and more of them per traced ray
    assert rc["raysHit"] != open_rc["raysHit"]
    assert rc["raysHit"] * open_rc["raysTraced"] < open_rc["raysHit"] * rc["raysTraced"]
    # queries that reached the emitter: direct light arrived somewhere
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0


@pytest.mark.parametrize("pipeline", [0, 1], ids=["multikernel", "fused"])
def test_te_in_a_register_every_table_mode_and_stack(renderer, occluded, pipeline):
    s, ref, rc = occluded
    renderer.upload_scene(s)
    try:
        renderer.set_tuning("pipeline", pipeline)
        for cap in (16, 24):
            for hot in (0, 1, 2):
                renderer.set_tuning("lds_stack", cap)
                renderer.set_tuning("hot_pairs", hot)
                renderer.reset_counters()
                img = renderer.render(_pc(), W, H)
                cnt = renderer.counters()
                what = f"pipeline {pipeline}, lds_stack {cap}, hot_pairs {hot}"
                assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{what}: pixels not bit-identical"
                for k in COUNTERS:
                    assert cnt[k] == rc[k], f"{what}: counter {k}: gpu {cnt[k]} oracle {rc[k]}"
    finally:
        renderer.set_tuning("hot_pairs", 2)
        renderer.set_tuning("lds_stack", 24)
        renderer.set_tuning("pipeline", -1)


# ---------------------------------------------------------------- the leaf step: both triangles of a step fetched ahead of both tests
#
# In the traversal kernels without overflow stack, per-pixel counters and object culling the second triangle's loads are pinned in
# front of the first triangle's test (RT_LEAF_PRELOAD); a leaf of one triangle fetches that triangle twice (j1 == j) and tests it
# once, a leaf of up to seven goes two by two, and a bigger leaf takes the loop beside it. The builder's leaves hold one or two
# triangles (the cube: 12 triangles; the bunny: some thousand leaves of either kind); nine coplanar triangles with one common
# centroid, which no split plane separates, stay one leaf.

def _fan9_obj(path):
    """Nine triangles in the plane z = 0, each (-s, -s) (s, -s) (0, 2 s) with s = k / 16: every centroid is the origin, exactly."""
    with open(path, "w") as f:
        for k in range(1, 10):
            s = k / 16.0
            f.write(f"v {-s} {-s} 0\nv {s} {-s} 0\nv 0 {2 * s} 0\n")
        f.write("vt 0 0\nvn 0 0 1\n")
        for k in range(9):
            f.write(f"f {3 * k + 1}/1/1 {3 * k + 2}/1/1 {3 * k + 3}/1/1\n")
    return str(path)


@pytest.fixture(scope="module")
def leaf_scenes(tmp_path_factory):
    """{name: (scene, oracle frame, oracle counters)}, computed once."""
    objs = {"cube": "cube.obj", "bunny": "bunny.obj", "fan9": _fan9_obj(tmp_path_factory.mktemp("leaf") / "fan9.obj")}
    out = {}
    for name, obj in objs.items():
        s = model_scene(obj, material=0, scale=0.5, position=(0.0, 0.1, -0.2))
        out[name] = (s,) + tuple(pyoracle.render(s, _leaf_pc(), W, H))
    return out


def _leaf_pc():
    return engine.push_constants(W, H, singleRender=1, sampleLimit=2)


def test_leaf_scenes_have_the_leaves_they_are_there_for(leaf_scenes):
    assert leaf_scenes["cube"][0].last_bvh_stats()["maxTri"] == 2
    assert leaf_scenes["bunny"][0].last_bvh_stats()["maxTri"] == 2
    assert leaf_scenes["fan9"][0].last_bvh_stats()["maxTri"] == 9
    for name, (_, ref, rc) in leaf_scenes.items():
        assert rc["triTests"] > 0 and rc["stackOverflow"] == 0 and np.isfinite(ref).all(), name


@pytest.mark.parametrize("name", ["cube", "bunny", "fan9"])
def test_leaf_step_with_both_triangles_fetched_ahead(renderer, leaf_scenes, name):
    s, ref, rc = leaf_scenes[name]
    renderer.upload_scene(s)
    try:
        for pipeline, hot in ((0, 0), (0, 1), (0, 2), (1, 2)):
            renderer.set_tuning("pipeline", pipeline)
            renderer.set_tuning("hot_pairs", hot)
            renderer.reset_counters()
            img = renderer.render(_leaf_pc(), W, H)
            cnt = renderer.counters()
            what = f"{name}, pipeline {pipeline}, hot_pairs {hot}"
            assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{what}: pixels not bit-identical"
            for k in COUNTERS:
                assert cnt[k] == rc[k], f"{what}: counter {k}: gpu {cnt[k]} oracle {rc[k]}"
    finally:
        renderer.set_tuning("hot_pairs", 2)
        renderer.set_tuning("pipeline", -1)
