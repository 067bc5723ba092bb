"""render.py --bake-object: the lightmap of one object of the scene from the command line (rt_bake_lightmap through
Renderer.bake_lightmap), and what the options refuse before a device is touched."""
import numpy as np
import pytest

from ray_tracer_amd import _capi, engine, render, scenes


def test_bake_options_are_refused_without_an_npy_file():
    for argv in (["--bake-object", "0"], ["--bake-object", "0", "--bake-out", "map.png"]):
        with pytest.raises(SystemExit, match="--bake-out FILE.npy"):
            render.main(argv)


@pytest.mark.gpu
def test_bake_object_writes_the_map_bake_lightmap_gives(renderer, tmp_path):
    """The floor of the Cornell box (object 0), 24 x 16 texels, 4 samples: the file holds what Renderer.bake_lightmap returns for
    the same scene and parameters, bit for bit, and the fill plane beside it."""
    out = tmp_path / "floor.npy"
    assert render.main(f"--scene cornell --bake-object 0 --bake-size 24 16 --rays-per-pixel 4 --bounce-limit 3 --bake-dilate 1 --bake-out {out}".split()) == 0
    got, fill = np.load(out), np.load(str(out)[:-4] + ".fill.npy")
    renderer.upload_scene(scenes.CONFIGS["cornell"]()[0])
    pc = engine.push_constants(1728, 1117, bounceLimit=3, raysPerPixel=4)
    want, wfill, st = renderer.bake_lightmap(0, 24, 16, params=_capi.RtIrradianceParams(4, 3, 0, 0, 1e-5), env=pc.environment, dilate=1)
    assert got.shape == (16, 24, 4) and got.dtype == np.float32 and fill.shape == (16, 24)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(fill, wfill)
    print(st)
