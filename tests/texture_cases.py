"""Texture and material-map fixtures shared by the texture tests: small images, the map set of a material, and the comparison with the oracle."""
import os
import shutil

import numpy as np

from oracle import pyoracle
from ray_tracer_amd import engine

from util import EditedScene, cornell_scene


def _checker(w, h, a=(230, 40, 40, 255), b=(30, 60, 220, 255), cell=4):
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.where((((xx // cell) + (yy // cell)) % 2 == 0)[..., None], np.array(a, np.uint8), np.array(b, np.uint8)).astype(np.uint8)
    img[0, :, :] = (255, 255, 255, 255)     # first row and column marked: clamping and wrapping differ there
    img[:, 0, :] = (10, 200, 10, 255)
    return img


def _plane_scene(tmp_path, sampler, uv_scale=1.0):
    """test_plane.obj + test_plane.mtl (map_Bump is skipped: case-sensitive; map_Kd claims slot 0) in a temporary directory
    next to a generated vase_dif.png; the plane replaces the Cornell box's floor region."""
    d = tmp_path / f"plane_{sampler}_{uv_scale}"
    d.mkdir(parents=True)
    for f in ("test_plane.obj", "test_plane.mtl"):
        shutil.copy(os.path.join(engine.ASSET_DIR, f), d / f)
    if uv_scale != 1.0:   # uvs beyond [0, 1]: the two samplers must disagree
        lines = []
        for ln in open(d / "test_plane.obj"):
            if ln.startswith("vt "):
                u, v = (float(x) for x in ln.split()[1:3])
                ln = f"vt {u * uv_scale - 0.75:.6f} {v * uv_scale - 0.75:.6f}\n"
            lines.append(ln)
        open(d / "test_plane.obj", "w").writelines(lines)
    from PIL import Image
    Image.fromarray(_checker(24, 16)).save(d / "vase_dif.png")
    s = cornell_scene(False)
    s.read_obj(str(d / "test_plane.obj"), engine.placement(position=(0.0, 0.3, 0.2), scale=0.6, samplerIndex=sampler), 0)
    assert s.texture_paths() == [str(d / "vase_dif.png")]
    # read_obj leaves the samplerIndex of a file's last (here: only) group at 0 whatever the placement says
    # (src/vk_engine.cpp:1009-1019 never copies it); the object editor's field is what selects the clamp sampler
    ed = EditedScene(s)
    assert ed.objects[ed.nObjects - 1].samplerIndex == 0
    ed.objects[ed.nObjects - 1].samplerIndex = sampler
    ed.texture_paths = s.texture_paths
    ed.find_material, ed.material, ed.set_material = s.find_material, s.material, s.set_material
    return ed


def _plane_material(s):
    return s.find_material(s.texture_paths()[0].replace("vase_dif.png", "test_plane.mtl") + "/Material.001")


def _grey(w, h, value):
    """A map whose red channel is `value` (a number, or an [h, w] array) — the channel the three maps read."""
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = value
    img[..., 1] = 7; img[..., 2] = 201; img[..., 3] = 255   # the other channels must not matter
    return img


def _bound(tmp_path, sampler=0, uv_scale=1.0, **slots):
    """The plane scene with map slots bound on the plane's material: _bound(tmp, alphaIndex=1, reflectance=1.0, ...)."""
    s = _plane_scene(tmp_path, sampler, uv_scale)
    mi = _plane_material(s)
    for k, v in slots.items():
        setattr(s.materials[mi], k, v)
    return s


def _map_set(seed=5):
    """Generated maps: slot 0 the albedo checker, 1 alpha (holes), 2 metalness (stripes and a few faint texels), 3 bump (noise)."""
    rng = np.random.default_rng(seed)
    holes = np.where(rng.uniform(size=(12, 20)) < 0.35, rng.integers(0, 188, (12, 20)), rng.integers(188, 256, (12, 20)))
    stripes = np.where(np.arange(10)[None, :] % 3 == 0, rng.integers(1, 256, (7, 10)), 0)
    return [_checker(24, 16), _grey(20, 12, holes), _grey(10, 7, stripes), _grey(16, 16, rng.integers(0, 256, (16, 16)))]


KEYS = ("boxTests", "triTests", "raysTraced", "raysHit", "raysReference", "paths", "segments", "emitterTests")


def _same_as_oracle(renderer, s, tex, pc, W, H, what, kernel=None, maps=True):
    renderer.upload_scene(s.scene)
    s.push(renderer, "objects")
    s.push(renderer, "materials")
    renderer.upload_textures(tex)
    renderer.reset_counters()
    img = renderer.render(pc, W, H)
    cnt = renderer.counters()
    pyoracle.set_textures(tex)
    ref, rc = pyoracle.render(s, pc, W, H)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"{what}: pixels differ from the oracle's ({renderer.last_kernel()})"
    assert {k: cnt[k] for k in KEYS} == {k: rc[k] for k in KEYS}, what
    assert rc["lightQueryMismatch"] == 0
    assert not maps or renderer.last_pipeline() == 0, "scenes that bind these maps belong to the multi-kernel pipeline"
    if kernel:
        assert renderer.last_kernel() == kernel, (what, renderer.last_kernel())
    return img
