"""First-hit AOVs (rt_render_aovs, Renderer.render_aovs / pick, InteractiveSession.pick, render.py --aov-out).

One pass shoots every pixel's camera ray — the ray each sample of that pixel starts with in rt_render (no jitter,
raytrace.comp:547-556) — through the ordinary traversal and writes the closest hit as per-pixel planes. The planes must be the
oracle's calculateIntersections record for the same ray bit for bit, the counters its per-ray tests, and a pass must leave
every later rt_render exactly as it would have been. CPU: the ctypes layout, the plane decoding and the CLI flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import _capi, engine, render, scenes
from ray_tracer_amd.session import InteractiveSession

from aov_cases import _albedos, _as_hits, _check_misses, _upload, PLANES
from instantiation_scenes import build_scene, skewed, soup
from util import EditedScene, assert_hits_equal, cornell_scene, device_buffers, frames_between_passes, model_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = 2.0 ** -23   # one float32 ulp of a unit component


# ---------------------------------------------------------------- CPU
def test_aov_buffers_layout_matches_the_header():
    fields = [n for n, _ in _capi.RtAovBuffers._fields_]
    assert fields == list(engine.AOV_PLANES) == ["normalDepth", "position", "albedo", "rayDir", "ids"]
    assert C.sizeof(_capi.RtAovBuffers) == 5 * C.sizeof(C.c_void_p)
    src = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    body = re.search(r"typedef struct RtAovBuffers \{(.*?)\} RtAovBuffers;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == fields
    assert "rt_render_aovs" in _capi.SYMBOLS and "rt_read_aovs" in _capi.SYMBOLS


def test_planes_decode():
    n, w = 2, 3
    rng = np.random.default_rng(5)
    planes = {k: rng.random((n, w, 4)).astype(np.float32) for k in ("normalDepth", "position", "albedo", "rayDir")}
    ids = rng.integers(0, 1 << 20, (n, w, 4)).astype(np.uint32)
    ids[..., 3] = np.arange(n * w).reshape(n, w) % 8
    planes["ids"] = ids
    a = engine.aovs_to_numpy(planes)
    assert set(a) == set(PLANES)
    assert a["depth"].shape == (n, w) and a["normal"].shape == (n, w, 3) and a["object"].dtype == np.uint32
    assert np.array_equal(a["depth"], planes["normalDepth"][..., 3]) and np.array_equal(a["ray_dir"], planes["rayDir"][..., :3])
    assert np.array_equal(a["triangle"], ids[..., 1]) and np.array_equal(a["material"], ids[..., 2])
    assert np.array_equal(a["hit"], ids[..., 3] & 1 == 1) and np.array_equal(a["sphere"], ids[..., 3] & 2 == 2)
    assert np.array_equal(a["front_face"], ids[..., 3] & 4 == 4)


def test_aov_out_flag():
    assert render.build_parser().parse_args([]).aov_out is None
    assert render.build_parser().parse_args(["--aov-out", "planes.npz"]).aov_out == "planes.npz"


def _raw_pass(renderer, pc, W, H, row0=0, rowStride=1, nRows=None, objectCount=None):
    """rt_render_aovs with the scene's counts (objectCount overrides) into the ctx-owned planes."""
    nRows = (H - row0 + rowStride - 1) // rowStride if nRows is None else nRows
    pc.rayTraceParams.sphereCount = renderer._counts["spheres"]
    pc.rayTraceParams.objectCount = renderer._counts["objects"] if objectCount is None else objectCount
    renderer._check(renderer._l.rt_render_aovs(renderer._h, C.byref(pc), W, H, row0, rowStride, nRows, None), "rt_render_aovs")
    renderer._aov_shape = (nRows, W)
    return renderer.read_aovs()


def _same_as_oracle(renderer, s, pc, W, H, what, objectCount=None, **tile):
    """One pass against oracle_trace_rays on the pass's own rays (camInfo.pos, the rayDir plane): fields and counters."""
    renderer.reset_counters()
    if objectCount is None:
        a = renderer.render_aovs(pc, W, H, **tile)
        objectCount = renderer._counts["objects"]
    else:   # fewer objects than uploaded (Renderer.render_aovs fills in the scene's counts)
        a = _raw_pass(renderer, pc, W, H, objectCount=objectCount, **tile)
    c = renderer.counters()
    d = np.ascontiguousarray(a["ray_dir"].reshape(-1, 3))
    o = np.tile(np.array(list(pc.camInfo.pos), np.float32), (d.shape[0], 1))
    arr = s.arrays()
    hits = (_capi.RtHit * d.shape[0])()
    fp = C.POINTER(C.c_float)
    assert pyoracle.lib().oracle_trace_rays(C.byref(arr), arr.sphereCount, objectCount, d.shape[0], o.ctypes.data_as(fp),
                                            d.ctypes.data_as(fp), hits) == 0
    ref = engine.hits_to_numpy(hits)
    got = _as_hits(a)
    assert_hits_equal(got, {k: ref[k] for k in got})
    _check_misses(a)
    assert c["boxTests"] == int(ref["boxTests"].sum()), what
    assert c["triTests"] == int(ref["triTests"].sum()), what
    assert c["raysTraced"] == d.shape[0] and c["raysHit"] == int(ref["didHit"].sum()), what
    assert (c["raysReference"], c["paths"], c["segments"], c["emitterTests"], c["traceLaunches"]) == (0, 0, 0, 0, 1), what
    return a


def _placed_scene(n, seed=7):
    """The Cornell box and n small meshes under rotations and non-uniform scales (from 48 on: the object hierarchy)."""
    rng = np.random.default_rng(seed)
    s = cornell_scene(False)
    for k in range(n):
        t, nr = soup(12, 100 + k, 0.08)
        pl = engine.placement(position=tuple(rng.uniform(-0.6, 0.6, 3) + (0, -0.4, 0)), rotation=tuple(rng.uniform(-60, 60, 3)),
                              scale=tuple(rng.uniform(0.3, 0.9, 3)))
        s.add_mesh(f"p{k}", t, nr, pl, int(rng.integers(0, 6)))
    return s


def _inside_scene():
    s = cornell_scene(False)
    pos, nrm = scenes.blob(3000, seed=3, radius=0.45, center=(0.0, -0.5, 0.0))
    s.add_mesh("blob", pos.astype(np.float32), nrm.astype(np.float32), engine.placement(), 2)
    return s


# ---------------------------------------------------------------- 1. parity with the oracle
PARITY = {
    "cornell_spheres": lambda: cornell_scene(True),
    "bunny": lambda: model_scene("bunny.obj"),
    "klein": lambda: model_scene("klein_bottle.obj", scale=0.5, position=(0, -0.2, 0)),
    "placed_nonuniform": lambda: build_scene(lambda: soup(1200, 2, 0.04), True)[0],
    "placed_56": lambda: _placed_scene(56),
    "deep_bvh": lambda: build_scene(lambda: skewed(100000, 4, 5), False),   # (scene, BVH depth)
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_with_the_oracle(renderer, name):
    s = PARITY[name]()
    if name == "deep_bvh":
        s, depth = s
        assert depth > 24
    W, H = 72, 52
    renderer.upload_scene(s)
    a = _same_as_oracle(renderer, s, engine.push_constants(W, H, fov=70.0), W, H, name)
    assert a["hit"].sum() > 200
    if name == "cornell_spheres":
        assert a["sphere"].any() and (a["hit"] & ~a["sphere"]).any()


@pytest.mark.gpu
def test_parity_camera_inside_a_mesh(renderer):
    s = _inside_scene()
    W, H = 64, 48
    renderer.upload_scene(s)
    a = _same_as_oracle(renderer, s, engine.push_constants(W, H, pos=(0.0, -0.5, 0.0), fov=90.0), W, H, "inside")
    assert (a["hit"] & ~a["front_face"]).mean() > 0.5   # the blob seen from inside: its back faces


@pytest.mark.gpu
def test_parity_with_fewer_objects_than_uploaded(renderer):
    s = _placed_scene(56)
    W, H = 64, 48
    renderer.upload_scene(s)
    n = renderer._counts["objects"]
    pc = engine.push_constants(W, H, fov=70.0)
    full = _raw_pass(renderer, pc, W, H)
    for k in (n - 1, n - 30, 3):
        a = _same_as_oracle(renderer, s, pc, W, H, f"objectCount {k} of {n}", objectCount=k)
        assert a["object"][a["hit"] & ~a["sphere"]].max() < k
    assert not np.array_equal(a["object"], full["object"])
    back = renderer.render_aovs(pc, W, H)   # the uploaded counts come back
    for key in PLANES:
        assert np.array_equal(back[key].view(np.uint8), full[key].view(np.uint8)), key


@pytest.mark.gpu
def test_parity_sponza_rows_at_1080p(renderer):
    s = scenes.sponza(0)[0]
    W, H = 1920, 1080
    renderer.upload_scene(s)
    a = _same_as_oracle(renderer, s, scenes.sponza_camera(W, H), W, H, "sponza", row0=7, rowStride=211, nRows=6)
    assert a["hit"].mean() > 0.5
    assert renderer.last_kernel().startswith("k_trace_pw<")


@pytest.mark.gpu
def test_parity_alpha_and_bump_maps(renderer, tmp_path):
    from texture_cases import _bound, _map_set
    tex = _map_set()
    W, H = 72, 54
    pc = engine.push_constants(W, H)
    n = 0
    try:
        pyoracle.set_textures(tex)
        for sampler in (0, 1):
            for slots in (dict(alphaIndex=1), dict(bumpIndex=3), dict(alphaIndex=1, bumpIndex=3, metalnessIndex=2)):
                n += 1
                s = _bound(tmp_path / f"s{n}", sampler, 2.5, **slots)
                _upload(renderer, s)
                renderer.upload_textures(tex)
                a = _same_as_oracle(renderer, s, pc, W, H, f"sampler {sampler} {slots}")
                if "alphaIndex" in slots:
                    assert renderer.last_kernel() == "k_trace_pw_alpha<false>"
                renderer.upload_textures(tex[:1])   # the map slots beyond the table: nothing bound, other records
                b = renderer.render_aovs(pc, W, H)
                assert not (np.array_equal(a["normal"], b["normal"]) and np.array_equal(a["hit"], b["hit"])), slots
    finally:
        pyoracle.set_textures([])
        renderer.upload_textures([])


# ---------------------------------------------------------------- 2. camera rays against a float64 restatement
from brute_force import camera_dirs as _camera_dirs   # noqa: E402  (the float64 camera lives with the float64 closest-hit reference)


@pytest.mark.gpu
def test_camera_rays_against_a_float64_restatement(renderer):
    """Bound: 16 float32 ulps of a unit component (rt_tan, rt_normalize and the float32 plane arithmetic against float64)."""
    renderer.upload_scene(cornell_scene(True))
    cases = [(64, 48, {}), (61, 45, dict(fov=90.0, cameraAngles=(10.0, 30.0, 5.0))),
             (40, 72, dict(fov=20.0, nearPlane=0.7, cameraAngles=(-25.0, 200.0, 0.0))),
             (33, 17, dict(fov=120.0, aspectRatio=3.0, cameraAngles=(0.0, -90.0, 45.0)))]
    for W, H, kw in cases:
        pc = engine.push_constants(W, H, **kw)
        err = np.abs(renderer.render_aovs(pc, W, H)["ray_dir"].astype(np.float64) - _camera_dirs(pc, W, H)).max()
        assert err <= 16 * ULP1, (W, H, kw, err)
    # the vec4(dir, 1) of the reference: a translation column moves every direction
    pc = engine.push_constants(24, 16)
    pc.camInfo.cameraRotation[12], pc.camInfo.cameraRotation[13], pc.camInfo.cameraRotation[14] = 0.25, -0.5, 0.125
    err = np.abs(renderer.render_aovs(pc, 24, 16)["ray_dir"].astype(np.float64) - _camera_dirs(pc, 24, 16)).max()
    assert err <= 16 * ULP1, err


@pytest.mark.gpu
def test_albedo_of_untextured_materials(renderer):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    W, H = 64, 48
    a = renderer.render_aovs(engine.push_constants(W, H), W, H)
    h = a["hit"]
    assert a["sphere"].any() and h.sum() > 1000
    assert np.array_equal(a["albedo"][h].view(np.uint32), _albedos(s)[a["material"][h]].view(np.uint32))


def _quad_scene(sampler, uv_lo, uv_hi, sphere=False):
    """A quad facing the default camera (x in [-0.6, 0.6], y in [-1.1, 0.1], z = 0), uv linear in x and y from uv_lo to uv_hi,
    its material binding texture slot 0; `sphere`: a sphere of the same material in front of it."""
    s = engine.Scene()
    m = s.add_material(engine.default_material(albedo=(0.75, 0.5, 0.25), albedoIndex=0))
    x0, x1, y0, y1 = -0.6, 0.6, -1.1, 0.1
    P = np.array([[[x0, y0, 0], [x1, y0, 0], [x1, y1, 0]], [[x0, y0, 0], [x1, y1, 0], [x0, y1, 0]]], np.float32)
    UV = uv_lo + (uv_hi - uv_lo) * np.stack([(P[..., 0] - x0) / (x1 - x0), (P[..., 1] - y0) / (y1 - y0)], -1)
    s.add_mesh("quad", P, np.tile(np.array([0, 0, -1], np.float32), (2, 3, 1)), engine.placement(), m, uvs=UV.astype(np.float32))
    if sphere:
        s.set_sphere(0, (0.3, -0.2, -0.5), 0.15, m)
    ed = EditedScene(s)   # the mesh's sampler is the object editor's field, as for read_obj's last group (tests/test_textures.py)
    ed.objects[0].samplerIndex = sampler
    return ed, m, (x0, x1, y0, y1)


def _decode_exact(byte):
    """rt_srgb8_to_linear where its arithmetic is fixed: byte / 255, and / 12.92 on the linear segment (bytes <= 10)."""
    c = np.float32(byte) / np.float32(255)
    return c / np.float32(12.92) if byte <= 10 else c


@pytest.mark.gpu
def test_albedo_of_a_constant_texture(renderer):
    """albedo x decode(c): bit for bit for bytes 0, 255 and the linear segment; elsewhere rt_pow against the float64 curve
    within 16 float32 ulps (relative). Spheres of the textured material keep the plain albedo."""
    s, m, _ = _quad_scene(0, 0.0, 1.0, sphere=True)
    _upload(renderer, s)
    W, H = 48, 40
    pc = engine.push_constants(W, H)
    mat = _albedos(s)[m]
    try:
        for rgb in ((0, 255, 7), (10, 3, 255), (128, 200, 60), (11, 90, 254)):
            img = np.zeros((3, 5, 4), np.uint8)
            img[...] = (*rgb, 255)
            renderer.upload_textures([img])
            a = renderer.render_aovs(pc, W, H)
            tri = a["hit"] & ~a["sphere"]
            assert tri.sum() > 100 and a["sphere"].sum() > 10
            got = a["albedo"][tri]
            assert np.all(got == got[0])
            for ch, byte in enumerate(rgb):
                if byte in (0, 255) or byte <= 10:
                    assert got[0, ch].view(np.uint32) == (mat[ch] * _decode_exact(byte)).view(np.uint32), (rgb, ch)
                else:
                    c = byte / 255.0
                    want = float(mat[ch]) * ((c + 0.055) / 1.055) ** 2.4
                    assert abs(float(got[0, ch]) - want) <= 16 * ULP1 * want, (rgb, ch, float(got[0, ch]), want)
            assert np.array_equal(a["albedo"][a["sphere"]], np.tile(mat, (int(a["sphere"].sum()), 1)))
    finally:
        renderer.upload_textures([])


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", [0, 1])
def test_albedo_of_a_two_by_two_map(renderer, sampler):
    """Each quadrant of uv space gets its texel at (u, 1 - v); uvs run from -0.5 to 1.5, where repeat (0) and clamp to edge (1)
    part ways. Pixels whose uv lies within 0.02 texels of a texel edge are left out (the interpolated uv may round across)."""
    lo, hi = -0.5, 1.5
    s, m, (x0, x1, y0, y1) = _quad_scene(sampler, lo, hi)
    _upload(renderer, s)
    W, H = 96, 80
    texels = np.array([[(255, 0, 0, 255), (0, 255, 0, 255)], [(0, 0, 255, 255), (255, 255, 255, 255)]], np.uint8)   # rows top to bottom
    mat = _albedos(s)[m]
    try:
        renderer.upload_textures([texels])
        a = renderer.render_aovs(engine.push_constants(W, H), W, H)
    finally:
        renderer.upload_textures([])
    h = a["hit"]
    p = a["position"][h].astype(np.float64)
    fu = 2 * (lo + (hi - lo) * (p[:, 0] - x0) / (x1 - x0))            # texel coordinates, 2 texels per unit of uv
    fv = 2 * (1.0 - (lo + (hi - lo) * (p[:, 1] - y0) / (y1 - y0)))
    keep = (np.abs(fu - np.round(fu)) > 0.02) & (np.abs(fv - np.round(fv)) > 0.02)
    assert keep.sum() > 300
    if sampler == 1:
        ix, iy = np.clip(np.floor(fu), 0, 1), np.clip(np.floor(fv), 0, 1)
    else:
        ix, iy = np.floor(fu) % 2, np.floor(fv) % 2
    want = texels[iy.astype(int), ix.astype(int), :3].astype(np.float32) / np.float32(255)   # bytes 0 and 255: 0 and 1 exactly
    assert np.array_equal(a["albedo"][h][keep], mat * want[keep])
    assert len(np.unique(want[keep], axis=0)) == 4


# ---------------------------------------------------------------- 4. tiling
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 48), (61, 45), (13, 7)])
def test_strips_and_rows_equal_the_full_frame(renderer, W, H):
    renderer.upload_scene(model_scene("bunny.obj", spheres=True))
    pc = engine.push_constants(W, H)
    full = renderer.render_aovs(pc, W, H)

    def same(part, rows, what):
        for k in PLANES:
            assert np.array_equal(part[k].view(np.uint8), full[k][rows].view(np.uint8)), (what, k)

    for row0 in range(3):
        same(renderer.render_aovs(pc, W, H, row0=row0, rowStride=3), slice(row0, None, 3), f"stride 3 row0 {row0}")
    for y in (0, H // 2, H - 1):
        same(renderer.render_aovs(pc, W, H, row0=y, nRows=1), slice(y, y + 1), f"row {y}")


@pytest.mark.gpu
def test_device_planes(renderer):
    import torch  # noqa: F401  (its wheel's copy of the HIP runtime now sits beside the library's: devmem.hip must not take it)
    renderer.upload_scene(cornell_scene(True))
    W, H = 40, 30
    pc = engine.push_constants(W, H)
    ref = renderer.render_aovs(pc, W, H)
    nbytes = H * W * 16
    with device_buffers(list(engine.AOV_PLANES) + ["only"], nbytes, fill=7) as bufs:
        assert renderer.render_aovs(pc, W, H, out_ptrs={k: bufs[k].ptr for k in engine.AOV_PLANES}) is None
        got = engine.aovs_to_numpy({k: bufs[k].download((H, W, 4), np.uint32 if k == "ids" else np.float32) for k in engine.AOV_PLANES})
        for k in PLANES:
            assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k
        renderer.render_aovs(pc, W, H, out_ptrs={"ids": bufs["only"].ptr, "position": 0})   # one plane only
        assert np.array_equal(bufs["only"].download((H, W, 4), np.uint32)[..., 0], ref["object"])


# ---------------------------------------------------------------- 5. no side effects on rendering
@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [-1, 0])
def test_passes_leave_rendering_untouched(renderer, pipeline):
    s = model_scene("bunny.obj", spheres=True)
    W, H = 64, 48
    renderer.set_tuning("pipeline", pipeline)

    def aov_passes(other, w, h):
        renderer.render_aovs(other, w, h)
        renderer.render_aovs(other, w, h, row0=1, rowStride=2, sync=False)

    try:
        a = frames_between_passes(renderer, s, W, H)
        b = frames_between_passes(renderer, s, W, H, aov_passes)
    finally:
        renderer.set_tuning("pipeline", -1)
    for fa, fb in zip(a[0], b[0]):
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert a[1] == b[1]
    assert a[2] == b[2]


@pytest.mark.gpu
def test_pass_after_a_heat_map_render(renderer):
    renderer.upload_scene(model_scene("bunny.obj"))
    W, H = 48, 40
    pc = engine.push_constants(W, H)
    before = renderer.render_aovs(pc, W, H)
    kernel = renderer.last_kernel()
    args = kernel[kernel.index("<") + 1:-1].split(", ")
    assert kernel.startswith("k_trace_pw<") and args[2:4] == ["false", "false"], kernel   # no PIX, no STATS
    renderer.render(engine.push_constants(W, H, debug=0), W, H)
    after = renderer.render_aovs(pc, W, H)
    assert renderer.last_kernel() == kernel
    for k in PLANES:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k


# ---------------------------------------------------------------- 6. picking
@pytest.mark.gpu
def test_pick_equals_the_full_pass(renderer):
    W, H = 80, 60
    sess = InteractiveSession(renderer, cornell_scene(True), W, H)
    sess._rotation()
    full = renderer.render_aovs(sess.pc, W, H)
    picks = {"sphere": np.argwhere(full["sphere"]), "mesh": np.argwhere(full["hit"] & ~full["sphere"]), "miss": np.argwhere(~full["hit"])}
    for what, px in picks.items():
        assert len(px), what
        y, x = (int(v) for v in px[len(px) // 2])
        for rec in (renderer.pick(sess.pc, W, H, x, y), sess.pick(x, y)):
            assert set(rec) == set(PLANES)
            for k in PLANES:
                assert np.array_equal(np.asarray(rec[k]), full[k][y, x]), (what, k)
            assert rec["hit"] == (what != "miss") and rec["sphere"] == (what == "sphere")
    with pytest.raises(ValueError):
        renderer.pick(sess.pc, W, H, W, 0)


# ---------------------------------------------------------------- 7. CLI
@pytest.mark.gpu
def test_cli_aov_out_on_one_and_two_ranks(tmp_path):
    import subprocess
    import sys
    job = "--scene cornell --width 56 --height 37 --single-render --sample-limit 1"
    one, two = tmp_path / "one.npz", tmp_path / "two.npz"
    assert render.main(f"{job} --aov-out {one}".split()) == 0
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29551", "-m", "ray_tracer_amd.render", *job.split(), "--backend", "gloo", "--aov-out", str(two)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    a, b = np.load(one), np.load(two)
    assert sorted(a.files) == sorted(b.files) == sorted(PLANES)
    assert a["depth"].shape == (37, 56) and a["hit"].dtype == np.bool_ and a["object"].dtype == np.uint32 and a["hit"].any()
    for k in PLANES:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---------------------------------------------------------------- 8. errors
@pytest.mark.gpu
def test_errors(built):
    r = engine.Renderer(0)
    try:
        pc = engine.push_constants(8, 8)
        r._counts = {"spheres": 0, "objects": 0}
        with pytest.raises(engine.RtError, match="rt_render_aovs before rt_upload_scene"):
            r.render_aovs(pc, 8, 8)
        with pytest.raises(engine.RtError, match="no ctx-owned AOV planes"):
            r._check(r._l.rt_read_aovs(r._h, C.byref(_capi.RtAovBuffers()), 64), "rt_read_aovs")
        r.upload_scene(cornell_scene(True))
        with pytest.raises(engine.RtError, match="bad image geometry"):
            r.render_aovs(pc, 0, 8, nRows=1)
        with pytest.raises(engine.RtError, match="rows exceed the image"):
            r.render_aovs(pc, 8, 8, row0=8, nRows=1)
        with pytest.raises(engine.RtError, match="rows exceed the image"):
            r.render_aovs(pc, 8, 8, row0=1, rowStride=4, nRows=3)
        for field, extra in (("objectCount", (0, 1)), ("sphereCount", (1, 0))):
            pc.rayTraceParams.sphereCount = r._counts["spheres"] + extra[0]
            pc.rayTraceParams.objectCount = r._counts["objects"] + extra[1]
            assert r._l.rt_render_aovs(r._h, C.byref(pc), 8, 8, 0, 1, 8, None) != 0
            assert f"{field} exceeds" in r._l.rt_last_error(r._h).decode()
        a = r.render_aovs(engine.push_constants(8, 8), 8, 8)   # the context is still good
        assert a["depth"].shape == (8, 8) and a["hit"].any()
        buf = np.zeros((63, 4), np.float32)
        assert r._l.rt_read_aovs(r._h, C.byref(_capi.RtAovBuffers(normalDepth=buf.ctypes.data)), 63) != 0
        assert "size mismatch" in r._l.rt_last_error(r._h).decode()
    finally:
        r.close()
