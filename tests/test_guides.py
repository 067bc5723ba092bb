"""Mirror-following guide planes (rt_render_guides / rt_read_guides, Renderer.render_guides, InteractiveSession(mirror_guides=N),
render.py --guide-bounces; DESIGN.md, "Mirror-following guide planes").

The pass follows each pixel's camera ray through the scene's mirrors, as shade_path reflects it, to the first surface that is no
mirror, and writes that surface's record where rt_render_aovs writes the first hit's. `follow` (tests/guides_cases.py, with the scenes
and the cameras, which tests/test_guides_float64.py shares) restates it on the CPU: it chains the
oracle's calculateIntersections (pyoracle.trace_rays) with the reflect and the origin offset in numpy float32, in the kernel's order.
Every comparison against it is exact, ids and float bits alike, and so are the counters: the sums over all rays of all chains."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import _capi, devmem, engine, render
from ray_tracer_amd.session import InteractiveSession

from aov_cases import PLANES, _as_hits, _check_misses, _upload
from denoise_float64 import planes_of, restate
from guides_cases import COUNTERS, HALL_CAMERA, HIT_FIELDS, MIRROR, as_guides, camera_rays, f32, follow, hall_of_mirrors, metal_quad
from temporal_float64 import camera_path, emission_of
from util import assert_hits_equal, cornell_scene, device_buffers, frames_between_passes, model_scene


def mse_table(noisy, clean, first, guides, emission):
    """The denoiser (float64 restatement) guided by the first-hit planes and by the guide planes, against the clean frame, all clamped
    to [0, 1]: the MSEs on the pixels whose chain has a mirror segment and on the rest."""
    c = lambda x: np.clip(np.asarray(x, np.float64)[..., :3], 0.0, 1.0)  # noqa: E731
    mask = guides["bounces"] >= 1
    den = {k: restate(noisy, *planes_of(a), emission)[0] for k, a in (("first", first), ("guides", guides))}
    mse = lambda x, m: float(((c(x) - c(clean))[m] ** 2).mean())  # noqa: E731
    return dict(mask_pixels=int(mask.sum()), noisy_mask=mse(noisy, mask), first_mask=mse(den["first"], mask), guides_mask=mse(den["guides"], mask),
                first_rest=mse(den["first"], ~mask), guides_rest=mse(den["guides"], ~mask))


# ---------------------------------------------------------------- CPU
def test_bindings_and_header_agree():
    assert "rt_render_guides" in _capi.SYMBOLS and "rt_read_guides" in _capi.SYMBOLS
    assert len(_capi.SYMBOLS["rt_render_guides"][1]) == 10


def test_follow_on_the_hall_of_mirrors():
    """The scene of the GPU test is right: at 8 bounces some chains are cut on a mirror with L = 8, others end earlier, and with
    no bounce allowed every mirror hit is a cut chain of length 0 whose record is the first hit's."""
    W, H = 64, 48
    s = hall_of_mirrors()
    o, d = camera_rays(engine.push_constants(W, H, **HALL_CAMERA), W, H)
    ref = follow(s, o, d, 8)
    assert ((ref["bounces"] == 8) & ref["cut"]).sum() > 20 and ((ref["bounces"] < 8) & (ref["bounces"] > 0)).sum() > 100
    assert not (ref["cut"] & (ref["bounces"] < 8)).any()
    long = ref["bounces"] >= 2
    assert np.all(ref["depth"][long & (ref["didHit"] == 1)] > ref["dst"][long & (ref["didHit"] == 1)])
    zero = follow(s, o, d, 0)
    assert_hits_equal({k: zero[k] for k in HIT_FIELDS}, {k: zero["first"][k] for k in HIT_FIELDS})
    assert not zero["bounces"].any() and zero["cut"].sum() > 100
    assert np.array_equal(zero["depth"].view(np.uint32), zero["first"]["dst"].view(np.uint32))


def test_follow_reads_the_metalness_map():
    W, H = 64, 48
    s, m, tex = metal_quad()
    o, d = camera_rays(engine.push_constants(W, H), W, H)
    ref = follow(s, o, d, 4, tex)
    quad = (ref["first"]["didHit"] == 1) & (ref["first"]["materialIndex"] == m)
    assert (quad & (ref["bounces"] == 1)).sum() >= 80 and (quad & (ref["bounces"] == 0)).sum() >= 80
    assert not follow(s, o, d, 4)["bounces"].any()   # without the table nothing binds: reflectance 0


def test_guide_bounces_flag():
    assert render.build_parser().parse_args([]).guide_bounces == 0
    assert render.build_parser().parse_args(["--denoise", "--guide-bounces", "3"]).guide_bounces == 3
    with pytest.raises(SystemExit, match="needs --denoise"):
        render.main(["--scene", "cornell", "--guide-bounces", "2"])
    with pytest.raises(SystemExit, match="0..8"):
        render.main(["--scene", "cornell", "--denoise", "--guide-bounces", "9"])


def test_what_it_is_for_on_the_cpu():
    """DESIGN.md's table from the oracle's frames, follow() and the denoiser's float64 restatement: on the pixels that show a
    reflection the guided denoiser leaves less than 0.6 of the error the first-hit planes leave, and the rest of the frame moves by
    less than 2 %. (Measured: 0.42 and 1.003.)"""
    W, H = 160, 120
    s = cornell_scene(True)
    noisy, _ = pyoracle.render(s, camera_path(W, H, 7, raysPerPixel=4), W, H)
    clean, _ = pyoracle.render(s, camera_path(W, H, 7, singleRender=1, sampleLimit=1024), W, H)
    pc = camera_path(W, H, 7)
    o, d = camera_rays(pc, W, H)
    first, guides = as_guides(follow(s, o, d, 0), (H, W), s), as_guides(follow(s, o, d, 4), (H, W), s)
    q = mse_table(noisy, clean, first, guides, emission_of(s))
    print(q)
    assert q["mask_pixels"] >= 500, q
    assert q["guides_mask"] < 0.6 * q["first_mask"], q
    assert q["guides_rest"] <= 1.02 * q["first_rest"], q


# ---------------------------------------------------------------- GPU: parity with the restatement
def _same_as_follow(renderer, s, pc, W, H, max_bounces, what, textures=(), **tile):
    """One pass against follow() on the pass's own camera rays (camInfo.pos, the first-hit rayDir plane): every plane, the counters,
    and the first-hit planes against rt_render_aovs."""
    renderer.reset_counters()
    g, first = renderer.render_guides(pc, W, H, max_bounces, first_hit=True, **tile)
    c = renderer.counters()
    a = renderer.render_aovs(pc, W, H, **tile)
    for k in PLANES:
        assert np.array_equal(first[k].view(np.uint8), a[k].view(np.uint8)), (what, "first hit", k)
    d = np.ascontiguousarray(a["ray_dir"].reshape(-1, 3))
    o = np.tile(np.array(list(pc.camInfo.pos), f32), (len(d), 1))
    ref = follow(s, o, d, max_bounces, textures)
    assert_hits_equal(_as_hits(g), {k: (ref["depth"] if k == "dst" else ref[k]) for k in _as_hits(g)})
    _check_misses(g)
    want = as_guides(ref, a["depth"].shape, s)
    for k in ("ray_dir", "albedo", "depth"):
        assert np.array_equal(g[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
    assert np.array_equal(g["bounces"], want["bounces"]) and np.array_equal(g["cut"], want["cut"]), what
    assert {k: c[k] for k in COUNTERS} == ref["counters"], what
    assert (c["raysReference"], c["paths"], c["segments"], c["emitterTests"], c["traceLaunches"]) == (0, 0, 0, 0, max_bounces + 1), what
    return g, a, ref


@pytest.mark.gpu
@pytest.mark.parametrize("max_bounces", [0, 1, 4])
def test_cornell_spheres(renderer, max_bounces):
    s = cornell_scene(True)
    W, H = 64, 48
    renderer.upload_scene(s)
    g, a, _ = _same_as_follow(renderer, s, engine.push_constants(W, H), W, H, max_bounces, f"cornell {max_bounces}")
    mirror = a["hit"] & (a["material"] == MIRROR)
    assert mirror.sum() > 50
    if max_bounces == 0:   # the first-hit planes, up to bit 3
        for k in PLANES:
            assert np.array_equal(g[k].view(np.uint8), a[k].view(np.uint8)), k
        assert np.array_equal(g["cut"], mirror) and not g["bounces"].any()
    else:
        assert np.array_equal(g["bounces"] >= 1, mirror) and (g["bounces"] <= 1).mean() > 0.98
        assert not np.array_equal(g["normal"], a["normal"])


@pytest.mark.gpu
def test_hall_of_mirrors(renderer):
    s = hall_of_mirrors()
    W, H = 64, 48
    _upload(renderer, s)
    g, _, _ = _same_as_follow(renderer, s, engine.push_constants(W, H, **HALL_CAMERA), W, H, 8, "hall of mirrors")
    assert ((g["bounces"] == 8) & g["cut"]).any() and ((g["bounces"] > 0) & (g["bounces"] < 8)).any()
    assert not (g["cut"] & (g["bounces"] < 8)).any()


@pytest.mark.gpu
def test_mirror_bunny_with_interpolated_normals(renderer):
    s = model_scene("bunny.obj", material=MIRROR, spheres=True)
    W, H = 64, 48
    renderer.upload_scene(s)
    g, _, _ = _same_as_follow(renderer, s, engine.push_constants(W, H), W, H, 4, "mirror bunny")
    assert (g["bounces"] >= 1).sum() > 100 and (g["bounces"] >= 2).any()


@pytest.mark.gpu
def test_metalness_map_decides(renderer):
    s, m, tex = metal_quad()
    W, H = 64, 48
    renderer.upload_scene(s)
    pc = engine.push_constants(W, H)
    try:
        renderer.upload_textures(tex)
        pyoracle.set_textures(tex)
        g, a, _ = _same_as_follow(renderer, s, pc, W, H, 4, "metalness map", tex)
        quad = a["hit"] & (a["material"] == m)
        assert (quad & (g["bounces"] == 1)).sum() >= 80 and (quad & (g["bounces"] == 0)).sum() >= 80
        renderer.upload_textures([])   # nothing bound: the material's own reflectance, 0
        g, _, _ = _same_as_follow(renderer, s, pc, W, H, 4, "metalness map gone")
        assert not g["bounces"].any()
    finally:
        pyoracle.set_textures([])
        renderer.upload_textures([])


@pytest.mark.gpu
def test_scene_without_mirrors(renderer):
    s = model_scene("bunny.obj")
    W, H = 64, 48
    renderer.upload_scene(s)
    g, a, _ = _same_as_follow(renderer, s, engine.push_constants(W, H), W, H, 8, "no mirrors")
    for k in PLANES:
        assert np.array_equal(g[k].view(np.uint8), a[k].view(np.uint8)), k
    assert not g["bounces"].any() and not g["cut"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (1, 67), (16, 16)])
def test_small_frames_and_tiles(renderer, W, H):
    s = cornell_scene(True)
    renderer.upload_scene(s)
    # narrow and turned, so that the frame's bottom left corner, which is all a 1 x 1 frame has, looks at the mirror sphere
    pc = engine.push_constants(W, H, fov=25.0, aspectRatio=1.0, cameraAngles=(18.0, -20.0, 0.0))
    full, _, _ = _same_as_follow(renderer, s, pc, W, H, 4, f"{W} x {H}")
    assert full["bounces"].any()
    if H > 1:
        part, _, _ = _same_as_follow(renderer, s, pc, W, H, 4, f"{W} x {H} rows 1 + 3k", row0=1, rowStride=3)
        for k in full:
            assert np.array_equal(part[k].view(np.uint8), full[k][1::3].view(np.uint8)), k
        assert part["bounces"].any()


# ---------------------------------------------------------------- GPU: routes and side effects
@pytest.mark.gpu
def test_device_ctx_owned_and_null_field_routes_agree(renderer):
    import torch  # noqa: F401  (as tests/test_aovs.py: devmem.hip must not take the second copy of the HIP runtime now in the process)
    renderer.upload_scene(cornell_scene(True))
    W, H = 40, 30
    pc = engine.push_constants(W, H)
    ref, first = renderer.render_guides(pc, W, H, 4, first_hit=True)
    nbytes = H * W * 16
    names = [f"g_{k}" for k in engine.AOV_PLANES] + [f"f_{k}" for k in engine.AOV_PLANES]
    with device_buffers(names, nbytes, fill=7) as bufs:
        def fetch(b, dtype):
            return b.download((H, W, 4), dtype)

        def planes(prefix, only=engine.AOV_PLANES):
            return _capi.RtAovBuffers(**{k: bufs[f"{prefix}_{k}"].ptr for k in only})

        def run(guides, first_hit):
            renderer.fill_counts(pc)
            renderer._check(renderer._l.rt_render_guides(renderer._h, C.byref(pc), W, H, 0, 1, H, 4, C.byref(guides) if guides else None,
                                                         C.byref(first_hit) if first_hit else None), "rt_render_guides")
            renderer.sync()

        run(planes("g"), planes("f"))
        got = {k: fetch(bufs[f"g_{k}"], np.uint32 if k == "ids" else np.float32) for k in engine.AOV_PLANES}
        assert np.array_equal((got["ids"][..., 3] >> 8) & 15, ref["bounces"]) and np.array_equal(got["ids"][..., 3] & 8 != 0, ref["cut"])
        got, got_first = engine.aovs_to_numpy(got), engine.aovs_to_numpy({k: fetch(bufs[f"f_{k}"], np.uint32 if k == "ids" else np.float32)
                                                                          for k in engine.AOV_PLANES})
        for k in PLANES:
            assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k
            assert np.array_equal(got_first[k].view(np.uint8), first[k].view(np.uint8)), k
        # NULL fields are skipped: one guide plane and one first-hit plane, the others keep their fill
        for b in bufs.values():
            b.fill(7)
        devmem.synchronize()
        run(planes("g", ["normalDepth"]), planes("f", ["ids"]))
        assert np.array_equal(fetch(bufs["g_normalDepth"], np.float32)[..., 3], ref["depth"])
        assert np.array_equal(fetch(bufs["f_ids"], np.uint32)[..., 0], first["object"])
        for k in ("g_position", "g_albedo", "g_rayDir", "g_ids", "f_normalDepth", "f_position", "f_albedo", "f_rayDir"):
            assert np.all(fetch(bufs[k], np.uint32) == 0x07070707), k   # (fetch copies 16 bytes per pixel: a 4-byte dtype)
        # d_guides alone (no first-hit planes wanted), and the ctx-owned set is still that of the last call that asked for it
        run(planes("g"), None)
        assert np.array_equal(fetch(bufs["g_normalDepth"], np.float32)[..., 3], ref["depth"])
        own = {k: np.empty((H, W, 4), np.uint32 if k == "ids" else np.float32) for k in engine.AOV_PLANES}
        b = _capi.RtAovBuffers(**{k: v.ctypes.data for k, v in own.items()})
        renderer._check(renderer._l.rt_read_guides(renderer._h, C.byref(b), H * W), "rt_read_guides")
        own = engine.aovs_to_numpy(own)
        for k in PLANES:
            assert np.array_equal(own[k].view(np.uint8), ref[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [-1, 0])
def test_passes_leave_rendering_untouched(renderer, pipeline):
    s = model_scene("bunny.obj", material=MIRROR, spheres=True)
    W, H = 64, 48
    renderer.set_tuning("pipeline", pipeline)

    def guide_passes(other, w, h):
        renderer.render_guides(other, w, h, 4)
        renderer.render_guides(other, w, h, 8, first_hit=True, row0=1, rowStride=2)

    try:
        a = frames_between_passes(renderer, s, W, H)
        b = frames_between_passes(renderer, s, W, H, guide_passes)
    finally:
        renderer.set_tuning("pipeline", -1)
    for fa, fb in zip(a[0], b[0]):
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert a[1] == b[1]
    assert a[2] == b[2]


@pytest.mark.gpu
def test_pass_leaves_the_framebuffer_and_the_first_hit_planes(renderer):
    s = cornell_scene(True)
    W, H = 64, 48
    renderer.upload_scene(s)
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2)
    frame = renderer.render(pc, W, H)
    a = renderer.render_aovs(pc, W, H)
    den = renderer.denoise()
    state = lambda: (renderer.last_pipeline(), renderer.last_parts(), renderer.ray_cost())  # noqa: E731
    before = state()
    g = renderer.render_guides(engine.push_constants(W, H, cameraAngles=(10.0, 20.0, 0.0)), W, H, 4)
    assert state() == before
    assert np.array_equal(renderer.read_rgba().view(np.uint32), frame.view(np.uint32))
    again = renderer.read_aovs()
    for k in a:
        assert np.array_equal(again[k].view(np.uint8), a[k].view(np.uint8)), k
    assert np.array_equal(renderer.denoise().view(np.uint32), den.view(np.uint32))   # d_aovs = NULL still means the first-hit planes
    assert not np.array_equal(g["normal"], a["normal"])


# ---------------------------------------------------------------- GPU: errors
@pytest.mark.gpu
def test_errors(built):
    r = engine.Renderer(0)
    try:
        pc = engine.push_constants(8, 8)
        l, h = r._l, r._h

        def refused(message, *args):
            a = dict(W=8, H=8, row0=0, stride=1, nRows=8, mb=4, guides=None, first=None)
            a.update(dict(zip(("W", "H", "row0", "stride", "nRows", "mb", "guides", "first"), args)))
            assert l.rt_render_guides(h, C.byref(pc), a["W"], a["H"], a["row0"], a["stride"], a["nRows"], a["mb"], a["guides"], a["first"]) != 0
            assert message in l.rt_last_error(h).decode(), (message, l.rt_last_error(h).decode())

        refused("rt_render_guides before rt_upload_scene")
        assert l.rt_read_guides(h, C.byref(_capi.RtAovBuffers()), 64) != 0
        assert "no ctx-owned guide planes" in l.rt_last_error(h).decode()
        r.upload_scene(cornell_scene(True))
        r.fill_counts(pc)
        refused("rt_render_guides: maxBounces must be 0..8", 8, 8, 0, 1, 8, 9)
        refused("rt_render_guides: maxBounces must be 0..8", 0, 8, 0, 1, 8, 9)   # before the geometry
        refused("rt_render_guides: bad image geometry", 0, 8, 0, 1, 1)
        refused("rt_render_guides: bad image geometry", 8, 8, 0, 0, 1)
        refused("rt_render_guides: rows exceed the image", 8, 8, 8, 1, 1)
        refused("rt_render_guides: rows exceed the image", 8, 8, 1, 4, 3)
        refused("rt_render_guides: tile too large", 1 << 15, 1 << 15, 0, 1, 1 << 15)
        for field, extra in (("objectCount", (0, 1)), ("sphereCount", (1, 0))):
            pc.rayTraceParams.sphereCount = r._counts["spheres"] + extra[0]
            pc.rayTraceParams.objectCount = r._counts["objects"] + extra[1]
            refused(f"{field} exceeds")
        r.fill_counts(pc)
        base = 0x7000000000   # made-up addresses: a refused call touches no plane
        g = _capi.RtAovBuffers(normalDepth=base, ids=base + 4 * 64 * 16)
        refused("rt_render_guides: d_guides.ids overlaps d_firstHit.position", 8, 8, 0, 1, 8, 4, C.byref(g),
                C.byref(_capi.RtAovBuffers(position=base + 4 * 64 * 16 + 16, albedo=base + 64 * 16)))
        refused("rt_render_guides: d_guides.normalDepth overlaps d_firstHit.normalDepth", 8, 8, 0, 1, 8, 4, C.byref(g), C.byref(g))
        a = r.render_guides(engine.push_constants(8, 8), 8, 8)   # the context is still good
        assert a["depth"].shape == (8, 8) and a["hit"].any()
        buf = np.zeros((63, 4), np.float32)
        assert l.rt_read_guides(h, C.byref(_capi.RtAovBuffers(normalDepth=buf.ctypes.data)), 63) != 0
        assert "rt_read_guides: size mismatch" in l.rt_last_error(h).decode()
    finally:
        r.close()


# ---------------------------------------------------------------- GPU: what it is for
@pytest.mark.gpu
def test_reflections_keep_their_edges(renderer):
    """DESIGN.md's table on the GPU: one 4-spp frame of cornell_scene(True) at pose 7 of camera_path, denoised with the first-hit
    planes and with the guide planes, against 1024 spp, clamped. Measured on the oracle's frames with the restatements (the kernels
    are pinned to them at 1e-4): 0.42 x on the pixels with a mirror segment, 1.003 x on the rest."""
    W, H = 160, 120
    s = cornell_scene(True)
    renderer.upload_scene(s)
    clean = renderer.render(camera_path(W, H, 7, singleRender=1, sampleLimit=1024), W, H)
    noisy = renderer.render(camera_path(W, H, 7, raysPerPixel=4), W, H)
    guides, first = renderer.render_guides(camera_path(W, H, 7), W, H, 4, first_hit=True)
    den_first, den_guides = renderer.denoise(noisy, first), renderer.denoise(noisy, guides)
    mask = guides["bounces"] >= 1
    c = lambda x: np.clip(np.asarray(x, np.float64)[..., :3], 0.0, 1.0)  # noqa: E731
    mse = lambda x, m: float(((c(x) - c(clean))[m] ** 2).mean())  # noqa: E731
    q = dict(mask_pixels=int(mask.sum()), noisy_mask=mse(noisy, mask), first_mask=mse(den_first, mask), guides_mask=mse(den_guides, mask),
             noisy_rest=mse(noisy, ~mask), first_rest=mse(den_first, ~mask), guides_rest=mse(den_guides, ~mask),
             first_frame=mse(den_first, Ellipsis), guides_frame=mse(den_guides, Ellipsis))
    print(q)
    assert q["mask_pixels"] >= 500, q
    assert q["guides_mask"] < 0.6 * q["first_mask"], q
    assert q["guides_rest"] <= 1.02 * q["first_rest"], q


# ---------------------------------------------------------------- GPU: session and CLI
@pytest.mark.gpu
def test_session_with_mirror_guides(renderer):
    s = cornell_scene(True)
    W, H = 64, 48

    def frames(denoise=True, **kw):
        ses = InteractiveSession(renderer, s, W, H, temporal=True, denoise=denoise, **kw)
        out = []
        for k in range(3):
            ses.frame(keys="W", frame_time_ms=2.0)
            out.append((ses.filtered.copy(), ses.image.copy(), ses.history_length.copy()))
        return ses, out

    _, plain = frames()
    _, zero = frames(mirror_guides=0)
    for (fa, ia, na), (fb, ib, nb) in zip(plain, zero):
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
    ses, four = frames(mirror_guides=4)
    for (fa, ia, na), (fb, ib, nb) in zip(plain, four):   # the same frames into the same history: the temporal pass takes the first-hit planes
        assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)) and np.array_equal(na, nb)
    assert not np.array_equal(plain[-1][0], four[-1][0])
    # the last frame by hand: the temporal pass's output of the same sequence through denoise with the guide planes of its camera
    hand, accumulated = frames(denoise=False)
    assert bytes(hand.pc) == bytes(ses.pc)
    by_hand = renderer.denoise(accumulated[-1][0], renderer.render_guides(hand.pc, W, H, 4))
    assert np.array_equal(by_hand.view(np.uint32), four[-1][0].view(np.uint32))
    only = InteractiveSession(renderer, s, W, H, denoise=True, mirror_guides=4)
    only.frame()
    assert np.array_equal(only.filtered.view(np.uint32), renderer.denoise(only.image, renderer.render_guides(only.pc, W, H, 4)).view(np.uint32))


@pytest.mark.gpu
def test_cli_guide_bounces(tmp_path):
    job = "--scene cornell --width 56 --height 37 --single-render --sample-limit 2 --denoise"
    first, guided = tmp_path / "first.npy", tmp_path / "guided.npy"
    assert render.main(f"{job} --out {first}".split()) == 0
    assert render.main(f"{job} --guide-bounces 4 --out {guided}".split()) == 0
    a, b = np.load(first), np.load(guided)
    assert a.shape == b.shape == (37, 56, 4) and not np.array_equal(a, b)
