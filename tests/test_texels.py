"""Lightmap texels on the device: rt_bake_texels, rt_texels_compact, rt_texels_scatter, rt_dilate_texels and rt_bake_lightmap
(Renderer.bake_texels, texels_compact, texels_scatter, dilate_texels, bake_lightmap; include/rt_amd.h, DESIGN.md "Lightmap texels").

The rule is integer coverage and a record computed by one text both sides compile (include/rt_texels.h), and the exhaustive host
loop is held to float64 on the CPU (tests/test_texels_host.py), so every test here asks for every byte. The meshes and maps are
tests/texels_cases.py's: maps that are no multiple of the 8 x 8 block or of a work-group (37 x 23), a single texel, a single
row of 8192, and for M a 1024 x 1024 map on which one triangle is 2^14 work items while 3 000 others are one each, so that the
scan runs over several work-groups and levels."""
import math

import numpy as np
import pytest

from ray_tracer_amd import _capi, devmem, engine

import irradiance_float64 as f64
import texels_cases as tc
from util import EditedScene, bits

REC = 48


def _raw(recs, n):
    return np.frombuffer(recs, dtype=np.uint32).reshape(n, 12).copy() if n else np.zeros((0, 12), np.uint32)


def _same_records(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} records differ, first at {bad[:5].tolist()}: {got[bad[0]].tolist()} against {want[bad[0]].tolist()}"


def _device_bake(r, w, h, obj=0):
    """rt_bake_texels into device memory the test owns, with a guard record after the map"""
    n = w * h
    with devmem.DeviceBuffer(REC * (n + 1)) as d:
        d.fill(0xAB)
        st = r.bake_texels(obj, w, h, out=d.ptr)
        raw = d.download((n + 1, 12), np.uint32)
    assert (raw[n] == 0xABABABAB).all(), "the bake wrote past the map"
    return raw[:n], st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["Q", "Qid", "G", "G2", "S", "M"])
def test_bake_equals_the_exhaustive_host_loop_in_every_byte(renderer, name):
    """Through the _host form and through device pointers, at every map; the statistics too. Q and both G are watertight."""
    s = tc.scene(name)
    renderer.upload_scene(s)
    for w, h in tc.MAPS + ((tc.BIG_MAP,) if name == "M" else ()):
        want, wst = engine.texels_exhaustive(s.arrays(), 0, w, h)
        want = _raw(want, w * h)
        recs, st = renderer.bake_texels(0, w, h)
        _same_records(_raw(recs, w * h), want, f"{name} {w} x {h}, host form")
        assert st == wst, (name, w, h, st, wst)
        got, st = _device_bake(renderer, w, h)
        _same_records(got, want, f"{name} {w} x {h}, device pointers")
        assert st == wst, (name, w, h, st, wst)
        if name in ("Q", "Qid", "G", "G2"):
            assert st["covered"] == w * h and st["overlapped"] == 0 and st["skippedTriangles"] == 0
        empty = want[want[:, 3] == 0]
        assert not empty.any(), "an empty record has every field 0"
    if name == "S":
        assert wst["skippedTriangles"] >= 3 and wst["overlapped"] > 0
    if name == "M":
        assert wst["covered"] == tc.BIG_MAP[0] * tc.BIG_MAP[1]


@pytest.mark.gpu
def test_bake_into_torch_tensors(renderer):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    s = tc.scene("S")
    renderer.upload_scene(s)
    w, h = 37, 23
    out = torch.zeros((h * w, 12), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = renderer.bake_texels(0, w, h, out=out)
    want, wst = engine.texels_exhaustive(s.arrays(), 0, w, h)
    _same_records(out.cpu().numpy().view(np.uint32), _raw(want, w * h), "S 37 x 23, torch tensor")
    assert st == wst


@pytest.mark.gpu
def test_after_update_objects_the_records_follow_the_moved_object(renderer):
    s = EditedScene(tc.scene("S"))
    renderer.upload_scene(s)
    w, h = 64, 64
    before = _raw(engine.texels_exhaustive(s.arrays(), 0, w, h)[0], w * h)
    _same_records(_device_bake(renderer, w, h)[0], before, "before the move")
    s.set_transform(0, engine.placement(position=(-1.0, 0.4, 0.2), rotation=(-35, 10, 80), scale=(0.6, 1.9, 1.1)))
    s.push(renderer, "objects")
    after = _raw(engine.texels_exhaustive(s.arrays(), 0, w, h)[0], w * h)
    assert (after != before).any() and np.array_equal(after[:, 3], before[:, 3]), "the move changes points and normals, not the coverage"
    _same_records(_device_bake(renderer, w, h)[0], after, "after the move")


def _planes(rng, w, h, share=0.3):
    fill = (rng.random((h, w)) < share).astype(np.uint8)
    rgba = rng.uniform(0, 4, (h, w, 4)).astype(np.float32) * fill[..., None]
    return rgba, fill


@pytest.mark.gpu
def test_compact_scatter_and_dilate_equal_the_host_forms(renderer):
    """Compaction in numpy's nonzero order (a scan over several work-groups: 64 x 64 and 8192 x 1; one texel; 37 x 23), scatter and
    0, 1 and 3 dilation passes against the host rule in every bit."""
    s = tc.scene("S")
    renderer.upload_scene(s)
    rng = np.random.default_rng(3)
    for w, h in tc.MAPS:
        n = w * h
        recs, _ = engine.texels_exhaustive(s.arrays(), 0, w, h)
        raw = _raw(recs, n)
        d = engine.texels_to_numpy(raw)
        order = np.flatnonzero(d["state"])
        with devmem.DeviceBuffer(REC * n) as dt, devmem.DeviceBuffer(12 * n) as dp, devmem.DeviceBuffer(12 * n) as dn, \
                devmem.DeviceBuffer(4 * n) as di, devmem.DeviceBuffer(4) as dc, devmem.DeviceBuffer(16 * n) as dv, \
                devmem.DeviceBuffer(16 * n) as drgba, devmem.DeviceBuffer(n) as dfill:
            dt.upload(raw)
            for b in (dp, dn, di):
                b.fill(0xCD)
            renderer.texels_compact(dt.ptr, n, dp.ptr, dn.ptr, di.ptr, dc.ptr)
            k = int(dc.download((1,), np.uint32)[0])
            assert k == len(order), (w, h, k, len(order))
            assert np.array_equal(di.download((n,), np.uint32)[:k], order.astype(np.uint32)), f"{w} x {h}: not nonzero's order"
            assert np.array_equal(bits(dp.download((n, 3), np.float32)[:k]), bits(d["point"][order]))
            assert np.array_equal(bits(dn.download((n, 3), np.float32)[:k]), bits(d["normal"][order]))
            assert (di.download((n,), np.uint32)[k:] == 0xCDCDCDCD).all(), "the compaction wrote past the count"
            values = rng.uniform(0, 3, (max(k, 1), 4)).astype(np.float32)
            dv.upload(values)
            drgba.fill(0xEE)
            dfill.fill(0xEE)
            renderer.texels_scatter(n, k, di.ptr, dv.ptr, drgba.ptr, dfill.ptr)
            want = np.zeros((n, 4), np.float32)
            want[order] = values[:k]
            wfill = np.zeros(n, np.uint8)
            wfill[order] = 1
            assert np.array_equal(bits(drgba.download((n, 4), np.float32)), bits(want)), f"{w} x {h}: scatter"
            assert np.array_equal(dfill.download((n,), np.uint8), wfill)
            for passes in (0, 1, 3):
                rgba, fill = _planes(rng, w, h)
                drgba.upload(rgba)
                dfill.upload(fill)
                renderer.dilate_texels(w, h, passes, drgba.ptr, dfill.ptr)
                wr, wf = engine.dilate_texels(rgba, fill, passes)
                assert np.array_equal(dfill.download((h, w), np.uint8), wf), f"{w} x {h}, {passes} passes: fill"
                assert np.array_equal(bits(drgba.download((h, w, 4), np.float32)), bits(wr)), f"{w} x {h}, {passes} passes"
                if passes:
                    assert (wf > 1).any() or fill.all() or not fill.any()


def _lit(scene):
    """a ground sphere and a small light above the mesh, so that the irradiance varies over the map"""
    glow = scene.add_material(engine.default_material(emissionColor=(1.0, 0.9, 0.7), emissionStrength=6.0))
    scene.set_sphere(0, (0.3, -3.0, 1.5), 0.8, glow)
    scene.set_sphere(1, (0.0, 103.0, 0.0), 100.0, 0)


SKY = dict(lightDir=(0.3, 0.8, -0.5, 1.0), horizonColor=(0.9, 0.8, 0.7, 40.0), zenithColor=(0.2, 0.4, 0.9, 5.0), groundColor=(0.3, 0.25, 0.2))


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [1, 5, 64])
def test_lightmap_equals_the_composition_by_hand_and_the_host_texels(renderer, samples):
    """rt_bake_lightmap against its five parts called one by one on device memory, and against query_irradiance's _host form over the
    exhaustive host texels with ids = index, scattered and dilated by the host rule: every bit, 2 dilation passes."""
    s = tc.scene("S", _lit)
    renderer.upload_scene(s)
    env = engine.push_constants(8, 8, **SKY).environment
    w, h, passes, n = 37, 23, 2, 37 * 23
    p = _capi.RtIrradianceParams(samples, 3, 0, 1, 1e-4)
    rgba, fill, st = renderer.bake_lightmap(0, w, h, params=p, env=env, dilate=passes)
    # by hand
    with devmem.DeviceBuffer(REC * n) as dt, devmem.DeviceBuffer(12 * n) as dp, devmem.DeviceBuffer(12 * n) as dn, devmem.DeviceBuffer(4 * n) as di, \
            devmem.DeviceBuffer(4) as dc, devmem.DeviceBuffer(16 * n) as dv, devmem.DeviceBuffer(16 * n) as drgba, devmem.DeviceBuffer(n) as dfill:
        hst = renderer.bake_texels(0, w, h, out=dt.ptr)
        renderer.texels_compact(dt.ptr, n, dp.ptr, dn.ptr, di.ptr, dc.ptr)
        k = int(dc.download((1,), np.uint32)[0])
        renderer.query_irradiance(dp.ptr, dn.ptr, samples=samples, bounces=3, ids=di.ptr, frame=1, bias=1e-4, environment=env, n=k, out=dv.ptr)
        renderer.texels_scatter(n, k, di.ptr, dv.ptr, drgba.ptr, dfill.ptr)
        renderer.dilate_texels(w, h, passes, drgba.ptr, dfill.ptr)
        hand, hfill = drgba.download((h, w, 4), np.float32), dfill.download((h, w), np.uint8)
    assert st == hst and k == st["covered"]
    assert np.array_equal(fill, hfill) and np.array_equal(bits(rgba), bits(hand)), f"S = {samples}: the composite differs from its parts"
    # over the host texels
    recs, wst = engine.texels_exhaustive(s.arrays(), 0, w, h)
    d = engine.texels_to_numpy(recs)
    order = np.flatnonzero(d["state"]).astype(np.uint32)
    E = renderer.query_irradiance(np.ascontiguousarray(d["point"][order]), np.ascontiguousarray(d["normal"][order]), samples=samples, bounces=3,
                                  ids=order, frame=1, bias=1e-4, environment=env)
    flat = np.zeros((n, 4), np.float32)
    flat[order] = E
    f0 = np.zeros(n, np.uint8)
    f0[order] = 1
    wr, wf = engine.dilate_texels(flat.reshape(h, w, 4), f0.reshape(h, w), passes)
    assert st == wst
    assert np.array_equal(fill, wf) and np.array_equal(bits(rgba), bits(wr)), f"S = {samples}: the composite differs from the host texels' light"
    if samples == 64:
        lit = rgba[fill == 1][:, :3]
        assert np.isfinite(rgba).all() and lit.max() > 0 and len(np.unique(bits(lit[:, :1]))) > len(lit) // 2
        assert (rgba[fill == 1][:, 3] == 1.0).all() and (rgba[fill > 1][:, 3] == 0.0).all() and (fill > 1).any()


@pytest.mark.gpu
def test_lightmap_of_a_quad_under_a_constant_sky_is_pi_L(renderer):
    """Q alone under a sky of one colour L with nothing else in reach: every ray of every texel leaves the scene (the quad is a
    sheet: a ray that starts on it and leaves along its normal's hemisphere may still meet the curved sheet again, so the sheet
    here is flat), and E = pi L within the irradiance tests' derived bound: tests/irradiance_float64.py's for the sum plus 6 u pi |L|
    for the records' own roundings (tests/test_irradiance.py)."""
    uv = tc.quad_uvs()
    pos = np.stack([2 * uv[..., 0] - 1, np.zeros(uv.shape[:2]), 2 * uv[..., 1] - 1], -1).astype(np.float32)
    nrm = np.zeros_like(pos)
    nrm[..., 1] = -1.0                                    # up is -y
    s = engine.Scene()
    s.add_material(engine.default_material())
    s.add_mesh("flat", pos, nrm, engine.placement(**tc.PLACED), 0, uvs=uv)
    renderer.upload_scene(s)
    L = np.array((0.75, 2.0, 0.125), np.float32)
    env = engine.push_constants(8, 8, lightDir=(0.0, 1.0, 0.0, 1.0), horizonColor=(*L, 1.0), zenithColor=(*L, 0.0), groundColor=tuple(L)).environment
    w, h, S = 37, 23, 65
    p = _capi.RtIrradianceParams(S, 3, 0, 0, 1e-4)
    rgba, fill, st = renderer.bake_lightmap(0, w, h, params=p, env=env, dilate=0)
    assert st["covered"] == w * h and (fill == 1).all()
    rad = np.ones((w * h * S, 4), np.float32)
    rad[:, :3] = L
    _, bound = f64.irradiance(rad, w * h, S)
    L64 = L.astype(np.float64)
    err = np.abs(rgba.reshape(-1, 4)[:, :3] - math.pi * L64)
    print(f"E off by at most {(err / (bound + 6 * f64.U * math.pi * L64)).max():.3f} of the bound")
    assert (err <= bound + 6 * f64.U * math.pi * L64).all(), err.max()


@pytest.mark.gpu
def test_a_render_before_and_after_is_bit_identical(renderer):
    s = tc.scene("S", _lit)
    renderer.upload_scene(s)
    pc = engine.push_constants(48, 32, singleRender=1, sampleLimit=2, pos=(0.0, -1.0, -4.0))
    renderer.clear_framebuffer()
    before = renderer.render(pc, 48, 32).copy()
    renderer.bake_texels(0, 64, 64)
    renderer.bake_lightmap(0, 37, 23, params=_capi.RtIrradianceParams(5, 3, 0, 0, 1e-4), dilate=3)
    renderer.clear_framebuffer()
    after = renderer.render(pc, 48, 32)
    assert before[..., :3].max() > 0 and np.array_equal(bits(before), bits(after))


@pytest.mark.gpu
def test_refusals_through_the_c_abi(renderer):
    renderer.upload_scene(tc.scene("Q"))
    for bad in ((5, 8, 8), (0, 0, 8), (0, 8, 8193)):
        with pytest.raises(engine.RtError):
            renderer.bake_texels(*bad)
    with pytest.raises(engine.RtError, match="one shot"):
        renderer.bake_lightmap(0, 8, 8, params=_capi.RtIrradianceParams(4, 3, 1, 0, 1e-4))
    with pytest.raises(engine.RtError, match="samples"):
        renderer.bake_lightmap(0, 8, 8, params=_capi.RtIrradianceParams(0, 3, 0, 0, 1e-4))
