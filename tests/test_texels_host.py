"""The lightmap texel passes' host-only unit and rule on the CPU (ray_tracer_amd/csrc/texel_queries.h, include/rt_texels.h):
tests/texels_check.cpp provokes every refusal in the stated order with its message, shows watertightness and the fill rule on a
quad and two grids, the lowest-index owner on hand-made overlaps, the dilation against passes written out by hand and the block
and scan arithmetic. Then the exhaustive host form (engine.texels_exhaustive) is held to the float64 restatement of
tests/texels_float64.py, whose docstring derives m = 1 / 256 texel and the bounds of the record; the share of ambiguous texels and
the largest fraction of each bound are printed ("Lightmap texels", quotes them). The second grid, whose uv vertices lie
on texel centres and corners of a 64 x 64 map so that edges pass through centres, is exempt from the float64 pin by design
and covered by watertightness instead (here and in texels_check.cpp). For the same reason the condition that at most 2 % of a
case's texels are ambiguous is not asked of Q on the 1 x 1 map: its only centre, (0.5, 0.5), lies on the diagonal the quad's two
triangles share, whichever diagonal that is and whatever the seed; its other checks run (on a 64 x 64 map the 64 centres on the
diagonal are 1.56 % of the texels). Nor is it asked of G on the 8192 x 1 map, where no seed can meet it: the map is one texel tall, so an
edge that crosses the row's centre line while it advances s texels per texel of height keeps 2 m s centres within m of itself, and
the edges of a tiling of five rows that cross the line advance 8192 texels between them over a fifth of a texel of height each:
2 m x 8192 / 0.2 = 320 centres, 3.9 %, whatever the vertices (G: 4.99 % measured; a single quad's diagonal, a whole texel tall,
gives 0.8 %, the soup 1.8 %). The shares are printed; every other check runs there on the texels that are not ambiguous."""
import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
import texels_cases as tc
import texels_float64 as f64


def test_texel_checks_on_the_cpu(tmp_path, built):
    """texel_queries.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they are
    installed."""
    exe = hostcheck.build(tmp_path, "texels_check", ["texel_queries.cpp"], "texels_check.cpp", rocm=False)
    hostcheck.run(exe, ok="texel queries ok")


@pytest.mark.parametrize("name", ["Q", "G", "G2", "Qid"])
def test_tilings_are_watertight_at_every_map(built, name):
    s = tc.scene(name)
    for w, h in tc.MAPS + (tc.BIG_MAP, (200, 300)):
        recs, st = engine.texels_exhaustive(s.arrays(), 0, w, h)
        assert st == dict(covered=w * h, overlapped=0, skippedTriangles=0, degenerateTexels=0), (name, w, h, st)
        assert (engine.texels_to_numpy(recs)["state"] == 1).all()


@pytest.mark.parametrize("name", ["Q", "G", "S", "M", "Qid"])
def test_host_form_agrees_with_the_float64_restatement(built, name):
    s = tc.scene(name)
    first, uv, pos, nrm, matrix = tc.scene_triangles(s)
    identity = name == "Qid"
    worst = dict(ambiguous=0.0, uv=0.0, point=0.0, normal=0.0)
    for w, h in tc.MAPS:
        what = f"{name} {w} x {h}"
        recs, st = engine.texels_exhaustive(s.arrays(), 0, w, h)
        d = engine.texels_to_numpy(recs)
        covered = d["state"] != 0
        owner = d["triIndex"].astype(np.int64) - first
        P, ok = f64.corners(uv, w, h)
        cls = f64.classify(P, ok, w, h)
        certain_in, certain_out = (cls == f64.IN).any(axis=0), (cls == f64.FAR).all(axis=0)
        share = 1.0 - float((certain_in | certain_out).mean())
        worst["ambiguous"] = max(worst["ambiguous"], share)
        print(f"{what}: {100 * share:.2f} % of the texels ambiguous, {int(covered.sum())} covered, {st}")
        if not (name in ("Q", "Qid") and (w, h) == (1, 1)) and not (name == "G" and (w, h) == (8192, 1)):   # (the module's docstring: two exceptions)
            assert share <= 0.02, f"{what}: {share:.4f} of the texels within m of an edge: choose other seeds"
        # a degenerate texel's owner covers it and has no normal: only the soup's last triangle may do that
        lost = certain_in & ~covered
        assert int(lost.sum()) <= st["degenerateTexels"] and (name == "S" or not lost.any()), f"{what}: {int(lost.sum())} certainly covered texels are empty"
        assert not (certain_out & covered).any(), f"{what}: {int((certain_out & covered).sum())} texels are covered though every triangle is more than m away"
        idx = np.flatnonzero(covered)
        assert (owner[idx] >= 0).all() and (owner[idx] < len(uv)).all()
        assert (cls[owner[idx], idx] != f64.FAR).all(), f"{what}: an owner is more than m away from its texel"
        lower = np.arange(len(uv))[:, None] < owner[idx][None, :]
        if name != "S":
            assert not ((cls[:, idx] == f64.IN) & lower).any(), f"{what}: a triangle below the owner certainly covers the texel"
        else:   # (the soup's degenerate triangle is the last one: nothing lies above it)
            assert not ((cls[:, idx] == f64.IN) & lower).any()
        assert ((d["state"][idx] == 3) | ~((cls[:, idx] == f64.IN).sum(axis=0) >= 2)).all(), f"{what}: two triangles certainly cover a texel that is not marked overlapped"
        if not len(idx):
            continue
        bu, bv = d["uv"][idx, 0], d["uv"][idx, 1]
        where, b_uv, point, b_point, normal, b_normal = f64.record_bounds(P, d["uv"][idx], owner[idx], pos, nrm, matrix, identity)
        ys, xs = np.divmod(idx, w)
        err = np.linalg.norm(where - np.stack([xs + 0.5, ys + 0.5], -1), axis=1)
        assert (err <= b_uv).all(), f"{what}: a record's uv is {err.max():.5f} texel from its centre"
        worst["uv"] = max(worst["uv"], float((err / b_uv).max()))
        bw = (np.float32(1.0) - bu) - bv
        h_uv = f64.hit_uv(uv, owner[idx], bu, bv, bw)
        assert np.array_equal(f64.tex_index(h_uv[:, 0], w), xs) and np.array_equal(f64.tex_index(np.float32(1.0) - h_uv[:, 1], h), ys), \
            f"{what}: rt_tex_index of hit_uv at the record's barycentrics is not the texel"
        err = np.abs(d["point"][idx].astype(np.float64) - point)
        assert (err <= b_point).all(), f"{what}: point off by {(err / b_point).max():.3f} of the bound"
        worst["point"] = max(worst["point"], float((err / b_point).max()))
        has = np.isfinite(b_normal)
        assert has.sum() > 0.9 * len(idx) or name == "S"
        err = np.linalg.norm(d["normal"][idx].astype(np.float64) - normal, axis=1)
        assert (err[has] <= b_normal[has]).all(), f"{what}: normal off by {(err[has] / b_normal[has]).max():.3f} of the bound"
        worst["normal"] = max(worst["normal"], float((err[has] / b_normal[has]).max()))
        length = np.linalg.norm(d["normal"][idx].astype(np.float64), axis=1)
        assert (np.abs(length - 1.0) < 4 * f64.U).all()
    print(f"{name}: largest ambiguous share {100 * worst['ambiguous']:.2f} %, largest fraction of the bound: uv {worst['uv']:.3f}, point {worst['point']:.3f}, normal {worst['normal']:.3f}")
    assert 0.0 < worst["uv"] <= 1.0 and 0.0 < worst["point"] <= 1.0 and 0.0 < worst["normal"] <= 1.0


def test_dilation_fills_from_the_previous_pass_only(built):
    """engine.dilate_texels against a numpy restatement: pass k sees what pass k - 1 left, fills with 1 + k, sums in the rule's order."""
    rng = np.random.default_rng(2)
    h, w = 9, 13
    fill = (rng.random((h, w)) < 0.12).astype(np.uint8)
    rgba = rng.uniform(0, 2, (h, w, 4)).astype(np.float32) * fill[..., None]
    for passes in (0, 1, 2, 3):
        got, gf = engine.dilate_texels(rgba, fill, passes)
        want, wf = rgba.copy(), fill.copy()
        for k in range(1, passes + 1):
            prev, pf = want.copy(), wf.copy()
            for y in range(h):
                for x in range(w):
                    if pf[y, x]:
                        continue
                    acc, count = np.zeros(3, np.float32), 0
                    for dy, dx in ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < h and 0 <= xx < w and pf[yy, xx]:
                            acc = (acc + prev[yy, xx, :3]).astype(np.float32)
                            count += 1
                    if count:
                        want[y, x, :3] = acc / np.float32(count)
                        want[y, x, 3] = 0.0
                        wf[y, x] = 1 + k
        assert np.array_equal(gf, wf) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), passes
    assert (wf == 4).any() and (wf == 2).any()
