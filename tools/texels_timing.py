#!/usr/bin/env python3
"""What the lightmap texel passes cost ("Lightmap texels"). rt_bake_texels at 1024^2, 2048^2 and 4096^2 texels over
  (a) quad: one quad over the whole uv square, two triangles of 2^14 .. 2^18 work items each;
  (b) grid: the same square as a 256 x 256 grid of quads, 131 072 triangles of one to a few work items each;
  (c) sponza: the largest object (by triangles) of the Sponza stand-in under a per-triangle atlas (sponza() below);
beside each a hipMemsetAsync of the 48-byte record plane in the same run, as the floor: the bake writes that plane once. (a)
against (b) is the measurement that shows whether the (triangle, block) work distribution does its job: the same texels, from two
triangles or from 131 072. Then rt_bake_lightmap at 256^2 with 64 samples and 8 bounces over the Sponza object against
rt_query_irradiance over the same compacted batch in the same run: the difference is what the four small passes and the one wait
add. Everything writes device buffers (no read-back) and is timed with the host clock around the enqueue and a device synchronise; two
warm-ups of each, then `runs` of each, interleaved; median, min, max.
usage: tools/texels_timing.py [runs] [out.json]   (default: 9, profiles/texels_timing.json)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_amd import _capi, devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "texels_timing.json")
SIZES = (1024, 2048, 4096)
LM, S, BOUNCES = 256, 64, 8

r = engine.Renderer(0)
hip = devmem.hip()
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]


def timed(fn):
    t = time.perf_counter()
    fn()
    devmem.synchronize()   # (the memset runs on the null stream)
    return (time.perf_counter() - t) * 1e3


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def flat_mesh(cells):
    k = np.arange(cells + 1, dtype=np.float64) / cells
    u, v = np.meshgrid(k, k, indexing="ij")
    vert = np.stack([u, v], -1).astype(np.float32)
    a, b, c, d = vert[:-1, :-1], vert[1:, :-1], vert[1:, 1:], vert[:-1, 1:]
    uv = np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 2), np.stack([a, c, d], 2).reshape(-1, 3, 2)])
    pos = np.stack([2 * uv[..., 0] - 1, np.zeros(uv.shape[:2], np.float32), 2 * uv[..., 1] - 1], -1).astype(np.float32)
    nrm = np.zeros_like(pos)
    nrm[..., 1] = -1.0
    s = engine.Scene()
    s.add_material(engine.default_material())
    s.add_mesh(f"grid{cells}", pos, nrm, engine.placement(rotation=(20, 35, -10), scale=(1.5, 0.7, 2.0)), 0, uvs=uv)
    return s, 0, len(uv)


def sponza():
    """The Sponza stand-in, whose meshes carry no uv layout (every uv is 0: every triangle would be skipped): its largest object gets
    the simplest atlas there is, two triangles to each cell of a square grid with a margin of a tenth of a cell around each,
    written into the host scene's points (Scene.update_points) before the upload. Unwrapping is not the library's business; the
    bake only needs some layout with as many triangles as a real one."""
    s = scenes.CONFIGS["sponza"]()[0]
    a = s.arrays()
    best, lo, hi = 0, 0, 0
    for i in range(a.objectCount):
        nodes, first, last = [a.objects[i].bvhIndex], 1 << 40, 0
        while nodes:
            b = a.bvhNodes[nodes.pop()]
            if b.triCount:
                first, last = min(first, b.index), max(last, b.index + b.triCount)
            else:
                nodes += [b.index, b.index + 1]
        if last - first > hi - lo:
            best, lo, hi = i, first, last
    raw = s.numpy()
    pts = raw["triPoints"].view(np.float32).reshape(-1, 8).copy()
    tri = raw["triangles"].view(np.uint32).reshape(-1, 12)[lo:hi, :3].astype(np.int64)
    n = hi - lo
    G = int(np.ceil(np.sqrt((n + 1) // 2)))
    k = np.arange(n)
    cx, cy, upper, m = (k // 2) % G, (k // 2) // G, (k % 2).astype(bool), 0.1
    corner = np.where(upper[:, None, None], np.array([(1 - m, 1 - m), (2 * m, 1 - m), (1 - m, 2 * m)]), np.array([(m, m), (1 - 2 * m, m), (m, 1 - 2 * m)]))
    uv = ((np.stack([cx, cy], -1)[:, None, :] + corner) / G).astype(np.float32)
    pts[tri, 3], pts[tri, 7] = uv[..., 0], uv[..., 1]
    first, last = int(tri.min()), int(tri.max()) + 1
    s.update_points(pts[first:last], first)
    return s, best, n


row = dict(runs=runs, bake={}, note="ms, host clock around the enqueue and a device synchronise")
cases = (("quad", lambda: flat_mesh(1)), ("grid", lambda: flat_mesh(256)), ("sponza", sponza))
with devmem.DeviceBuffer(48 * SIZES[-1] ** 2, "records") as recs:
    for name, make in cases:
        scene, obj, tris = make()
        r.upload_scene(scene)
        row["bake"][name] = dict(object=obj, triangles=tris)
        for size in SIZES:
            bake = lambda: r.bake_texels(obj, size, size, out=recs.ptr, stats=False, sync=False)   # noqa: E731
            floor = lambda: hip.hipMemsetAsync(recs.ptr, 0, 48 * size * size, None)              # noqa: E731
            for _ in range(2):
                timed(bake)
                timed(floor)
            st = r.bake_texels(obj, size, size, out=recs.ptr)
            ms = dict(bake=[], memset=[])
            for _ in range(runs):
                ms["bake"].append(timed(bake))
                ms["memset"].append(timed(floor))
            row["bake"][name][str(size)] = dict(stats=st, bake_ms=stats(ms["bake"]), memset_ms=stats(ms["memset"]),
                                                 bake_over_memset=round(statistics.median(ms["bake"]) / statistics.median(ms["memset"]), 2))
            print(name, size, row["bake"][name][str(size)], flush=True)
for size in SIZES:
    qa, gb = row["bake"]["quad"][str(size)]["bake_ms"]["median"], row["bake"]["grid"][str(size)]["bake_ms"]["median"]
    row["bake"].setdefault("quad_over_grid", {})[str(size)] = round(qa / gb, 3)

# the composite against the irradiance query over the same compacted batch (the scene is still the Sponza stand-in)
n = LM * LM
p = _capi.RtIrradianceParams(S, BOUNCES, 0, 0, 1e-5)
env = scenes.sponza_camera(64, 64).environment
with devmem.DeviceBuffer(48 * n) as dt, devmem.DeviceBuffer(12 * n) as dp, devmem.DeviceBuffer(12 * n) as dn, devmem.DeviceBuffer(4 * n) as di, \
        devmem.DeviceBuffer(4) as dc, devmem.DeviceBuffer(16 * n) as dv, devmem.DeviceBuffer(16 * n) as drgba, devmem.DeviceBuffer(n) as dfill:
    st = r.bake_texels(obj, LM, LM, out=dt.ptr)
    r.texels_compact(dt.ptr, n, dp.ptr, dn.ptr, di.ptr, dc.ptr)
    k = int(dc.download((1,), np.uint32)[0])
    lightmap = lambda: r.bake_lightmap(obj, LM, LM, params=p, env=env, dilate=2, out=drgba.ptr, fill=dfill.ptr, sync=False)   # noqa: E731
    query = lambda: r.query_irradiance(dp.ptr, dn.ptr, samples=S, bounces=BOUNCES, ids=di.ptr, environment=env, n=k, out=dv.ptr, sync=False)   # noqa: E731
    for _ in range(2):
        timed(lightmap)
        timed(query)
    ms = dict(lightmap=[], query=[])
    for _ in range(runs):
        ms["lightmap"].append(timed(lightmap))
        ms["query"].append(timed(query))
    added = statistics.median(ms["lightmap"]) - statistics.median(ms["query"])
    row["lightmap"] = dict(scene="sponza stand-in", object=obj, size=LM, samples=S, bounceLimit=BOUNCES, dilate=2, stats=st, covered=k, rays=k * S,
                           bake_lightmap_ms=stats(ms["lightmap"]), query_irradiance_ms=stats(ms["query"]), added_ms=round(added, 3),
                           added_share=round(added / statistics.median(ms["query"]), 4),
                           query_spread=round((max(ms["query"]) - min(ms["query"])) / statistics.median(ms["query"]), 4))
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
