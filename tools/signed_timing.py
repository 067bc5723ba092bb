#!/usr/bin/env python3
"""The signed point queries on two scenes of about 260 k triangles: the Sponza stand-in (mostly open: the side pass leaves early)
and a closed one, 16 tori of 16 384 triangles each in a 4 x 4 grid. On the same 128^3 grid of points over the scene's box, in device
buffers: rt_query_nearest, rt_query_nearest_signed, and k_nearest_side alone as the difference of the two within a run (the pass has
no entry point of its own). Timed with the host clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each,
interleaved; median and min. Per scene also the share of points per feature kind and the mean fan length, from
rt_nearest_side_features_host on a seeded sample of 1 in 64 of the device's own records (which must reproduce the device's sides), and the
seconds rt_upload_topology took. Recorded, not judged. With a third argument only that scene runs ("sponza" or "tori"): what a
kernel trace of one scene is taken from (rocprofv3 --kernel-trace --stats -- python tools/signed_timing.py 7 out.json tori gives
k_nearest_side's own time beside k_nearest_points').
usage: tools/signed_timing.py [runs] [out.json] [scene]   (default: 7, profiles/signed_timing.json, both)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_amd import _capi, devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "signed_timing.json")
only = sys.argv[3] if len(sys.argv) > 3 else ""
G = 128
REC = C.sizeof(_capi.RtNearest)


def torus(nu=128, nv=64, R=1.0, r=0.4):
    u, v = 2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv
    U, V = np.meshgrid(u, v, indexing="ij")
    P = np.stack([(R + r * np.cos(V)) * np.cos(U), (R + r * np.cos(V)) * np.sin(U), r * np.sin(V)], axis=-1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b, c, d = P[i, j], P[(i + 1) % nu, j], P[(i + 1) % nu, (j + 1) % nv], P[i, (j + 1) % nv]
    return np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([a, c, d], axis=2).reshape(-1, 3, 3)])


def tori_scene():
    s = engine.Scene()
    s.add_material(engine.default_material(albedo=(0.7, 0.7, 0.7)))
    tri = torus()
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    nrm = np.repeat(n[:, None, :], 3, axis=1).astype(np.float32)
    for k in range(16):
        s.add_mesh(f"torus{k}", tri, nrm, engine.placement(position=(3.0 * (k % 4) - 4.5, 3.0 * (k // 4) - 4.5, 0.3 * (k % 3)), rotation=(17.0 * k, 31.0 * k, 0.0)), 0)
    return s


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def measure(r, name, scene):
    r.upload_scene(scene)
    t = time.perf_counter()
    r.upload_topology(scene)
    topo_s = time.perf_counter() - t
    pos = scene.numpy()["triPoints"].view(np.float32).reshape(-1, 8)[:, :3]
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    if name != "sponza stand-in":                 # (the tori are placed: the box of their world corners)
        lo, hi = np.array([-6.0, -6.0, -1.5], np.float32), np.array([6.0, 6.0, 2.0], np.float32)
    axes = [np.linspace(lo[d], hi[d], G, dtype=np.float32) for d in range(3)]
    grid = np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3))
    n = len(grid)
    bufs = [devmem.DeviceBuffer(grid.nbytes), devmem.DeviceBuffer(n * REC), devmem.DeviceBuffer(n)]
    bufs[0].upload(grid)
    d_p, d_out, d_side = (b.ptr for b in bufs)
    passes = {"nearest": lambda: r.query_nearest(d_p, None, n=n, out=d_out),
              "signed": lambda: r.query_nearest_signed(d_p, None, n=n, out=d_out, side=d_side)}
    for fn in passes.values():
        timed(fn)
    ms = {k: [] for k in passes}
    for _ in range(runs):
        for k, fn in passes.items():
            ms[k].append(timed(fn))
    side_alone = [b - a for a, b in zip(ms["nearest"], ms["signed"])]
    raw, side = np.empty(n * REC, np.uint8), np.empty(n, np.int8)
    bufs[1].download(into=raw)
    bufs[2].download(into=side)
    pick = np.sort(np.random.default_rng(64).choice(n, n // 64, replace=False))
    recs = (_capi.RtNearest * len(pick)).from_buffer_copy(raw.reshape(n, REC)[pick].tobytes())
    host, feat, fan = engine.nearest_side_host(scene.arrays(), grid[pick], recs, features=True)
    assert np.array_equal(host, side[pick]), "rt_nearest_side_host does not reproduce the device's sides"
    topo = scene.topology()
    row = dict(scene=name, triangles=int(scene.counts()["triangles"]), objects=len(topo), points=n, runs=runs,
               signable_triangles=int(sum(t["signableTriangles"] for t in topo)), upload_topology_s=round(topo_s, 3),
               nearest_ms=round(statistics.median(ms["nearest"]), 3), nearest_ms_min=round(min(ms["nearest"]), 3),
               signed_ms=round(statistics.median(ms["signed"]), 3), signed_ms_min=round(min(ms["signed"]), 3),
               side_alone_ms=round(statistics.median(side_alone), 3), side_alone_ms_min=round(min(side_alone), 3),
               sides={str(v): round(float((side == v).mean()), 4) for v in (-1, 0, 1)},
               feature_share=dict(unsigned=round(float((feat == 255).mean()), 4), face=round(float((feat == 0).mean()), 4),
                                  vertex=round(float(((feat >= 1) & (feat <= 3)).mean()), 4), edge=round(float(((feat >= 4) & (feat <= 6)).mean()), 4)),
               mean_fan=round(float(fan[fan > 0].mean()), 2) if (fan > 0).any() else 0.0)
    for b in bufs:
        b.free()
    return row


r = engine.Renderer(0)
rows = []
if only in ("", "sponza"):
    rows.append(measure(r, "sponza stand-in", scenes.sponza(0)[0]))
if only in ("", "tori"):
    rows.append(measure(r, "16 tori, closed", tori_scene()))
r.close()
print(json.dumps(rows), flush=True)
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
print("wrote", out)
