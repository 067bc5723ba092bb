#!/usr/bin/env python3
"""The point queries on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080): rt_query_nearest over two point sets in device
buffers, and rt_query_closest over the same number of rays in the same run as context. Set "offset": the 2 073 600 first-hit
positions of the frame (rt_render_aovs), pushed 0.05 along their normals (pixels that hit nothing keep the position plane's
record). Set "grid": a 128^3 grid over the box of the scene's points. Timed with the host clock around the enqueue and an rt_sync;
one warm-up of each, then `runs` of each, interleaved; median and min. Box and triangle evaluations per point come from the
counters around one more pass. Recorded, not judged.
usage: tools/nearest_timing.py [runs] [out.json]   (default: 7, profiles/nearest_timing.json)"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "nearest_timing.json")
W, H = 1920, 1080
N = W * H
G = 128

r = engine.Renderer(0)
BUFS = {}   # device address -> the devmem.DeviceBuffer that owns it


def device(nbytes, host=None):
    b = devmem.DeviceBuffer(nbytes)
    if host is not None:
        b.upload(host)
    BUFS[b.ptr] = b
    return b.ptr


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


scene = scenes.sponza(0)[0]
r.upload_scene(scene)
pc = scenes.sponza_camera(W, H)
ptrs = {k: device(N * 16) for k in engine.AOV_PLANES}
r.render_aovs(pc, W, H, out_ptrs=ptrs)
planes = {k: np.empty((N, 4), np.float32) for k in ("position", "normalDepth", "rayDir")}
for k, a in planes.items():
    BUFS[ptrs[k]].download(into=a)
offset = np.ascontiguousarray(planes["position"][:, :3] + np.float32(0.05) * planes["normalDepth"][:, :3])
pos = scene.numpy()["triPoints"].view(np.float32).reshape(-1, 8)[:, :3]
lo, hi = pos.min(axis=0), pos.max(axis=0)
axes = [np.linspace(lo[d], hi[d], G, dtype=np.float32) for d in range(3)]
grid = np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3))
assert len(grid) == G ** 3 and len(offset) == N
dirs = np.ascontiguousarray(planes["rayDir"][:, :3])
origins = np.ascontiguousarray(np.tile(np.array(list(pc.camInfo.pos), np.float32), (N, 1)))

d_sets = {"offset": (device(offset.nbytes, offset), len(offset)), "grid": (device(grid.nbytes, grid), len(grid))}
d_near = device(max(N, G ** 3) * C.sizeof(_capi.RtNearest))
d_o, d_d, d_hits = device(origins.nbytes, origins), device(dirs.nbytes, dirs), device(N * C.sizeof(_capi.RtHit))
passes = {f"nearest_{k}": (lambda p=p, n=n: r.query_nearest(p, None, n=n, out=d_near)) for k, (p, n) in d_sets.items()}
passes["closest"] = lambda: r.query_closest(d_o, d_d, None, n=N, out=d_hits)
kernels = {}
for k, fn in passes.items():
    timed(fn)
    kernels[k] = r.last_kernel()
ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in", triangles=int(scene.counts()["triangles"]), width=W, height=H, runs=runs, kernels=kernels,
           points={k: n for k, (_, n) in d_sets.items()}, rays=N)
for k, v in ms.items():
    row[f"{k}_ms"] = round(statistics.median(v), 3)
    row[f"{k}_ms_min"] = round(min(v), 3)
for k in d_sets:
    before = r.counters()
    passes[f"nearest_{k}"]()
    after = r.counters()
    n = d_sets[k][1]
    row[f"nearest_{k}_box_per_point"] = round((after["boxTests"] - before["boxTests"]) / n, 2)
    row[f"nearest_{k}_tri_per_point"] = round((after["triTests"] - before["triTests"]) / n, 2)
    row[f"nearest_{k}_found_share"] = round((after["raysHit"] - before["raysHit"]) / n, 4)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
