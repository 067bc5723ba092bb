#!/usr/bin/env python3
"""The radius point queries on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080): rt_query_within over the "offset" point
set of tools/nearest_timing.py (the 2 073 600 first-hit positions of the frame, pushed 0.05 along their normals) in device
buffers, with the reaches 0.1 and 0.4 and k = 0, 1 and 8, and rt_query_nearest beside it with the same limits in the same run.
Timed with the host clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved; median and
min. Members per point, the share of points with a member and with more than 8, and the box and triangle distances per point come
from one more pass of each. Recorded, not judged.
usage: tools/within_timing.py [runs] [out.json]   (default: 7, profiles/within_timing.json)"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "within_timing.json")
W, H = 1920, 1080
N = W * H
REACHES = (0.1, 0.4)
KS = (0, 1, 8)

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
planes = {k: np.empty((N, 4), np.float32) for k in ("position", "normalDepth")}
for k, a in planes.items():
    BUFS[ptrs[k]].download(into=a)
offset = np.ascontiguousarray(planes["position"][:, :3] + np.float32(0.05) * planes["normalDepth"][:, :3])
d_points = device(offset.nbytes, offset)
d_reach = {R: device(N * 4, np.full(N, R, np.float32)) for R in REACHES}
d_out, d_counts = device(N * max(KS) * C.sizeof(_capi.RtNearest)), device(N * 4)

passes = {}
for R in REACHES:
    for k in KS:
        passes[f"within_r{R}_k{k}"] = lambda R=R, k=k: r.query_within(d_points, d_reach[R], k, n=N, out=d_out if k else None, counts=d_counts)
    passes[f"nearest_r{R}"] = lambda R=R: r.query_nearest(d_points, d_reach[R], n=N, out=d_out)
kernels = {}
for k, fn in passes.items():
    timed(fn)
    kernels[k] = r.last_kernel()
ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in", triangles=int(scene.counts()["triangles"]), width=W, height=H, points=N, offset=0.05, runs=runs, kernels=kernels)
for k, v in ms.items():
    row[f"{k}_ms"] = round(statistics.median(v), 3)
    row[f"{k}_ms_min"] = round(min(v), 3)
counts = np.empty(N, np.uint32)
for R in REACHES:
    for name in (f"within_r{R}_k8", f"nearest_r{R}"):
        before = r.counters()
        passes[name]()
        after = r.counters()
        row[f"{name}_box_per_point"] = round((after["boxTests"] - before["boxTests"]) / N, 2)
        row[f"{name}_tri_per_point"] = round((after["triTests"] - before["triTests"]) / N, 2)
        row[f"{name}_found_share"] = round((after["raysHit"] - before["raysHit"]) / N, 4)
    passes[f"within_r{R}_k0"]()
    BUFS[d_counts].download(into=counts)
    row[f"within_r{R}_members_per_point"] = round(float(counts.mean()), 3)
    row[f"within_r{R}_max_members"] = int(counts.max())
    row[f"within_r{R}_share_above_8"] = round(float((counts > 8).mean()), 4)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
