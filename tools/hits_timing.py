#!/usr/bin/env python3
"""The all-hit ray queries on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080): rt_query_hits with k = 0, 1, 4 and 8 over
the 2 073 600 camera rays of the frame (camInfo.pos, the rayDir plane of rt_render_aovs) in device buffers, and rt_query_closest
over the same rays in the same run as context. No limit. Timed with the host clock around the enqueue and an rt_sync; one warm-up
of each, then `runs` of each, interleaved; median and min. The mean count per ray, the share of rays with a crossing and with more
than 8, and the box and triangle tests per ray come from one more pass. Recorded, not judged.
usage: tools/hits_timing.py [runs] [out.json]   (default: 7, profiles/hits_timing.json)"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "hits_timing.json")
W, H = 1920, 1080
N = W * H
KS = (0, 1, 4, 8)

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
ray_dir = np.empty((N, 4), np.float32)
BUFS[ptrs["rayDir"]].download(into=ray_dir)
dirs = np.ascontiguousarray(ray_dir[:, :3])
origins = np.ascontiguousarray(np.tile(np.array(list(pc.camInfo.pos), np.float32), (N, 1)))
d_o, d_d = device(origins.nbytes, origins), device(dirs.nbytes, dirs)
d_hits, d_counts = device(N * max(KS) * C.sizeof(_capi.RtHit)), device(N * 4)
passes = {f"hits_k{k}": (lambda k=k: r.query_hits(d_o, d_d, k, None, n=N, out=d_hits if k else None, counts=d_counts)) for k in KS}
passes["closest"] = lambda: r.query_closest(d_o, d_d, None, n=N, out=d_hits)
kernels = {}
for k, fn in passes.items():
    timed(fn)
    kernels[k] = r.last_kernel()
ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in", triangles=int(scene.counts()["triangles"]), width=W, height=H, rays=N, runs=runs, kernels=kernels)
for k, v in ms.items():
    row[f"{k}_ms"] = round(statistics.median(v), 3)
    row[f"{k}_ms_min"] = round(min(v), 3)
before = r.counters()
passes["hits_k8"]()
after = r.counters()
counts = np.empty(N, np.uint32)
BUFS[d_counts].download(into=counts)
row["mean_count"] = round(float(counts.mean()), 3)
row["max_count"] = int(counts.max())
row["share_with_a_crossing"] = round(float((counts > 0).mean()), 4)
row["share_above_8"] = round(float((counts > 8).mean()), 4)
row["box_per_ray"] = round((after["boxTests"] - before["boxTests"]) / N, 2)
row["tri_per_ray"] = round((after["triTests"] - before["triTests"]) / N, 2)
before = r.counters()
passes["closest"]()
after = r.counters()
row["closest_box_per_ray"] = round((after["boxTests"] - before["boxTests"]) / N, 2)
row["closest_tri_per_ray"] = round((after["triTests"] - before["triTests"]) / N, 2)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
