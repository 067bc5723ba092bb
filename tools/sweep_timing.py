#!/usr/bin/env python3
"""The sphere sweeps on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080): rt_query_sweep over the 2 073 600 camera rays
of the frame (camInfo.pos, the rayDir plane of rt_render_aovs) in device buffers, with the radii 0.01 and 0.1, and rt_query_closest
over the very same rays beside it in the same run. Timed with the host clock around the enqueue and an rt_sync; one warm-up of
each, then `runs` of each, interleaved; median and min. The grown boxes and the rule calls per ray, the share of rays found and of
rays that start in contact, and the ray query's own box and triangle tests per ray come from one more pass of each. Recorded, not
judged.
usage: tools/sweep_timing.py [runs] [out.json]   (default: 7, profiles/sweep_timing.json)"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sweep_timing.json")
W, H = 1920, 1080
N = W * H
RADII = (0.01, 0.1)

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
plane = np.empty((N, 4), np.float32)
BUFS[ptrs["rayDir"]].download(into=plane)
dirs = np.ascontiguousarray(plane[:, :3])
origins = np.ascontiguousarray(np.tile(np.array(list(pc.camInfo.pos), np.float32), (N, 1)))
d_o, d_d = device(origins.nbytes, origins), device(dirs.nbytes, dirs)
d_radius = {R: device(N * 4, np.full(N, R, np.float32)) for R in RADII}
d_out = device(N * C.sizeof(_capi.RtSweep))
d_hits = device(N * C.sizeof(_capi.RtHit))

passes = {f"sweep_r{R}": (lambda R=R: r.query_sweep(d_o, d_d, d_radius[R], n=N, out=d_out)) for R in RADII}
passes["closest"] = lambda: r.query_closest(d_o, d_d, n=N, out=d_hits)
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
for R in RADII:
    row[f"sweep_r{R}_over_closest"] = round(row[f"sweep_r{R}_ms"] / row["closest_ms"], 2)
recs = (_capi.RtSweep * N)()
for k, fn in passes.items():
    before = r.counters()
    fn()
    after = r.counters()
    row[f"{k}_box_per_ray"] = round((after["boxTests"] - before["boxTests"]) / N, 2)
    row[f"{k}_tri_per_ray"] = round((after["triTests"] - before["triTests"]) / N, 2)
    row[f"{k}_found_share"] = round((after["raysHit"] - before["raysHit"]) / N, 4)
    if k.startswith("sweep"):
        BUFS[d_out].download(into=np.frombuffer(recs, np.uint8))
        row[f"{k}_starts_in_contact_share"] = round(float(engine.sweep_to_numpy(recs)["startsInContact"].mean()), 4)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
