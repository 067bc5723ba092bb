#!/usr/bin/env python3
"""The ray queries against the first-hit AOV pass over the same rays: the Sponza stand-in at 1920 x 1080 (scenes.sponza_camera).
rt_render_aovs is the existing closest-hit pass over the camera rays; rt_query_closest gets the very same rays (camInfo.pos, the
rayDir plane) as a batch in device memory, rt_query_occluded gets them without a limit and with tmax = 0.5 x that ray's dst, and
rt_render_ao runs 4 samples over the planes (radius 0.5). Everything reads and writes device buffers (no read-back) and is timed
with the host clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved; median and min.
In a checkout that has no ray queries the tool times rt_render_aovs alone: its output there is the baseline to quote.
usage: tools/query_timing.py [runs] [out.json] [baseline.json]   (default: 7, profiles/query_timing.json; baseline.json: this tool's
output from the parent commit, copied into the result as "parent")"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "query_timing.json")
baseline = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080
N = W * H

r = engine.Renderer(0)
have_queries = hasattr(r, "query_closest")
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


r.upload_scene(scenes.sponza(0)[0])
pc = scenes.sponza_camera(W, H)
ptrs = {k: device(N * 16) for k in engine.AOV_PLANES}
passes = {"aov": lambda: r.render_aovs(pc, W, H, out_ptrs=ptrs)}   # sync=True: rt_sync
kernels = {}
timed(passes["aov"])
kernels["aov"] = r.last_kernel()
if have_queries:
    planes = {k: np.empty((N, 4), np.float32) for k in ("rayDir", "normalDepth")}
    for k, a in planes.items():
        BUFS[ptrs[k]].download(into=a)
    dirs = np.ascontiguousarray(planes["rayDir"][:, :3])
    origins = np.ascontiguousarray(np.tile(np.array(list(pc.camInfo.pos), np.float32), (N, 1)))
    half = np.ascontiguousarray(planes["normalDepth"][:, 3] * np.float32(0.5))
    d_o, d_d, d_t = device(origins.nbytes, origins), device(dirs.nbytes, dirs), device(half.nbytes, half)
    d_hits, d_occ, d_ao = device(N * C.sizeof(_capi.RtHit)), device(N), device(N * 4)
    aov_planes = _capi.RtAovBuffers(**ptrs)
    ao_params = _capi.RtAoParams(4, 0.5, 0)

    def ao():
        r._check(r._l.rt_render_ao(r._h, N, C.byref(aov_planes), C.byref(ao_params), d_ao), "rt_render_ao")
        r.sync()

    passes.update(closest=lambda: r.query_closest(d_o, d_d, None, n=N, out=d_hits),
                  occluded=lambda: r.query_occluded(d_o, d_d, None, n=N, out=d_occ),
                  occluded_half=lambda: r.query_occluded(d_o, d_d, d_t, n=N, out=d_occ), ao4=ao)
    for k, fn in passes.items():
        if k != "aov":
            timed(fn)
            kernels[k] = r.last_kernel()
ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in", width=W, height=H, rays=N, runs=runs, queries=have_queries, kernels=kernels)
for k, v in ms.items():
    row[f"{k}_ms"] = round(statistics.median(v), 3)
    row[f"{k}_ms_min"] = round(min(v), 3)
if have_queries:
    occ = np.empty(N, np.uint8)
    passes["occluded"]()
    BUFS[d_occ].download(into=occ)
    row["hit_share"] = round(float(occ.mean()), 4)
if baseline:
    with open(baseline) as f:
        row["parent"] = json.load(f)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
