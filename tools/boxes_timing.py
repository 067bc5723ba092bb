#!/usr/bin/env python3
"""The box queries on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080), in device buffers: rt_query_boxes over
 - a 128^3 grid over the scene's box (engine.grid_boxes: 2 097 152 cells) at k = 0 and k = 8, and
 - the 2 073 600 first-hit positions of the frame as the centres of cubes of half-extent 0.05 and 0.2, and of 1 : 4 : 16 boxes
   of the same volume (half-extents h / 4, h, 4 h along x, y, z), at k = 0 and k = 8,
with rt_query_within at each set's circumscribed radius (k = 0) beside it in the same run as the yardstick. Timed with the host
clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved; median and min. Box tests,
triangle tests and members per box come from one more pass of each. Recorded, not judged.
usage: tools/boxes_timing.py [runs] [out.json]   (default: 7, profiles/boxes_timing.json)"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "boxes_timing.json")
W, H = 1920, 1080
N = W * H
GRID = 128
HALVES = (0.05, 0.2)

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
position = np.empty((N, 4), np.float32)
BUFS[ptrs["position"]].download(into=position)
centre = np.ascontiguousarray(position[:, :3])
pts = scene.numpy()["triPoints"].view(np.float32).reshape(-1, 8)[:, :3]   # the mesh corners as stored
slo, shi = pts.min(axis=0), pts.max(axis=0)

sets = {}   # name -> (n, device lo, device hi, device centres or None, circumscribed radius or None)
glo, ghi = engine.grid_boxes(slo, shi, (GRID, GRID, GRID))
sets[f"grid{GRID}"] = (len(glo), device(glo.nbytes, glo), device(ghi.nbytes, ghi), None, None)
d_centre = device(centre.nbytes, centre)
for h in HALVES:
    for name, half in ((f"cube_h{h}", np.array([h, h, h], np.float32)), (f"slab_h{h}", np.array([h / 4, h, 4 * h], np.float32))):
        lo, hi = np.ascontiguousarray(centre - half), np.ascontiguousarray(centre + half)
        sets[name] = (N, device(lo.nbytes, lo), device(hi.nbytes, hi), d_centre, float(np.linalg.norm(half.astype(np.float64))))
most = max(n for n, *_ in sets.values())
d_out, d_counts = device(most * 8 * C.sizeof(_capi.RtOverlap)), device(most * 4)
d_reach = {name: device(N * 4, np.full(N, R, np.float32)) for name, (_, _, _, c, R) in sets.items() if c is not None}

passes = {}
for name, (n, lo, hi, c, R) in sets.items():
    for k in (0, 8):
        passes[f"boxes_{name}_k{k}"] = lambda n=n, lo=lo, hi=hi, k=k: r.query_boxes(lo, hi, k, n=n, out=d_out if k else None, counts=d_counts)
    if c is not None:
        passes[f"within_{name}_k0"] = lambda name=name, c=c: r.query_within(c, d_reach[name], 0, n=N, counts=d_counts)
kernels = {}
for k, fn in passes.items():
    timed(fn)
    kernels[k] = r.last_kernel()
ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in", triangles=int(scene.counts()["triangles"]), width=W, height=H, grid=GRID, runs=runs, kernels=kernels,
           boxes={name: n for name, (n, *_) in sets.items()}, radius={name: R for name, (_, _, _, _, R) in sets.items() if R is not None})
for k, v in ms.items():
    row[f"{k}_ms"] = round(statistics.median(v), 3)
    row[f"{k}_ms_min"] = round(min(v), 3)
for name, (n, *_rest) in sets.items():
    for pass_name in [f"boxes_{name}_k0"] + ([f"within_{name}_k0"] if f"within_{name}_k0" in passes else []):
        before = r.counters()
        passes[pass_name]()
        after = r.counters()
        counts = np.empty(n, np.uint32)
        BUFS[d_counts].download(into=counts)
        row[f"{pass_name}_box_tests_per_box"] = round((after["boxTests"] - before["boxTests"]) / n, 2)
        row[f"{pass_name}_tri_tests_per_box"] = round((after["triTests"] - before["triTests"]) / n, 2)
        row[f"{pass_name}_members_per_box"] = round(float(counts.mean()), 3)
        row[f"{pass_name}_max_members"] = int(counts.max())
        row[f"{pass_name}_share_above_8"] = round(float((counts > 8).mean()), 4)
        row[f"{pass_name}_share_occupied"] = round(float((counts > 0).mean()), 4)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
