#!/usr/bin/env python3
"""The cut queries on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080), in device buffers, k = 0 and 8, on the two
workloads of tools/triangles_timing.py, each beside its yardstick in the same run:
 (i)  2 073 600 small triangles with edges of about 0.1, turned by seeded rotations about the first-hit positions of the frame;
 (ii) as many slivers of about 0.05 x 0.8, turned the same way.
For each: rt_query_cuts and rt_query_triangles over the same batch (the same descent; the cut query adds steps 2 to 5 of its rule
on the pairs that touch, and the 48-byte records). Timed with the host clock around the enqueue and an rt_sync; one warm-up of
each, then `runs` of each, interleaved; median, min and max (the run-to-run spread). Nodes tested, rule calls and cuts or members
per query come from one more pass of each. Recorded, not judged.
usage: tools/cuts_timing.py [runs] [out.json]   (default: 7, profiles/cuts_timing.json)"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_amd import devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "cuts_timing.json")
W, H = 1920, 1080
N = W * H
KS = (0, 8)

r = engine.Renderer(0)
BUFS = {}   # device address -> the devmem.DeviceBuffer that owns it


def device(nbytes, host=None):
    b = devmem.DeviceBuffer(nbytes)
    if host is not None:
        b.upload(np.ascontiguousarray(host))
    BUFS[b.ptr] = b
    return b.ptr


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


scene = scenes.sponza(0)[0]
r.upload_scene(scene)
pc = scenes.sponza_camera(W, H)
ptrs = {k: device(N * 16) for k in engine.AOV_PLANES}
r.render_aovs(pc, W, H, out_ptrs=ptrs)
position = np.empty((N, 4), np.float32)
BUFS[ptrs["position"]].download(into=position)
centre = position[:, :3].astype(np.float64)
d_counts = device(N * 4)
d_out = device(N * 8 * 48)   # the cut records; the triangle query's 16-byte ones fit in it

R = rotations(np.random.default_rng(2025), N)
SHAPES = {"small": 0.1 / np.sqrt(3.0) * np.array([[1.0, 0.0, 0.0], [-0.5, np.sqrt(0.75), 0.0], [-0.5, -np.sqrt(0.75), 0.0]]),   # edges 0.1
          "sliver": np.array([[0.4, 0.0, 0.0], [-0.4, 0.025, 0.0], [-0.4, -0.025, 0.0]])}                                      # 0.05 x 0.8

passes = {}
for shape, base in SHAPES.items():
    corners = (centre[:, None, :] + np.einsum("nij,kj->nki", R, base)).astype(np.float32)
    d_corners = device(corners.nbytes, corners)
    for k in KS:
        o = d_out if k else None
        passes[f"{shape}_k{k}_cuts"] = (lambda c=d_corners, k=k, o=o: r.query_cuts(c, k, n=N, out=o, counts=d_counts))
        passes[f"{shape}_k{k}_triangles"] = (lambda c=d_corners, k=k, o=o: r.query_triangles(c, k, n=N, out=o, counts=d_counts))
    del corners

kernels = {}
for name, fn in passes.items():
    timed(fn)
    kernels[name] = r.last_kernel()
ms = {name: [] for name in passes}
for _ in range(runs):
    for name, fn in passes.items():
        ms[name].append(timed(fn))
row = dict(scene="sponza stand-in", triangles=int(scene.counts()["triangles"]), width=W, height=H, queries=N, runs=runs, kernels=kernels)
for name, v in ms.items():
    row[f"{name}_ms"] = round(statistics.median(v), 3)
    row[f"{name}_ms_min"] = round(min(v), 3)
    row[f"{name}_ms_max"] = round(max(v), 3)
answers = {}
for name, fn in passes.items():
    r.sync()
    before = r.counters()
    fn()
    after = r.counters()
    counts = np.empty(N, np.uint32)
    BUFS[d_counts].download(into=counts)
    answers[name] = counts
    row[f"{name}_box_tests_per_query"] = round((after["boxTests"] - before["boxTests"]) / N, 2)
    row[f"{name}_tri_tests_per_query"] = round((after["triTests"] - before["triTests"]) / N, 2)
    row[f"{name}_per_query"] = round(float(counts.mean()), 3)      # cuts, or members of the triangle query
    row[f"{name}_max"] = int(counts.max())
    row[f"{name}_share_with_any"] = round(float((counts > 0).mean()), 4)
for shape in SHAPES:
    for k in KS:
        row[f"{shape}_k{k}_cuts_never_exceed_members"] = bool((answers[f"{shape}_k{k}_cuts"] <= answers[f"{shape}_k{k}_triangles"]).all())
        row[f"{shape}_k{k}_same_descent"] = bool(row[f"{shape}_k{k}_cuts_box_tests_per_query"] == row[f"{shape}_k{k}_triangles_box_tests_per_query"] and row[f"{shape}_k{k}_cuts_tri_tests_per_query"] == row[f"{shape}_k{k}_triangles_tri_tests_per_query"])
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
