#!/usr/bin/env python3
"""The oriented box queries on the Sponza stand-in (scenes.sponza_camera at 1920 x 1080), in device buffers, k = 0, each beside
its yardstick in the same run:
 1. the 2 073 600 cubes of half-extent 0.05 about the first-hit positions of the frame under identity frames (one a box, and one
    shared), against rt_query_boxes over the same boxes: the answers are the same, the difference is the price of the frame step;
 2. 1 : 4 : 16 boxes of the half-extent-0.2 volume (half-extents 0.05, 0.2, 0.8) about the same centres, turned by seeded
    rotations, against rt_query_boxes over each turned box's world bounding box: what a caller does without this query;
 3. a 128^3 grid in a frame turned 30 degrees about the vertical through the middle of the scene's box (one shared frame),
    against the axis-aligned 128^3 grid over that box.
Timed with the host clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved; median, min
and max (the run-to-run spread). Box tests, triangle-rule calls and members per box come from one more pass of each. Recorded,
not judged.
usage: tools/obbs_timing.py [runs] [out.json]   (default: 5, profiles/obbs_timing.json)"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_amd import devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "obbs_timing.json")
W, H = 1920, 1080
N = W * H
GRID = 128
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)

r = engine.Renderer(0)
BUFS = {}   # device address -> the devmem.DeviceBuffer that owns it


def device(nbytes, host=None):
    b = devmem.DeviceBuffer(nbytes)
    if host is not None:
        b.upload(np.ascontiguousarray(host))
    BUFS[b.ptr] = b
    return b.ptr


class Frames:
    """Device frames as Renderer.query_oriented_boxes takes a tensor: data_ptr() and numel() (16: one shared frame)."""

    def __init__(self, host):
        host = np.ascontiguousarray(host, np.float32)
        self.ptr, self.n = device(host.nbytes, host), host.size

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n


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
centre = np.ascontiguousarray(position[:, :3])
pts = scene.numpy()["triPoints"].view(np.float32).reshape(-1, 8)[:, :3]   # the mesh corners as stored
slo, shi = pts.min(axis=0), pts.max(axis=0)
d_counts = device(max(N, GRID ** 3) * 4)

passes, boxes = {}, {}   # name -> the pass; name -> boxes of it


def add(name, n, frames, lo, hi):
    """frames: None for rt_query_boxes, else a Frames."""
    dl, dh = device(lo.nbytes, lo), device(hi.nbytes, hi)
    boxes[name] = n
    if frames is None:
        passes[name] = lambda: r.query_boxes(dl, dh, 0, n=n, counts=d_counts)
    else:
        passes[name] = lambda: r.query_oriented_boxes(frames, dl, dh, 0, n=n, counts=d_counts)


# 1. cubes under identity frames
half = np.float32([0.05, 0.05, 0.05])
clo, chi = centre - half, centre + half
add("cubes_boxes", N, None, clo, chi)
add("cubes_identity_frames", N, Frames(np.tile(IDENTITY, (N, 1))), clo, chi)
add("cubes_shared_identity", N, Frames(IDENTITY), clo, chi)
# 2. thin boxes turned by seeded rotations, and their world bounding boxes
thin = np.array([0.05, 0.2, 0.8])
R = rotations(np.random.default_rng(2024), N)
add("thin_turned", N, Frames(engine.obb_frames(centre, R)), np.tile(-thin.astype(np.float32), (N, 1)), np.tile(thin.astype(np.float32), (N, 1)))
world = np.abs(R) @ thin                                               # the half-extents of the turned box's world box
add("thin_world_boxes", N, None, (centre - world).astype(np.float32), (centre + world).astype(np.float32))
# 3. the grid, axis-aligned and in a frame turned 30 degrees about the vertical
glo, ghi = engine.grid_boxes(slo, shi, (GRID, GRID, GRID))
add("grid_boxes", GRID ** 3, None, glo, ghi)
a = np.radians(30.0)
turn = np.array([[[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]])
mid, ext = (slo.astype(np.float64) + shi) / 2, (shi.astype(np.float64) - slo) / 2
tlo, thi = engine.grid_boxes(-ext, ext, (GRID, GRID, GRID))
add("grid_turned", GRID ** 3, Frames(engine.obb_frames(mid[None], turn)[0]), tlo, thi)

kernels = {}
for k, fn in passes.items():
    timed(fn)
    kernels[k] = r.last_kernel()
ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in", triangles=int(scene.counts()["triangles"]), width=W, height=H, grid=GRID, runs=runs, kernels=kernels, boxes=boxes)
for k, v in ms.items():
    row[f"{k}_ms"] = round(statistics.median(v), 3)
    row[f"{k}_ms_min"] = round(min(v), 3)
    row[f"{k}_ms_max"] = round(max(v), 3)
answers = {}
for name, n in boxes.items():
    before = r.counters()
    passes[name]()
    after = r.counters()
    counts = np.empty(n, np.uint32)
    BUFS[d_counts].download(into=counts)
    answers[name] = counts
    row[f"{name}_box_tests_per_box"] = round((after["boxTests"] - before["boxTests"]) / n, 2)
    row[f"{name}_tri_tests_per_box"] = round((after["triTests"] - before["triTests"]) / n, 2)
    row[f"{name}_members_per_box"] = round(float(counts.mean()), 3)
    row[f"{name}_max_members"] = int(counts.max())
    row[f"{name}_share_occupied"] = round(float((counts > 0).mean()), 4)
row["cubes_counts_equal"] = bool(np.array_equal(answers["cubes_boxes"], answers["cubes_identity_frames"]) and np.array_equal(answers["cubes_boxes"], answers["cubes_shared_identity"]))
row["cubes_frame_step_ms"] = round(row["cubes_identity_frames_ms"] - row["cubes_boxes_ms"], 3)
row["cubes_boxes_spread_ms"] = round(row["cubes_boxes_ms_max"] - row["cubes_boxes_ms_min"], 3)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
