#!/usr/bin/env python3
"""rt_query_radiance against rt_render over the same rays: the bench scene (the Sponza stand-in through scenes.sponza_camera) at
1920 x 1080, 8 samples, bounce limit 8. rt_render runs with "pipeline" 0, so both run the same traversal and the same shading code
on the same build; the query gets the frame's 2.07 M camera rays (camInfo.pos, the rayDir plane of rt_render_aovs) as a batch in
device memory, once in row-major order without ids ("rows": slot i is pixel i) and once in rt_render's own slot order with the
pixel indices as ids ("tiled": slot i is the pixel rt_render puts there, 8 x 8 blocks), which separates what the slot order costs
from what the entry point costs. Everything reads and writes device buffers (no read-back) and is timed with the host clock around
the enqueue and an rt_sync; two warm-ups of each, then `runs` of each, interleaved; median, min, max and the ratio of the medians.
The three images are compared bit for bit before anything is timed.
usage: tools/radiance_timing.py [runs] [out.json]   (default: 9, profiles/radiance_timing.json)"""
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py: the parts of a dispatch overlap on hardware queues of their own

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_amd import devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "radiance_timing.json")
W, H, SAMPLES, BOUNCES = 1920, 1080, 8, 8
N = W * H

r = engine.Renderer(0)
BUFS = {}   # device address -> the devmem.DeviceBuffer that owns it


def device(nbytes, host=None):
    b = devmem.DeviceBuffer(nbytes)
    if host is not None:
        b.upload(host)
    BUFS[b.ptr] = b
    return b.ptr


def host(ptr, shape, dtype=np.float32):
    a = np.empty(shape, dtype)
    BUFS[ptr].download(into=a)
    return a


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


r.upload_scene(scenes.CONFIGS["sponza"]()[0])
r.set_tuning("pipeline", 0)
pc = scenes.sponza_camera(W, H, singleRender=1, sampleLimit=SAMPLES, bounceLimit=BOUNCES, progressive=0)
d_dir = device(N * 16)
r.render_aovs(pc, W, H, out_ptrs=dict(rayDir=d_dir))
dirs = np.ascontiguousarray(host(d_dir, (N, 4))[:, :3])
origins = np.ascontiguousarray(np.tile(np.array(list(pc.camInfo.pos), np.float32), (N, 1)))
# rt_render's slot order (k_raygen: slot_to_pixel): 64 slots per 8 x 8 pixel block, the blocks in row-major order
assert W % 8 == 0 and H % 8 == 0
slot = np.arange(N, dtype=np.int64)
tile, within = slot >> 6, slot & 63
pixel = (((tile // (W // 8)) * 8 + (within >> 3)) * W + (tile % (W // 8)) * 8 + (within & 7)).astype(np.uint32)
assert np.array_equal(np.sort(pixel), np.arange(N, dtype=np.uint32))
d_o = device(origins.nbytes, origins)
d_rows, d_tiled, d_ids = device(dirs.nbytes, dirs), device(dirs.nbytes, np.ascontiguousarray(dirs[pixel])), device(pixel.nbytes, pixel)
d_img, d_out_rows, d_out_tiled = device(N * 16), device(N * 16), device(N * 16)
env = pc.environment

passes = {
    "render": lambda: r.render(pc, W, H, out_ptr=d_img),   # sync=True: rt_sync
    "query_rows": lambda: r.query_radiance(d_o, d_rows, samples=SAMPLES, bounces=BOUNCES, environment=env, n=N, out=d_out_rows),
    "query_tiled": lambda: r.query_radiance(d_o, d_tiled, samples=SAMPLES, bounces=BOUNCES, ids=d_ids, environment=env, n=N, out=d_out_tiled),
}
kernels, parts = {}, {}
for k, fn in passes.items():
    timed(fn)
    timed(fn)
    kernels[k] = r.last_kernel()
parts["render"] = r.last_parts()
assert r.last_pipeline() == 0
img = host(d_img, (N, 4)).view(np.uint32)
same_rows = bool(np.array_equal(host(d_out_rows, (N, 4)).view(np.uint32), img))
same_tiled = bool(np.array_equal(host(d_out_tiled, (N, 4)).view(np.uint32), img[pixel]))
assert same_rows and same_tiled, (same_rows, same_tiled)

ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
row = dict(scene="sponza stand-in (the bench scene)", width=W, height=H, rays=N, samples=SAMPLES, bounceLimit=BOUNCES, runs=runs, kernels=kernels,
           render_parts=parts["render"], bit_identical=dict(rows=same_rows, tiled=same_tiled))
for k, v in ms.items():
    row[f"{k}_ms"] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
row["query_rows_over_render"] = round(statistics.median(ms["query_rows"]) / statistics.median(ms["render"]), 4)
row["query_tiled_over_render"] = round(statistics.median(ms["query_tiled"]) / statistics.median(ms["render"]), 4)
row["render_spread"] = round((max(ms["render"]) - min(ms["render"])) / statistics.median(ms["render"]), 4)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
