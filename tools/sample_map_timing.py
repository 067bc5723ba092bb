#!/usr/bin/env python3
"""What a per-pixel sample count costs and saves, on the bench frame (the Sponza stand-in at 1920 x 1080, 8 spp, progressive, one
frame per dispatch) in both pipelines, and rt_build_sample_map at the same size. The method is the other *_timing.py tools': device
buffers, no read-back, the host clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved;
median and min.
  (a) rt_render_sampled with a map that gives every pixel S against rt_render_frames: what carrying the map costs;
  (b) maps with a quarter and a half of the pixels at 1 sample and the rest at S, chosen per pixel and per 8 x 8 block, against the
      uniform frame: the time as a share of the uniform time beside the share of the samples;
  (c) rt_build_sample_map of a moments plane against the bytes it moves (16 in, 4 out per pixel).
usage: tools/sample_map_timing.py [runs] [out.json]   (default: 7, profiles/sample_map_timing.json)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ray_tracer_amd import devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sample_map_timing.json")
W, H, S = 1920, 1080, 8

r = engine.Renderer(0)
BUFS = {}   # device address -> the devmem.DeviceBuffer that owns it


def device(nbytes, host=None):
    b = devmem.DeviceBuffer(nbytes)
    if host is not None:
        b.upload(host)
    BUFS[b.ptr] = b
    return b.ptr


def timed(call):
    r.sync()
    t = time.perf_counter()
    call()
    r.sync()
    return (time.perf_counter() - t) * 1e3


def interleaved(calls):
    """calls: name -> function. One warm-up of each, then `runs` rounds of all of them in turn."""
    for f in calls.values():
        timed(f)
    t = {k: [] for k in calls}
    for _ in range(runs):
        for k, f in calls.items():
            t[k].append(timed(f))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v)) for k, v in t.items()}


scene = scenes.sponza(0)[0]
r.upload_scene(scene)
pc = scenes.sponza_camera(W, H, raysPerPixel=S, progressive=1, singleRender=0)
frame = device(W * H * 16, np.zeros((H, W, 4), np.float32))
rng = np.random.default_rng(1)
maps = {"all at S": np.full((H, W), S, np.uint32)}
for share, label in ((0.25, "a quarter"), (0.5, "a half")):
    maps[f"{label} of the pixels at 1"] = np.where(rng.uniform(size=(H, W)) < share, 1, S).astype(np.uint32)
    blocks = np.where(rng.uniform(size=(H // 8, W // 8)) < share, 1, S).astype(np.uint32)
    maps[f"{label} of the 8x8 blocks at 1"] = np.kron(blocks, np.ones((8, 8), np.uint32))
d_maps = {k: device(m.nbytes, np.ascontiguousarray(m)) for k, m in maps.items()}
state = dict(frame=0)


def render(d_map):
    def call():
        pc.frameCount = state["frame"]
        state["frame"] += 1
        if d_map is None:
            r.render_frames(pc, W, H, 1, out_ptr=frame, sync=False)
        else:
            r.render_sampled(pc, W, H, d_map, out_ptr=frame, sync=False)
    return call


result = dict(produced_by="tools/sample_map_timing.py on one MI355X", scene="sponza stand-in", width=W, height=H, spp=S, runs=runs, pipelines={})
for pipeline, name in ((0, "multi-kernel"), (1, "fused")):
    r.set_tuning("pipeline", pipeline)
    calls = {"render_frames": render(None)}
    calls.update({k: render(p) for k, p in d_maps.items()})
    t = interleaved(calls)
    uniform = t["render_frames"]["median_ms"]
    rows = {}
    for k, v in t.items():
        rows[k] = dict(v, time_share=v["median_ms"] / uniform)
        if k in maps:
            rows[k]["sample_share"] = float(maps[k].sum()) / (S * W * H)
    result["pipelines"][name] = dict(kernel=r.last_kernel(), parts=r.last_parts(), cases=rows)
    for k, v in rows.items():
        print(f"{name:12s} {k:34s} {v['median_ms']:8.2f} ms (min {v['min_ms']:.2f})  time {100 * v['time_share']:5.1f} %"
              + (f"  samples {100 * v['sample_share']:5.1f} %" if "sample_share" in v else ""), flush=True)
r.set_tuning("pipeline", -1)

# (c) the map kernel: a synthetic moments plane with every case of the rule
mom = np.empty((H, W, 4), np.float32)
mom[..., 0] = rng.uniform(0.0, 2.0, (H, W))
mom[..., 2] = (10.0 ** rng.uniform(-3.0, 0.5, (H, W)) * mom[..., 0]) ** 2
mom[..., 1] = mom[..., 2] + mom[..., 0] ** 2
mom[..., 3] = np.floor(rng.uniform(0.0, 33.0, (H, W)))
d_mom, d_map = device(mom.nbytes, mom), device(W * H * 4)
t = interleaved({"build": lambda: r._check(r._l.rt_build_sample_map(r._h, W, H, C.c_void_p(d_mom), None, C.c_void_p(d_map)), "rt_build_sample_map")})
nbytes = W * H * 20
result["build_sample_map"] = dict(t["build"], bytes=nbytes, gb_per_s=nbytes / t["build"]["median_ms"] / 1e6, stats=r.sample_map_stats())
print(f"rt_build_sample_map {W}x{H}: {t['build']['median_ms']:.3f} ms (min {t['build']['min_ms']:.3f}) for {nbytes / 1e6:.1f} MB: "
      f"{result['build_sample_map']['gb_per_s']:.0f} GB/s including the launch and the synchronisation", flush=True)
with open(out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
for p in [frame, d_mom, d_map] + list(d_maps.values()):
    BUFS.pop(p).free()
r.close()
