#!/usr/bin/env python3
"""rt_render_aovs against one 8-spp rt_render of the same frame: the Sponza stand-in at 1920 x 1080 (scenes.sponza_camera) and
Cornell with its spheres at 1728 x 1117 (the CLI's default size). Both write into device buffers (no read-back) and are timed
with the host clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved; median and min.
usage: tools/aov_timing.py [runs] [out.json]   (default: 7, profiles/aov_timing.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_amd import devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "aov_timing.json")
CASES = [("sponza stand-in", lambda: scenes.sponza(0)[0], scenes.sponza_camera, 1920, 1080),
         ("cornell + spheres", lambda: scenes.cornell(True)[0], engine.push_constants, 1728, 1117)]

r = engine.Renderer(0)
rows = []
for label, make, camera, W, H in CASES:
    r.upload_scene(make())
    pc = camera(W, H, singleRender=1, sampleLimit=8)
    bufs = [devmem.DeviceBuffer(W * H * 16) for _ in range(6)]
    frame = bufs[0].ptr
    ptrs = {k: b.ptr for k, b in zip(engine.AOV_PLANES, bufs[1:])}

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def render():
        r.render(pc, W, H, out_ptr=frame)   # sync=True: rt_sync

    def aovs():
        r.render_aovs(pc, W, H, out_ptrs=ptrs)

    timed(render)   # warm-up: code objects, the ray-cost probe, the path state
    timed(aovs)
    tf, ta = [], []
    for _ in range(runs):
        tf.append(timed(render))
        ta.append(timed(aovs))
    pipeline, parts = r.last_pipeline(), r.last_parts()
    r.reset_counters()
    aovs()
    c = r.counters()
    row = dict(scene=label, width=W, height=H, spp=8, runs=runs, frame_ms=round(statistics.median(tf), 3), frame_ms_min=round(min(tf), 3),
               frame_pipeline=pipeline, frame_parts=parts, aov_ms=round(statistics.median(ta), 3), aov_ms_min=round(min(ta), 3),
               aov_share_of_frame=round(statistics.median(ta) / statistics.median(tf), 4), aov_kernel=r.last_kernel(),
               aov_mrays_per_s=round(W * H / statistics.median(ta) / 1e3, 1),
               aov_box_tests_per_ray=round(c["boxTests"] / c["raysTraced"], 1), aov_tri_tests_per_ray=round(c["triTests"] / c["raysTraced"], 1),
               frame_box_tests_per_ray=round(r.ray_cost(), 1))
    rows.append(row)
    for b in bufs:
        b.free()
    print(json.dumps(row), flush=True)
r.close()
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
print("wrote", out)
