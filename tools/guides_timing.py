#!/usr/bin/env python3
"""rt_render_guides against rt_render_aovs on the same frame: the Sponza stand-in at 1920 x 1080 (scenes.sponza_camera), which has
no mirror, so that every round after the first is empty and the difference is what `maxBounces` empty rounds cost over the plain
AOV pass; and Cornell with its spheres at 1728 x 1117 (the CLI's default size), where the mirror sphere's pixels go on. Both write
into device buffers (no read-back) and are timed with the host clock around the enqueue and an rt_sync; one warm-up of each, then
`runs` of each, interleaved; median and min, for maxBounces 0, 1, 4 and 8, with and without the first-hit planes.
usage: tools/guides_timing.py [runs] [out.json]   (default: 7, profiles/guides_timing.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

from ray_tracer_amd import _capi, devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "guides_timing.json")
CASES = [("sponza stand-in", lambda: scenes.sponza(0)[0], scenes.sponza_camera, 1920, 1080),
         ("cornell + spheres", lambda: scenes.cornell(True)[0], engine.push_constants, 1728, 1117)]
BOUNCES = (0, 1, 4, 8)

r = engine.Renderer(0)
rows = []
for label, make, camera, W, H in CASES:
    r.upload_scene(make())
    pc = r.fill_counts(camera(W, H))
    bufs = [devmem.DeviceBuffer(W * H * 16) for _ in range(10)]
    ptrs = {k: b.ptr for k, b in zip(engine.AOV_PLANES, bufs[:5])}
    guides = _capi.RtAovBuffers(**ptrs)
    first = _capi.RtAovBuffers(**{k: b.ptr for k, b in zip(engine.AOV_PLANES, bufs[5:])})

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def aovs():
        r.render_aovs(pc, W, H, out_ptrs=ptrs)   # sync=True: rt_sync

    def guide_pass(n, with_first):
        def run():
            r._check(r._l.rt_render_guides(r._h, C.byref(pc), W, H, 0, 1, H, n, C.byref(guides), C.byref(first) if with_first else None),
                     "rt_render_guides")
            r.sync()
        return run

    passes = {(n, wf): guide_pass(n, wf) for n in BOUNCES for wf in (False, True)}
    timed(aovs)   # warm-up: code objects, the path state
    for p in passes.values():
        timed(p)
    ta, tg = [], {k: [] for k in passes}
    for _ in range(runs):
        ta.append(timed(aovs))
        for k, p in passes.items():
            tg[k].append(timed(p))
    med = statistics.median
    r.reset_counters()
    passes[(8, False)]()
    c = r.counters()
    row = dict(scene=label, width=W, height=H, runs=runs, aov_ms=round(med(ta), 3), aov_ms_min=round(min(ta), 3),
               rays_per_pixel_at_8=round(c["raysTraced"] / (W * H), 4), trace_launches_at_8=c["traceLaunches"])
    for (n, wf), t in tg.items():
        key = f"guides_{n}{'_first_hit' if wf else ''}"
        row[key + "_ms"], row[key + "_ms_min"] = round(med(t), 3), round(min(t), 3)
    row["ms_per_round_over_aov"] = round((med(tg[(8, False)]) - med(tg[(0, False)])) / 8, 4)
    row["guides_8_over_aov"] = round(med(tg[(8, False)]) / med(ta), 4)
    rows.append(row)
    for b in bufs:
        b.free()
    print(json.dumps(row), flush=True)
r.close()
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
print("wrote", out)
