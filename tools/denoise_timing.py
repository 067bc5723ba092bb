#!/usr/bin/env python3
"""rt_denoise (K = 5, defaults) against one 8-spp rt_render and the first-hit AOV pass of the same frame: the Sponza stand-in at
1920 x 1080 (scenes.sponza_camera) and Cornell with its spheres at 1728 x 1117 (the CLI's default size). All three write into
device buffers (no read-back) and are timed with the host clock around the enqueue and an rt_sync; one warm-up of each, then
`runs` of each, interleaved; median and min. Then the quality ratios of tests/test_denoise.py (4 spp against 1024 spp, clamped
to [0, 1]) for its two scenes at 160 x 120.
usage: tools/denoise_timing.py [runs] [out.json]   (default: 7, profiles/denoise_timing.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C  # noqa: E402

from ray_tracer_amd import _capi, devmem, engine, scenes  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "denoise_timing.json")
CASES = [("sponza stand-in", lambda: scenes.sponza(0)[0], scenes.sponza_camera, 1920, 1080),
         ("cornell + spheres", lambda: scenes.cornell(True)[0], engine.push_constants, 1728, 1117)]

r = engine.Renderer(0)
params = _capi.RtDenoiseParams()
r._l.rt_denoise_params_default(C.byref(params))
rows = []
for label, make, camera, W, H in CASES:
    r.upload_scene(make())
    pc = camera(W, H, singleRender=1, sampleLimit=8)
    bufs = [devmem.DeviceBuffer(W * H * 16) for _ in range(7)]
    frame, dout = bufs[0].ptr, bufs[6].ptr
    ptrs = {k: b.ptr for k, b in zip(engine.AOV_PLANES, bufs[1:6])}
    planes = _capi.RtAovBuffers(**ptrs)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def render():
        r.render(pc, W, H, out_ptr=frame)   # sync=True: rt_sync

    def aovs():
        r.render_aovs(pc, W, H, out_ptrs=ptrs)

    def denoise():
        r._check(r._l.rt_denoise(r._h, W, H, frame, C.byref(planes), C.byref(params), dout), "rt_denoise")
        r.sync()

    timed(render)   # warm-up: code objects, the ray-cost probe, the path state, the denoiser's work planes
    timed(aovs)
    timed(denoise)
    tf, ta, td = [], [], []
    for _ in range(runs):
        tf.append(timed(render))
        ta.append(timed(aovs))
        td.append(timed(denoise))
    med = statistics.median
    row = dict(scene=label, width=W, height=H, spp=8, iterations=params.iterations, runs=runs,
               frame_ms=round(med(tf), 3), frame_ms_min=round(min(tf), 3), frame_pipeline=r.last_pipeline(),
               aov_ms=round(med(ta), 3), aov_ms_min=round(min(ta), 3),
               denoise_ms=round(med(td), 3), denoise_ms_min=round(min(td), 3),
               denoise_share_of_frame=round(med(td) / med(tf), 4), denoise_mpixels_per_s=round(W * H / med(td) / 1e3, 1))
    rows.append(row)
    for b in bufs:
        b.free()
    print(json.dumps(row), flush=True)

from denoise_float64 import _checker_scene  # noqa: E402
from test_denoise import quality  # noqa: E402

W, H = 160, 120
s, _, tex = _checker_scene()
for label, scene, textures in (("cornell + spheres", scenes.cornell(True)[0], None), ("cornell + checkerboard albedo map", s, [tex])):
    q, _ = quality(r, scene, W, H, textures)
    row = dict(scene=label, width=W, height=H, spp=4, reference_spp=1024, iterations=5,
               **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in q.items()})
    rows.append(row)
    print(json.dumps(row), flush=True)
r.close()
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
print("wrote", out)
