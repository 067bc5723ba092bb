#!/usr/bin/env python3
"""What rt_query_irradiance and rt_query_sh_probes cost on top of the radiance pipeline they run: the bench scene (the Sponza
stand-in through scenes.sponza_camera), 65 536 first-hit positions and normals of a frame, 64 samples per point (4.2 M rays), bounce
limit 8, both forms, beside rt_query_radiance over the very same rays (made on the host by engine.irradiance_rays and put in device
memory, with their ids) in the same run. The yardstick is that rt_query_radiance call; the figure is what the two kernels
(k_irradiance_rays, k_irradiance_gather) and the chunking add to it, as ms and as a share. Everything reads and writes device
buffers (no read-back) and is timed with the host clock around the enqueue and an rt_sync; two warm-ups of each, then `runs` of each,
interleaved; median, min, max. Before anything is timed the device's answers are compared bit for bit with
engine.irradiance_gather of the radiance records.
usage: tools/irradiance_timing.py [runs] [out.json]   (default: 9, profiles/irradiance_timing.json)"""
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
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "irradiance_timing.json")
W, H, N, S, BOUNCES = 320, 240, 65536, 64, 8

r = engine.Renderer(0)
BUFS = {}   # device address -> the devmem.DeviceBuffer that owns it


def device(nbytes, host=None):
    b = devmem.DeviceBuffer(nbytes)
    if host is not None:
        b.upload(np.ascontiguousarray(host))
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
pc = scenes.sponza_camera(W, H, singleRender=1, sampleLimit=1, bounceLimit=BOUNCES, progressive=0)
a = r.render_aovs(pc, W, H)
hit = np.flatnonzero(a["hit"].reshape(-1))
assert len(hit) >= N, f"{len(hit)} of {W * H} camera rays hit: fewer than {N}"
hit = hit[:N]
pts = np.ascontiguousarray(a["position"].reshape(-1, 3)[hit], np.float32)
nrm = np.ascontiguousarray(a["normal"].reshape(-1, 3)[hit], np.float32)
env = pc.environment
d_p, d_n = device(pts.nbytes, pts), device(nrm.nbytes, nrm)
d_E, d_c = device(N * 16), device(N * 108)
rays = {}
for form, normals in (("irradiance", nrm), ("probes", None)):
    o, d, rid = engine.irradiance_rays(pts, normals, samples=S)
    rays[form] = (device(o.nbytes, o), device(d.nbytes, d), device(rid.nbytes, rid), device(N * S * 16))

passes = {
    "irradiance": lambda: r.query_irradiance(d_p, d_n, samples=S, bounces=BOUNCES, environment=env, n=N, out=d_E),
    "radiance_of_irradiance_rays": lambda: r.query_radiance(*rays["irradiance"][:2], samples=1, bounces=BOUNCES, ids=rays["irradiance"][2], environment=env,
                                                            n=N * S, out=rays["irradiance"][3]),
    "probes": lambda: r.query_sh_probes(d_p, samples=S, bounces=BOUNCES, environment=env, n=N, out=d_c),
    "radiance_of_probe_rays": lambda: r.query_radiance(*rays["probes"][:2], samples=1, bounces=BOUNCES, ids=rays["probes"][2], environment=env, n=N * S,
                                                       out=rays["probes"][3]),
}
kernels = {}
for k, fn in passes.items():
    timed(fn)
    timed(fn)
    kernels[k] = r.last_kernel()
same_E = bool(np.array_equal(host(d_E, (N, 4)).view(np.uint32),
                             engine.irradiance_gather(host(rays["irradiance"][3], (N * S, 4)), N, samples=S).view(np.uint32)))
same_c = bool(np.array_equal(host(d_c, (N, 9, 3)).view(np.uint32),
                             engine.irradiance_gather(host(rays["probes"][3], (N * S, 4)), N, samples=S, sphere=True).view(np.uint32)))
assert same_E and same_c, (same_E, same_c)

ms = {k: [] for k in passes}
for _ in range(runs):
    for k, fn in passes.items():
        ms[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in ms.items()}
row = dict(scene="sponza stand-in (the bench scene)", points=N, samples=S, rays=N * S, bounceLimit=BOUNCES, runs=runs, kernels=kernels,
           bit_identical=dict(irradiance=same_E, probes=same_c))
for k, v in ms.items():
    row[f"{k}_ms"] = dict(median=round(med[k], 3), min=round(min(v), 3), max=round(max(v), 3))
for form, base in (("irradiance", "radiance_of_irradiance_rays"), ("probes", "radiance_of_probe_rays")):
    row[f"{form}_added_ms"] = round(med[form] - med[base], 3)
    row[f"{form}_added_share"] = round((med[form] - med[base]) / med[base], 4)
    row[f"{base}_spread"] = round((max(ms[base]) - min(ms[base])) / med[base], 4)
r.close()
print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(row, f, indent=1)
print("wrote", out)
