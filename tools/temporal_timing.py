#!/usr/bin/env python3
"""rt_temporal_accumulate (defaults) against one 1-spp rt_render, the first-hit AOV pass and rt_denoise (K = 5) of the same frame,
along a camera path that yaws 0.5 degrees per frame so that every timed call reprojects into a camera that differs from its
own: the Sponza stand-in at 1920 x 1080 (scenes.sponza_camera) and Cornell with its spheres at 1728 x 1117 (the CLI's default
size). The method is tools/denoise_timing.py's: all four write into device buffers (no read-back) and are timed with the host
clock around the enqueue and an rt_sync; one warm-up of each, then `runs` of each, interleaved; median and min. The last call's
moments plane is read back once, after the timing, for the share of the frame that kept a history. Then the error ratios of
tests/test_temporal.py's quality test.
--moving-object: the pass with rt_temporal_track_motion on, same scenes, sizes, camera path and method. Every iteration has a
frame before which one object of the Sponza stand-in (the one with the most pixels on screen) or one Cornell sphere was moved
0.002 along x through rt_update_objects / rt_update_spheres (not timed), so that the call builds and uploads the motion table and
runs k_tp_accumulate_motion, and a frame without an edit, on which the same call runs k_tp_accumulate as with tracking off;
rt_temporal_motion_state says which one ran. Both are timed the same way in the same run, and the ratio is what is reported.
usage: tools/temporal_timing.py [--moving-object] [runs] [out.json]
(default: 7, profiles/temporal_timing.json or, with --moving-object, profiles/temporal_motion_timing.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

from ray_tracer_amd import _capi, devmem, engine, scenes  # noqa: E402

MOVING = "--moving-object" in sys.argv
argv = [a for a in sys.argv if a != "--moving-object"]
runs = int(argv[1]) if len(argv) > 1 else 7
out = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "temporal_motion_timing.json" if MOVING else "temporal_timing.json")
CASES = [("sponza stand-in", lambda: scenes.sponza(0)[0], scenes.sponza_camera, (2.0, 0.0, 0.0), 1920, 1080),
         ("cornell + spheres", lambda: scenes.cornell(True)[0], engine.push_constants, (4.0, 0.0, 0.0), 1728, 1117)]
# per pixel: five input records, four taps of three records, the frame, the moments and three history records, 16 bytes each
BYTES_PER_PIXEL = (5 + 4 * 3 + 2 + 3) * 16

r = engine.Renderer(0)
rows = []


def moving_object_mode():
    from util import EditedScene

    r.temporal_track_motion(True)
    for label, make, camera, angles, W, H in CASES:
        scene = make()
        e = EditedScene(scene)
        r.upload_scene(scene)
        bufs = [devmem.DeviceBuffer(W * H * 16) for _ in range(8)]
        frame, acc, mom = bufs[0].ptr, bufs[6].ptr, bufs[7].ptr
        ptrs = {k: b.ptr for k, b in zip(engine.AOV_PLANES, bufs[1:6])}
        planes = _capi.RtAovBuffers(**ptrs)
        state = dict(k=0, edits=0)

        def frame_of(edit):
            """One frame of the path, after an edit or not: the time of the temporal call alone, and what it says it found."""
            k = state["k"]
            state["k"] = k + 1
            if edit:
                state["edits"] += 1
                if target[0] == "object":
                    e.objects[target[1]].transformMatrix[12] = x0 + 0.002 * state["edits"]
                    e.push(r, "objects")
                else:
                    e.spheres[target[1]].position[0] = x0 + 0.002 * state["edits"]
                    e.push(r, "spheres")
            pc = camera(W, H, cameraAngles=(angles[0], angles[1] + 0.5 * k, angles[2]), progressive=0, raysPerPixel=1, frameCount=k)
            r.render(pc, W, H, out_ptr=frame)
            r.render_aovs(pc, W, H, out_ptrs=ptrs)
            r.sync()
            t = time.perf_counter()
            r._check(r._l.rt_temporal_accumulate(r._h, W, H, C.byref(pc.camInfo), frame, C.byref(planes), None, acc, mom), "rt_temporal_accumulate")
            r.sync()
            return (time.perf_counter() - t) * 1e3, r.temporal_motion_state()

        # what to move: the Cornell sphere 2 (diffuse), or the object with the most pixels in the first frame
        target, x0 = ("sphere", 2), 0.0
        frame_of(False)
        ids = np.empty((H, W, 4), np.uint32)
        bufs[5].download(into=ids)   # (the ids plane)
        if label.startswith("sponza"):
            mesh = ids[..., 0][(ids[..., 3] & 3) == 1]
            target = ("object", int(np.bincount(mesh).argmax()))
            x0 = float(e.objects[target[1]].transformMatrix[12])
        else:
            x0 = float(e.spheres[2].position[0])
        for edit in (True, False):   # warm-up of both kernels, the table and its staging copy
            frame_of(edit)
        t_motion, t_static = [], []
        for _ in range(runs):
            ms, st = frame_of(True)
            assert st["movedObjects"] + st["movedSpheres"] == 1 and st["replacedObjects"] == 0, st
            t_motion.append(ms)
            ms, st = frame_of(False)
            assert not any(st.values()), st
            t_static.append(ms)
        m = np.empty((H, W, 4), np.float32)
        bufs[7].download(into=m)
        bufs[5].download(into=ids)
        N = m[..., 3]
        on_target = (ids[..., 0] == target[1]) & ((ids[..., 3] & 3) == (1 if target[0] == "object" else 3))
        med = statistics.median
        row = dict(scene=label, width=W, height=H, spp=1, yaw_deg_per_frame=0.5, runs=runs, moved=f"{target[0]} {target[1]}", step=0.002,
                   temporal_motion_ms=round(med(t_motion), 3), temporal_motion_ms_min=round(min(t_motion), 3),
                   temporal_static_ms=round(med(t_static), 3), temporal_static_ms_min=round(min(t_static), 3),
                   motion_over_static=round(med(t_motion) / med(t_static), 3), motion_over_static_min=round(min(t_motion) / min(t_static), 3),
                   moved_share_of_pixels=round(float(on_target.mean()), 4),
                   history_share_on_moved=round(float((N[on_target] > 1).sum() / max((N[on_target] > 0).sum(), 1)), 4),
                   history_share_of_filtered=round(float((N > 1).sum() / max((N > 0).sum(), 1)), 4))
        rows.append(row)
        for b in bufs:
            b.free()
        print(json.dumps(row), flush=True)
    r.temporal_track_motion(False)
    r.close()
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)
    print("wrote", out)


if MOVING:
    moving_object_mode()
    sys.exit(0)
for label, make, camera, angles, W, H in CASES:
    r.upload_scene(make())
    bufs = [devmem.DeviceBuffer(W * H * 16) for _ in range(9)]
    frame, acc, mom, dout = bufs[0].ptr, bufs[6].ptr, bufs[7].ptr, bufs[8].ptr
    ptrs = {k: b.ptr for k, b in zip(engine.AOV_PLANES, bufs[1:6])}
    planes = _capi.RtAovBuffers(**ptrs)
    state = dict(k=0, pc=None)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def render():
        k = state["k"]
        state["pc"] = camera(W, H, cameraAngles=(angles[0], angles[1] + 0.5 * k, angles[2]), progressive=0, raysPerPixel=1, frameCount=k)
        state["k"] = k + 1
        r.render(state["pc"], W, H, out_ptr=frame)   # sync=True: rt_sync

    def aovs():
        r.render_aovs(state["pc"], W, H, out_ptrs=ptrs)

    def temporal():
        r._check(r._l.rt_temporal_accumulate(r._h, W, H, C.byref(state["pc"].camInfo), frame, C.byref(planes), None, acc, mom), "rt_temporal_accumulate")
        r.sync()

    def denoise():
        r._check(r._l.rt_denoise(r._h, W, H, acc, C.byref(planes), None, dout), "rt_denoise")
        r.sync()

    steps = (render, aovs, temporal, denoise)
    for fn in steps:   # warm-up: code objects, the ray-cost probe, the path state, the histories and work planes
        timed(fn)
    t = [[] for _ in steps]
    for _ in range(runs):
        for ts, fn in zip(t, steps):
            ts.append(timed(fn))
    med = statistics.median
    m = np.empty((H, W, 4), np.float32)
    bufs[7].download(into=m)
    N = m[..., 3]
    row = dict(scene=label, width=W, height=H, spp=1, yaw_deg_per_frame=0.5, runs=runs,
               frame_ms=round(med(t[0]), 3), frame_ms_min=round(min(t[0]), 3), frame_pipeline=r.last_pipeline(),
               aov_ms=round(med(t[1]), 3), aov_ms_min=round(min(t[1]), 3),
               temporal_ms=round(med(t[2]), 3), temporal_ms_min=round(min(t[2]), 3),
               denoise_ms=round(med(t[3]), 3), denoise_ms_min=round(min(t[3]), 3),
               temporal_share_of_frame=round(med(t[2]) / med(t[0]), 4), temporal_mpixels_per_s=round(W * H / med(t[2]) / 1e3, 1),
               bytes_per_pixel=BYTES_PER_PIXEL, temporal_gbytes_per_s=round(W * H * BYTES_PER_PIXEL / med(t[2]) / 1e6, 1),
               filtered_share=round(float((N > 0).mean()), 4), history_share_of_filtered=round(float((N > 1).sum() / max((N > 0).sum(), 1)), 4),
               longest_history=float(N.max()))
    rows.append(row)
    for b in bufs:
        b.free()
    print(json.dumps(row), flush=True)

from test_temporal import quality  # noqa: E402

q = quality(r, scenes.cornell(True)[0], 160, 120)
row = dict(scene="cornell + spheres", width=160, height=120, spp=4, frames=8, reference_spp=1024,
           **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in q.items()})
rows.append(row)
print(json.dumps(row), flush=True)
r.close()
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
print("wrote", out)
