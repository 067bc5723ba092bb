"""TEST INFRASTRUCTURE — the first-hit planes of a frame as the oracle gives them, shared by tests/test_ao_rays_host.py and
tests/test_ao_float64.py (the planes engine.ao_rays shoots from on the CPU)."""
import numpy as np

from oracle import pyoracle
from ray_tracer_amd import engine

import brute_force as bf


def oracle_planes(scene, pc, w, h):
    """The dict render_aovs() returns, from the oracle's hit records of the float64 camera's rays (rounded)."""
    d = bf.camera_dirs(pc, w, h).astype(np.float32).reshape(-1, 3)
    o = np.repeat(np.asarray(list(pc.camInfo.pos), np.float32)[None], len(d), 0)
    r = engine.hits_to_numpy(pyoracle.trace_rays(scene, o, d))
    hit = r["didHit"].astype(bool)
    none = np.uint32(0xFFFFFFFF)
    shape = lambda x: x.reshape((h, w) + x.shape[1:])   # noqa: E731
    return dict(depth=shape(r["dst"]), normal=shape(r["normal"]), position=shape(r["hitPoint"]), albedo=np.zeros((h, w, 3), np.float32),
                ray_dir=shape(d), object=shape(np.where(hit, r["objectHitIndex"], none)), triangle=shape(np.where(hit, r["triHitIndex"], none)),
                material=shape(np.where(hit, r["materialIndex"], none)), hit=shape(hit), sphere=shape(r["isSphere"].astype(bool)),
                front_face=shape(r["frontFace"].astype(bool)))
