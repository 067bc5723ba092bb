#!/usr/bin/env python3
"""One single-render dispatch of a scene that binds the alpha, metalness and bump maps, on the multi-kernel pipeline and on the
fused one (k_render_fused_maps): the all-maps plane scene of tests/test_textures.py, and dread.obj with its albedo map plus the
three generated maps of test_textures._map_set bound to its material. Three sizes (256 x 256, 640 x 360, rank 0's rows of 8 GPUs
at 1920 x 1080), three settings (multi-kernel; fused_maps 1 + pipeline 1; fused_maps 1 + pipeline -1, the size / short-ray rule).
Median of 5 timed dispatches after one warm-up, into a device buffer (no read-back).
usage: tools/fused_maps_timing.py [spp] [out.json]"""
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from ray_tracer_amd import engine  # noqa: E402
from test_textures import _bound, _dread_scene, _map_set  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
out = sys.argv[2] if len(sys.argv) > 2 else None
SIZES = [("256x256", 256, 256, 0, 1), ("640x360", 640, 360, 0, 1), ("1080p rank 0 of 8", 1920, 1080, 0, 8)]
SETTINGS = [("multi-kernel", 0, -1), ("fused pipeline 1", 1, 1), ("fused pipeline -1", 1, -1)]


def scenes(tmp):
    tex = _map_set()
    plane = _bound(Path(tmp) / "plane", 0, 2.5, alphaIndex=1, metalnessIndex=2, bumpIndex=3)
    d = _dread_scene()
    mi = d.find_material(os.path.join(engine.ASSET_DIR, "dread.mtl") + "/M_Body")
    m = d.material(mi)
    m.alphaIndex, m.metalnessIndex, m.bumpIndex = 1, 2, 3
    d.set_material(mi, m)
    return [("plane, all maps", plane, tex), ("dread + alpha/metalness/bump", d, engine.load_textures(d) + tex[1:])]


r = engine.Renderer(0)
rows = []
with tempfile.TemporaryDirectory() as tmp:
    for label, s, tex in scenes(tmp):
        edited = not isinstance(s, engine.Scene)
        r.upload_scene(s.scene if edited else s)
        if edited:
            s.push(r, "objects")
            s.push(r, "materials")
        r.upload_textures(tex)
        for size, W, H, row0, stride in SIZES:
            nRows = (H - row0 + stride - 1) // stride
            buf = torch.empty((nRows, W, 4), dtype=torch.float32, device="cuda")
            pc = engine.push_constants(W, H, singleRender=1, sampleLimit=spp, environmentOn=True)
            for setting, fm, pipe in SETTINGS:
                r.set_tuning("fused_maps", fm)
                r.set_tuning("pipeline", pipe)
                ts = []
                for k in range(6):
                    t = time.perf_counter()
                    r.render(pc, W, H, row0=row0, rowStride=stride, nRows=nRows, out_ptr=buf.data_ptr())
                    if k:
                        ts.append((time.perf_counter() - t) * 1e3)
                row = dict(scene=label, size=size, setting=setting, spp=spp, ms=round(statistics.median(ts), 3),
                           ms_min=round(min(ts), 3), pipeline=r.last_pipeline(), kernel=r.last_kernel(), box_per_ray=round(r.ray_cost(), 1))
                rows.append(row)
                print(json.dumps(row), flush=True)
r.set_tuning("fused_maps", 0)
r.set_tuning("pipeline", -1)
r.close()
if out:
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)
