#!/usr/bin/env python3
"""Does a variance-driven sample map pay? Cornell with its spheres at 160 x 120, a still camera, eight non-progressive frames with
consecutive frameCounts through the temporal pass (max_history = the frame count, so the result is the plain mean of the frames),
against a 1024-spp render, everything clamped to [0, 1] as tests/test_temporal.py's quality test has it.
  run A: frame 0 at 4 spp, every later frame through rt_render_sampled with the map rt_build_sample_map makes of the moments so far
         (base 4, min 1, max 16, the default target and floor);
  run B: eight uniform frames at the smallest count whose total samples reach A's.
Reported: the samples of both, the MSE over the filtered set (hits on non-emitters: the pixels the pass accumulates) and the worst
8 x 8 tile's MSE (over the tile's filtered pixels; tiles with fewer than 32 of them are left out), and the ratios A / B.
usage: tools/sample_map_quality.py [out.json]   (default: profiles/sample_map_quality.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ray_tracer_amd import engine, scenes  # noqa: E402

W, H, FRAMES, BASE, REF_SPP = 160, 120, 8, 4, 1024
MAP = dict(base_samples=BASE, min_samples=1, max_samples=16)


def measure(r):
    scene = scenes.cornell(True)[0]
    r.upload_scene(scene)
    a = scene.arrays()
    emission = np.array([a.materials[i].emissionStrength for i in range(a.materialCount)])

    def pc_of(k, spp):
        return engine.push_constants(W, H, progressive=0, raysPerPixel=spp, frameCount=k)

    aovs = r.render_aovs(pc_of(0, 1), W, H)
    F = aovs["hit"] & (emission[np.where(aovs["hit"], aovs["material"], 0)] == 0.0)
    clean = r.render(engine.push_constants(W, H, singleRender=1, sampleLimit=REF_SPP, frameCount=FRAMES), W, H)

    def clip(x):
        return np.clip(np.asarray(x, np.float64)[..., :3], 0.0, 1.0)

    def errors(img):
        e = ((clip(img) - clip(clean)) ** 2).mean(axis=-1)
        tiles = []
        for y in range(0, H, 8):
            for x in range(0, W, 8):
                f = F[y:y + 8, x:x + 8]
                if f.sum() >= 32:
                    tiles.append((float(e[y:y + 8, x:x + 8][f].mean()), x, y))
        worst = max(tiles)
        return dict(mse=float(e[F].mean()), worst_tile_mse=worst[0], worst_tile=[worst[1], worst[2]], tiles=len(tiles))

    def run(spp_of_frame0, adaptive):
        r.temporal_reset()
        samples, out, per_frame = 0, None, []
        counts = None
        for k in range(FRAMES):
            if counts is None:
                r.render(pc_of(k, spp_of_frame0), W, H)
                n = spp_of_frame0 * W * H
            else:
                r.render_sampled(pc_of(k, MAP["max_samples"]), W, H, counts)
                n = int(counts.sum())
            samples += n
            per_frame.append(n)
            out = r.temporal_accumulate(pc_of(k, 1), max_history=FRAMES)
            if adaptive:
                counts = r.build_sample_map(**MAP)
        return out, samples, per_frame

    img_a, samples_a, per_frame = run(BASE, True)
    spp_b = -(-samples_a // (FRAMES * W * H))
    img_b, samples_b, _ = run(spp_b, False)
    ea, eb = errors(img_a), errors(img_b)
    return dict(scene="cornell + spheres", width=W, height=H, frames=FRAMES, reference_spp=REF_SPP, map=MAP, filtered_pixels=int(F.sum()),
                A=dict(samples=samples_a, samples_per_frame=per_frame, **ea), B=dict(spp=int(spp_b), samples=samples_b, **eb),
                mse_ratio=ea["mse"] / eb["mse"], worst_tile_ratio=ea["worst_tile_mse"] / eb["worst_tile_mse"])


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sample_map_quality.json")
    r = engine.Renderer(0)
    q = measure(r)
    q["produced_by"] = "tools/sample_map_quality.py on one MI355X"
    with open(out, "w") as f:
        json.dump(q, f, indent=1)
        f.write("\n")
    print(json.dumps(q))
    r.close()
