#!/usr/bin/env python3
"""What deforming a mesh in place costs and what it leaves behind (rt_update_points; DESIGN.md, "Deforming meshes"), on Cornell +
bunny and on the Sponza stand-in (262 k triangles), every point of the model displaced by a smooth seeded field.
  (a) update time: the median of `runs` rt_update_points calls of all the model's points after a warm-up (host clock around the
      synchronous call), against the only way to do the same without it: the model's meshes added again to a scene whose BVHs come
      from rt_bvh_build through the hook (rt_scene_add_mesh: the triangle records, the centroids, the build, the permutation),
      then rt_upload_scene. Both sides start from deformed positions computed before the clock starts. What a rebuild shares with
      any scene and an application keeps from the first time (the spheres, the materials and their file, the Cornell box or the
      light: `scene_setup_ms`) is timed beside it and is not part of the comparison; `of_it_rt_bvh_build_ms` is the device
      builder's own time summed over the meshes.
  (b) traversal cost after the update: executed box tests per ray, (boxTests - skippedBoxTests) / raysTraced, of one frame on the
      refit tree and on a tree rebuilt for the same deformed points, at a small and a large displacement (1 % and 25 % of the
      model's extent, one wave across it).
usage: tools/refit_timing.py [runs] [out.json]   (default: 25, profiles/refit_timing.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ray_tracer_amd import engine, scenes  # noqa: E402

runs = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 25
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "refit_timing.json")
REBUILDS = 5
W, H = 960, 540

r = engine.Renderer(0)


def field(extent, centre, share, seed):
    """p -> p + share * extent * sin(k (p - centre) + phase), one wave across the model, as a function of float32 positions."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.7, 1.3, (3, 3)) * 2 * np.pi / extent
    ph = rng.uniform(0, 6.28, 3)

    def f(p):
        q = p.reshape(-1, 3).astype(np.float64)
        return (q + share * extent * np.sin((q - centre) @ k.T + ph)).astype(np.float32).reshape(p.shape)
    return f


def bunny_model():
    s = engine.Scene()
    s.read_obj(os.path.join(engine.ASSET_DIR, "bunny.obj"), engine.placement(), 0)
    a = s.numpy()
    tri = a["triangles"].view(np.uint32).reshape(-1, 12)[:, :3]
    pts = a["triPoints"].view(np.float32).reshape(-1, 8)
    return pts[tri][:, :, :3].reshape(-1, 9).copy(), pts[tri][:, :, 4:7].reshape(-1, 9).copy()


BUNNY = bunny_model()


class Clock:
    """Milliseconds per named share of a build."""

    def __init__(self):
        self.ms = dict(setup=0.0, meshes=0.0, bvh=0.0)
        self.t = time.perf_counter()

    def lap(self, share):
        now = time.perf_counter()
        self.ms[share] += (now - self.t) * 1e3
        self.t = now


def build_bunny(positions, device_bvh, clock=None):
    """Cornell + the bunny's triangles at `positions` (None: as in the file). Returns the scene and the model's point range."""
    clock = clock or Clock()
    s = engine.Scene()
    s.prepare_storage_buffers()
    n0 = s.counts()["triPoints"]
    clock.lap("setup")
    if device_bvh:
        s.use_device_bvh(r)
    s.add_mesh("bunny", BUNNY[0] if positions is None else positions[0], BUNNY[1], engine.placement(position=(0.0, 0.53, 0.0), scale=0.7, samplerIndex=1), 0)
    clock.ms["bvh"] += r.bvh_last_build_ms() if device_bvh else 0.0
    clock.lap("meshes")
    return s, (n0, s.counts()["triPoints"])


SPONZA = list(scenes.sponza_standin_groups(scenes.SPONZA_TRIS, 1))


def build_sponza(positions, device_bvh, clock=None):
    """scenes.sponza()'s stand-in with its groups at `positions` (None: as generated)."""
    clock = clock or Clock()
    s = engine.Scene()
    for i in range(10):
        s.set_sphere(i, (0, 0, 0), 0.0, 0)
    for m in (engine.default_material(), engine.default_material(albedo=(1, 0, 0)), engine.default_material(albedo=(0, 1, 0)),
              engine.default_material(albedo=(0, 0, 0), emissionColor=(1, 1, 1), emissionStrength=2.4),
              engine.default_material(reflectance=1.0), engine.default_material(ior=2.0)):
        s.add_material(m)
    first = s.counts()["materials"]
    s.read_mtl(scenes._asset("sponza.mtl"))
    nmat = s.counts()["materials"] - first
    clock.lap("setup")
    if device_bvh:
        s.use_device_bvh(r)
    for gi, (name, pos, nrm) in enumerate(SPONZA):
        s.add_mesh(f"standin:sponza/{name}", pos if positions is None else positions[gi], nrm, engine.placement(), first + (gi % nmat))
        clock.ms["bvh"] += r.bvh_last_build_ms() if device_bvh else 0.0
    n1 = s.counts()["triPoints"]
    s.use_device_bvh(None)
    clock.lap("meshes")
    s.read_obj(os.path.join(engine.ASSET_DIR, "light2.obj"), engine.placement(position=(0, -1.5, 0), frontOnly=True), 3)
    clock.lap("setup")
    return s, (0, n1)


def deformed(groups, f):
    """The positions of every group passed through the field, made before any clock starts."""
    return [f(pos) for pos in groups]


def executed_box_tests_per_ray(pc):
    r.reset_counters()
    r.render(pc, W, H)
    c = r.counters()
    return (c["boxTests"] - c["skippedBoxTests"]) / max(c["raysTraced"], 1), c["raysTraced"]


def median_ms(call, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 4), round(min(t), 4)


results = []
for label, build, groups, pc in (("cornell + bunny", build_bunny, [BUNNY[0]], engine.push_constants(W, H, singleRender=1, sampleLimit=1)),
                                 ("sponza stand-in", build_sponza, [g[1] for g in SPONZA], scenes.sponza_camera(W, H, singleRender=1, sampleLimit=1))):
    base, (p0, p1) = build(None, False)
    pts0 = base.points()
    model = pts0[p0:p1, :3].astype(np.float64)
    extent, centre = float((model.max(0) - model.min(0)).max()), (model.max(0) + model.min(0)) / 2
    row = dict(scene=label, triangles=base.counts()["triangles"], points_updated=p1 - p0, meshes=len(set(base.numpy()["objects"].view(np.uint32).reshape(-1, 20)[:, 17].tolist())),
               runs=runs, rebuild_runs=REBUILDS, width=W, height=H)

    # ---- (a) update time
    fields = [field(extent, centre, 0.01, 1), field(extent, centre, 0.01, 2)]
    new = []
    for f in fields:
        p = pts0[p0:p1].copy()
        p[:, :3] = f(p[:, :3])
        new.append(p)
    r.upload_scene(base, dynamic=True)
    turn = [0]

    def update():
        r.update_points(new[turn[0] & 1], p0)
        turn[0] += 1

    for _ in range(3):
        update()
    row["update_points_ms"], row["update_points_ms_min"] = median_ms(update, runs)

    moved = [deformed(groups, f) for f in fields]
    shares = dict(setup=[], meshes=[], bvh=[], upload=[], rebuild=[])

    def rebuild():
        clock = Clock()
        s, _ = build(moved[turn[0] & 1], True, clock)
        turn[0] += 1
        t1 = time.perf_counter()
        r.upload_scene(s)
        upload = (time.perf_counter() - t1) * 1e3
        for k in ("setup", "meshes", "bvh"):
            shares[k].append(clock.ms[k])
        shares["upload"].append(upload)
        shares["rebuild"].append(clock.ms["meshes"] + upload)

    rebuild()
    shares = {k: [] for k in shares}
    for _ in range(REBUILDS):
        rebuild()
    med = lambda k: round(statistics.median(shares[k]), 4)   # noqa: E731
    row["rebuild_and_upload_ms"], row["rebuild_and_upload_ms_min"] = med("rebuild"), round(min(shares["rebuild"]), 4)
    row["of_it_meshes_added_with_rt_bvh_build_ms"] = med("meshes")
    row["of_it_rt_bvh_build_ms"] = med("bvh")
    row["of_it_rt_upload_scene_ms"] = med("upload")
    row["scene_setup_ms"] = med("setup")
    row["rebuild_over_update"] = round(row["rebuild_and_upload_ms"] / row["update_points_ms"], 1)

    # ---- (b) traversal cost after the update
    r.upload_scene(base)
    row["box_tests_per_ray_undeformed"] = round(executed_box_tests_per_ray(pc)[0], 3)
    for name, share in (("small", 0.01), ("large", 0.25)):
        f = field(extent, centre, share, 3)
        p = pts0[p0:p1].copy()
        p[:, :3] = f(p[:, :3])
        r.upload_scene(base, dynamic=True)
        r.update_points(p, p0)
        refit, rays = executed_box_tests_per_ray(pc)
        rebuilt_scene, _ = build(deformed(groups, f), True)
        r.upload_scene(rebuilt_scene)
        rebuilt, rays2 = executed_box_tests_per_ray(pc)
        row[f"{name}_displacement_share_of_extent"] = share
        row[f"{name}_box_tests_per_ray_refit"] = round(refit, 3)
        row[f"{name}_box_tests_per_ray_rebuilt"] = round(rebuilt, 3)
        row[f"{name}_refit_over_rebuilt"] = round(refit / rebuilt, 3)
        row[f"{name}_rays"] = [rays, rays2]
    print(json.dumps(row), flush=True)
    results.append(row)

with open(out, "w") as fh:
    json.dump(results, fh, indent=1)
    fh.write("\n")
print("wrote", out)
