"""TEST INFRASTRUCTURE — the scenes, the cameras and the float32 restatement `follow` of the mirror-following guide planes
(rt_render_guides; DESIGN.md, "Mirror-following guide planes"), shared by tests/test_guides.py (bit parity of the kernel with
`follow`) and tests/test_guides_float64.py (which holds `follow` and the kernel to tests/guides_float64.py).

`follow` restates the pass on the CPU: it chains the oracle's calculateIntersections (pyoracle.trace_rays) with the reflect and the
origin offset in numpy float32, in the kernel's order."""
import numpy as np

from oracle import pyoracle
from ray_tracer_amd import engine

from aov_cases import _albedos
from temporal_float64 import primary_dirs
from util import EditedScene, cornell_scene

MISS_DST = np.float32(99999999.0)   # RT_MISS_DST
MIRROR = 4                          # the built-in mirror material (reflectance 1)
HIT_FIELDS = ("dst", "didHit", "isSphere", "objectHitIndex", "triHitIndex", "materialIndex", "frontFace", "hitPoint", "normal")
COUNTERS = ("boxTests", "triTests", "raysTraced", "raysHit")
f32 = np.float32


# ---------------------------------------------------------------- the restatement
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _hit_uv(arr, hits, which):
    """hit.uv of the triangle hits `which`, on objects under the identity transform, in float64 from the hit point's barycentrics."""
    uv = np.full((len(hits["dst"]), 2), np.nan)
    for i in which:
        m = np.array(list(arr.objects[hits["objectHitIndex"][i]].transformMatrix)).reshape(4, 4)
        assert np.array_equal(m, np.eye(4)), "_hit_uv restates identity-placed objects only"
        t = arr.triangles[hits["triHitIndex"][i]]
        pts = [arr.triPoints[v] for v in (t.v0, t.v1, t.v2)]
        P = np.array([list(p.position)[:3] for p in pts], np.float64)
        T = np.array([[p.position[3], p.normal[3]] for p in pts], np.float64)
        e1, e2, q = P[1] - P[0], P[2] - P[0], hits["hitPoint"][i].astype(np.float64) - P[0]
        b1, b2 = np.linalg.lstsq(np.stack([e1, e2], 1), q, rcond=None)[0]
        uv[i] = (1.0 - b1 - b2) * T[0] + b1 * T[1] + b2 * T[2]
    return uv


def reflectance_of(scene, hits, textures):
    """What shade_path compares with 0 at each hit: the material's reflectance, or, on a triangle hit whose material binds a map of
    the table, the decoded red of the metalness texel at (u, 1 - v), which is 0 for byte 0 only. A hit within 1e-3 texels of a
    texel edge would make the restatement's float64 uv a guess: there must be none (the scenes are made so)."""
    arr = scene.arrays()
    mats = [arr.materials[i] for i in range(arr.materialCount)]
    r = np.array([mats[m].reflectance if h else 0.0 for m, h in zip(hits["materialIndex"], hits["didHit"])], np.float32)
    mapped = np.array([bool(h) and not s and 0 <= mats[m].metalnessIndex < len(textures)
                       for m, h, s in zip(hits["materialIndex"], hits["didHit"], hits["isSphere"])], bool)
    if mapped.any():
        uv = _hit_uv(arr, hits, np.flatnonzero(mapped))
        for i in np.flatnonzero(mapped):
            tex = textures[mats[hits["materialIndex"][i]].metalnessIndex]
            fu, fv = uv[i, 0] * tex.shape[1], (1.0 - uv[i, 1]) * tex.shape[0]
            assert 0.0 < uv[i, 0] < 1.0 and 0.0 < uv[i, 1] < 1.0, "uvs inside the unit square: both samplers agree"
            assert abs(fu - round(fu)) > 1e-3 and abs(fv - round(fv)) > 1e-3, (i, fu, fv)
            r[i] = 1.0 if tex[int(fv), int(fu), 0] != 0 else 0.0
    return r


def follow(scene, origins, dirs, max_bounces, textures=()):
    """The contract of rt_render_guides for the rays (origins, dirs), float32 [n, 3]: per ray the final segment's RtHit fields, its
    direction `rayDir`, the path length `depth`, `bounces` (L) and `cut`; `first`: segment 0's hits; `counters`: the four traversal
    counters summed over every ray of every chain."""
    o, d = np.array(origins, f32).reshape(-1, 3), np.array(dirs, f32).reshape(-1, 3)
    n = len(d)
    out = dict(dst=np.zeros(n, f32), didHit=np.zeros(n, np.uint32), isSphere=np.zeros(n, np.uint32), objectHitIndex=np.zeros(n, np.uint32),
               triHitIndex=np.zeros(n, np.uint32), materialIndex=np.zeros(n, np.uint32), frontFace=np.zeros(n, np.uint32),
               hitPoint=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32), rayDir=np.zeros((n, 3), f32), depth=np.zeros(n, f32),
               bounces=np.zeros(n, np.uint32), cut=np.zeros(n, bool))
    length = np.zeros(n, f32)
    alive = np.arange(n)
    counters = dict.fromkeys(COUNTERS, 0)
    first = None
    for j in range(max_bounces + 1):
        if not len(alive):
            break
        h = engine.hits_to_numpy(pyoracle.trace_rays(scene, o[alive], d[alive]))
        first = h if first is None else first
        counters["boxTests"] += int(h["boxTests"].sum()); counters["triTests"] += int(h["triTests"].sum())
        counters["raysTraced"] += len(alive); counters["raysHit"] += int(h["didHit"].sum())
        hit = h["didHit"] == 1
        mirror = hit & (reflectance_of(scene, h, textures) != 0)
        go = mirror & (j < max_bounces)
        end, idx = ~go, alive[~go]
        for k in HIT_FIELDS:
            out[k][idx] = h[k][end]
        out["rayDir"][idx] = d[idx]
        out["depth"][idx] = np.where(hit[end], length[idx] + h["dst"][end], h["dst"][end])   # ((d0 + d1) + d2) + ...; a miss: RT_MISS_DST
        out["bounces"][idx], out["cut"][idx] = j, mirror[end]
        c, nrm, rd = alive[go], h["normal"][go], d[alive[go]]
        length[c] = length[c] + h["dst"][go]
        k2 = f32(2) * _dot(nrm, rd)                                                        # rt_reflect: I - (2 dot(N, I)) N
        d[c] = rd - nrm * k2[:, None]
        o[c] = h["hitPoint"][go] + (nrm * f32(1)) * f32(0.00001)
        alive = c
    return dict(out, first=first, counters=counters)


HALL_CAMERA = dict(pos=(0.0, -1.0, -0.9), cameraAngles=(0.0, 80.0, 0.0), fov=40.0)   # inside the box, looking at the right wall


def hall_of_mirrors():
    """cornell_scene(True) with the red and the green wall turned into mirrors: chains bounce between them. Seen through HALL_CAMERA
    the rays near the walls' common normal go back and forth for more than eight segments, the others drift to the back wall, the
    floor or a sphere sooner."""
    ed = EditedScene(cornell_scene(True))
    walls = [i for i in range(ed.nObjects) if ed.objects[i].materialIndex in (1, 2)]
    assert len(walls) == 2
    for i in walls:
        ed.objects[i].materialIndex = MIRROR
    return ed


def metal_quad():
    """The Cornell box without spheres and a quad facing the camera whose material binds metalness map 0: a 2 x 2 map of which two
    texels decode to 0. The quad is off centre, so that no pixel's hit lies on a texel edge (reflectance_of asserts it)."""
    s = cornell_scene(False)
    m = s.add_material(engine.default_material(albedo=(0.75, 0.5, 0.25), metalnessIndex=0))
    x0, x1, y0, y1, z = -0.63, 0.57, -1.13, 0.07, 0.2
    P = np.array([[[x0, y0, z], [x1, y1, z], [x1, y0, z]], [[x0, y0, z], [x0, y1, z], [x1, y1, z]]], np.float32)   # wound to face the camera
    UV = np.stack([(P[..., 0] - x0) / (x1 - x0), (P[..., 1] - y0) / (y1 - y0)], -1).astype(np.float32)
    s.add_mesh("metal", P, np.tile(np.array([0, 0, -1], np.float32), (2, 3, 1)), engine.placement(), m, uvs=UV)
    tex = np.zeros((2, 2, 4), np.uint8)
    tex[..., 0] = [[0, 255], [90, 0]]
    tex[..., 1:] = (7, 201, 255)   # the other channels must not matter
    return s, m, [tex]


def camera_rays(pc, W, H):
    """The camera rays of a W x H frame for the CPU tests (float64 primary_dirs rounded to float32: within an ulp of the device's)."""
    d = primary_dirs(pc.camInfo, W, H).astype(f32).reshape(-1, 3)
    return np.tile(np.array(list(pc.camInfo.pos), f32), (len(d), 1)), d


def as_guides(ref, shape, scene):
    """follow()'s result as the dict Renderer.render_guides returns, (H, W[, 3]) arrays."""
    h = ref["didHit"] == 1
    none = np.uint32(0xFFFFFFFF)
    alb = np.where(h[:, None], _albedos(scene)[np.where(h, ref["materialIndex"], 0)], f32(0))
    g = dict(depth=ref["depth"], normal=ref["normal"], position=ref["hitPoint"], albedo=alb, ray_dir=ref["rayDir"],
             object=np.where(h, ref["objectHitIndex"], none), triangle=np.where(h, ref["triHitIndex"], none),
             material=np.where(h, ref["materialIndex"], none), hit=h, sphere=ref["isSphere"] == 1, front_face=ref["frontFace"] == 1,
             bounces=ref["bounces"], cut=ref["cut"])
    return {k: v.reshape(shape + v.shape[1:]) for k, v in g.items()}
