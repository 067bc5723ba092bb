"""Temporal accumulation (rt_temporal_accumulate; DESIGN.md, "Temporal accumulation") restated in numpy: `Restatement` keeps its own
history from call to call, in float64 (what the kernel is compared with) or float32 (what measures how far fp32 rounding alone
moves the result). With it: the synthetic planes, cameras and camera paths, the tolerances and the small plane helpers that
tests/test_temporal.py, tests/test_temporal_motion.py, tests/test_denoise.py and tests/test_guides.py share."""
import numpy as np

from ray_tracer_amd import engine


# |gpu - ref| <= T * max(|ref|, 1e-3), for rgba and for moments. T = 4 x the worst relative difference between the restatement run
# in float32 and in float64 on every input of the GPU tests of tests/test_temporal.py (the synthetic sequences of every size and camera path, and the
# rendered cornell_spheres and bunny sequences; `Checker` prints it beside every comparison), rounded up to one significant
# figure; the factor 4 is for the kernel's different but equally valid order of operations. The worst is always on the variance,
# max(0, m2 - m1^2): where a pixel's frames agree it is the difference of two numbers of magnitude l^2 that nearly cancel, so
# fp32 leaves it an absolute error of about 1e-7 l^2 whatever its own size. Measured worst T_MEASURED, hence T. The other
# channels (rgb, m1, m2, N) do not cancel, and the same measurement over them alone gives T_COLOUR_MEASURED and T_COLOUR, which
# this file holds them to as well: their worst comes from a point that lands within 1e-5 of a pixel of a tap's centre, where
# fp32 and float64 floor to different sides and a neighbour of very different colour enters or leaves with a weight of 1e-5.
# T_MEASURED is the synthetic sequences' (130 x 70; test_synthetic_sequences_are_rarely_fragile prints it per size, on the CPU;
# the rendered sequences reach 1.3e-3 there), T_COLOUR_MEASURED the rendered sequences' (both scenes; the synthetic ones reach
# 4.7e-4). `Checker` prints both distances beside every kernel comparison on a GPU run; on the run these were taken from, the
# kernel's own distances were the float32 restatement's to three digits, and at most 1.35 % of F was fragile in any call.
T_MEASURED, T = 7.7e-3, 4e-2
T_COLOUR_MEASURED, T_COLOUR = 1.12e-3, 5e-3
FRAGILE_CAP = 0.02   # fragile pixels (a hard decision of the contract within rounding of its threshold) are at most 2 % of F


# ---------------------------------------------------------------- the restatement
def filtered_set(ids, emission):
    """F: a hit (ids.w & 1) on a material index below the table's size whose emissionStrength is 0."""
    emission = np.asarray(emission, np.float64)
    m = ids[..., 2]
    ok = ((ids[..., 3] & 1) == 1) & (m < len(emission))
    return ok & (emission[np.where(ok, m, 0)] == 0.0)


def camera_of(ci, dt=np.float64):
    """frame_camera's view of a CameraInfo in `dt`: the rotation as M[row, column] (cameraRotation is column-major), the position,
    the plane's width and height and its bottom left corner, whose z is frame_camera's constant 0.1f."""
    f = dt
    m = np.array(list(ci.cameraRotation), np.float32).reshape(4, 4).T.astype(f)
    ph = f(np.float32(ci.nearPlane)) * np.tan(f(np.float32(ci.fov)) * f(0.5) * f(0.017453292519943295)) * f(2)
    pw = ph * f(np.float32(ci.aspectRatio))
    return dict(M=m[:3, :3], t=m[:3, 3], pos=np.array(list(ci.pos), np.float32).astype(f), pw=f(pw), ph=f(ph),
                bl=np.array([-pw / f(2), -ph / f(2), f(np.float32(0.1))], f))


def primary_dirs(ci, W, H):
    """primary_dir for every pixel, in float64: (H, W, 3) unit directions in the world. The plane's depth is camera_of's
    float32(0.1), the constant frame_camera hands the temporal kernels: brute_force.camera_dirs takes the double 0.1 instead."""
    c = camera_of(ci)
    gy, gx = np.mgrid[0:H, 0:W].astype(np.float64)
    pt = np.stack([c["bl"][0] + c["pw"] * (gx / W), c["bl"][1] + c["ph"] * (gy / H), np.full((H, W), c["bl"][2])], -1)
    d = pt / np.linalg.norm(pt, axis=-1, keepdims=True)
    return d @ c["M"].T + c["t"]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class Restatement:
    """The contract of rt_temporal_accumulate in numpy, in float64 (the reference) or float32 (the run that measures T). `step` takes
    the (H, W, 4) planes of one frame and the CameraInfo it was rendered with and returns the accumulated frame, the moments
    plane, F and the fragile pixels of this call; the history lives in the object."""

    def __init__(self, dt=np.float64):
        self.dt, self.hist = dt, None

    def reset(self):
        self.hist = None

    def step(self, ci, rgba, nd, position, albedo, ids, emission, max_history=32, normal_cos=0.9, depth_tolerance=0.02):
        f = self.dt
        H, W = rgba.shape[:2]
        F = filtered_set(ids, emission)
        d = np.maximum(albedo[..., :3].astype(f), f(np.float32(1e-3)))
        e = rgba[..., :3].astype(f) / d
        lum = (f(0.2126) * e[..., 0] + f(0.7152) * e[..., 1]) + f(0.0722) * e[..., 2]
        n, z, P = nd[..., :3].astype(f), nd[..., 3].astype(f), position[..., :3].astype(f)
        key = np.stack([ids[..., 0], (ids[..., 3] >> 1) & 1, ids[..., 2]], -1)
        N, eb, m1, m2 = np.ones((H, W), f), e.copy(), lum.copy(), lum * lum
        fragile = np.zeros((H, W), bool)
        h = self.hist
        if h is not None and h["N"].shape == (H, W):
            c = h["cam"]
            v = P - c["pos"]
            M = c["M"]   # q = M^T v
            q = [(M[0, k] * v[..., 0] + M[1, k] * v[..., 1]) + M[2, k] * v[..., 2] for k in range(3)]
            with np.errstate(all="ignore"):
                s = c["bl"][2] / q[2]
                fx = ((q[0] * s - c["bl"][0]) / c["pw"]) * f(W)
                fy = ((q[1] * s - c["bl"][1]) / c["ph"]) * f(H)
                ok = (q[2] > 0) & (fx >= -1) & (fx < W) & (fy >= -1) & (fy < H)
            fragile |= np.abs(q[2]) <= 1e-5
            fx, fy = np.where(ok, fx, f(0)), np.where(ok, fy, f(0))
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
            dist = np.sqrt(_dot(v, v))
            nc, tol = f(np.float32(normal_cos)), f(np.float32(depth_tolerance)) * dist
            S, sN, s1, s2, se = np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W, 3), f)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    cand = inside & (h["N"][cy, cx] > 0) & (h["key"][cy, cx] == key).all(-1)   # the taps a threshold decides
                    dn = _dot(n, h["n"][cy, cx])
                    res = np.abs(dist - h["z"][cy, cx])
                    valid = cand & (dn >= nc) & (res <= tol)
                    fragile |= cand & ((np.abs(dn - nc) <= 1e-4) | (np.abs(res - tol) <= 1e-4 * dist))
                    w = np.where(valid, (tx if i else f(1) - tx) * (ty if j else f(1) - ty), f(0))
                    S += w
                    se += w[..., None] * h["e"][cy, cx]
                    sN += w * h["N"][cy, cx]
                    s1 += w * h["m1"][cy, cx]
                    s2 += w * h["m2"][cy, cx]
            fragile |= ok & (np.abs(S - 1e-3) <= 1e-4)
            use = ok & (S >= f(np.float32(1e-3)))
            Ss = np.where(use, S, f(1))
            eh, Nh, h1, h2 = se / Ss[..., None], sN / Ss, s1 / Ss, s2 / Ss
            Nn = np.minimum(Nh + f(1), f(max_history))
            k = f(1) / Nn
            N = np.where(use, Nn, N)
            eb = np.where(use[..., None], eh + k[..., None] * (e - eh), eb)
            m1 = np.where(use, h1 + k * (lum - h1), m1)
            m2 = np.where(use, h2 + k * (lum * lum - h2), m2)
        out = rgba.astype(f)
        out[..., :3] = np.where(F[..., None], eb * d, out[..., :3])
        mom = np.where(F[..., None], np.stack([m1, m2, np.maximum(f(0), m2 - m1 * m1), N], -1), f(0))
        self.hist = dict(cam=camera_of(ci, f), e=eb, N=np.where(F, N, f(0)), m1=m1, m2=m2, n=n, z=z, key=key)
        return out, mom, F, fragile & F


def emission_of(scene):
    a = scene.arrays()
    return np.array([a.materials[i].emissionStrength for i in range(a.materialCount)], np.float64)


def rel(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), 1e-3)


def distances(got, mom, out, m, cmp):
    """Over the pixels `cmp`: the largest relative difference of (rgb, m1, m2, N) and of the variance."""
    if not cmp.any():
        return 0.0, 0.0
    colour = max(float(rel(got[cmp][:, :3], out[cmp][:, :3]).max()), float(rel(mom[cmp][:, [0, 1, 3]], m[cmp][:, [0, 1, 3]]).max()))
    return colour, float(rel(mom[cmp][:, 2], m[cmp][:, 2]).max())


# ---------------------------------------------------------------- synthetic planes: an analytic camera over planar patches
def synthetic(ci, W, H, emission, seed, dtype=np.float32):
    """First-hit planes of the surface |z| = 5 + max(x, 0) / 2 seen from the camera, computed in float64 from `primary_dirs` and
    rounded to `dtype` (float32 as the kernel gets them): four planar patches (two in front, two behind) with their own object, material and normal, a band of
    the second patch with the sphere bit, an emitter band above y = 0.5, misses left of x = -1.2, random triangle indices (never
    compared) and front-face bits, albedo with zeros, and a random frame whose demodulated colour is in [0, 2]."""
    rng = np.random.default_rng(seed)
    dark, light = np.flatnonzero(np.asarray(emission) == 0), int(np.argmax(emission))
    o = np.array(list(ci.pos), np.float32).astype(np.float64)
    D = primary_dirs(ci, W, H)
    sz = np.where(D[..., 2] >= 0, 1.0, -1.0)
    with np.errstate(all="ignore"):
        tA = (5.0 * sz - o[2]) / D[..., 2]
        tB = (5.0 - (sz * o[2] - 0.5 * o[0])) / (sz * D[..., 2] - 0.5 * D[..., 0])
    xA, xB = o[0] + tA * D[..., 0], o[0] + tB * D[..., 0]
    hitA, hitB = np.isfinite(tA) & (tA > 0) & (xA <= 0), np.isfinite(tB) & (tB > 0) & (xB > 0)
    hitB &= ~hitA
    t = np.where(hitA, tA, np.where(hitB, tB, 0.0))
    P = o + t[..., None] * D
    hit = (hitA | hitB) & (P[..., 0] >= -1.2)
    patch = np.where(hitA, 0, 1) + np.where(sz > 0, 0, 2)
    nB = np.array([0.5, 0.0, -1.0]) / np.sqrt(1.25)
    normal = np.where(hitA[..., None], np.array([0.0, 0.0, -1.0]), nB) * np.stack([np.ones_like(sz), np.ones_like(sz), sz], -1)
    nd, position, albedo = np.zeros((H, W, 4), dtype), np.zeros((H, W, 4), dtype), np.zeros((H, W, 4), np.float32)
    ids = np.zeros((H, W, 4), np.uint32)
    nd[..., :3], nd[..., 3] = np.where(hit[..., None], normal, 0.0), np.where(hit, t, 1e30)
    position[..., :3], position[..., 3] = np.where(hit[..., None], P, 0.0), hit
    a = rng.uniform(0.05, 1.0, (H, W, 3))
    a[rng.random((H, W)) < 0.05] = 0.0
    albedo[..., :3], albedo[..., 3] = np.where(hit[..., None], a, 0.0), hit
    ids[..., 0] = np.where(hit, patch, 0xFFFFFFFF)
    ids[..., 1] = np.where(hit, rng.integers(0, 1000, (H, W)), 0xFFFFFFFF)
    ids[..., 2] = np.where(hit, np.where(P[..., 1] > 0.5, light, dark[patch % len(dark)]), 0xFFFFFFFF)
    ids[..., 3] = np.where(hit, 1 | (((patch % 2 == 1) & (P[..., 0] > 0.8)) << 1) | (rng.integers(0, 2, (H, W)) << 2), 0)
    return nd, position, albedo, ids


def synthetic_frame(albedo, seed):
    """A noisy frame over the planes: rgb = e * max(albedo, 1e-3) with e uniform in [0, 2], any alpha."""
    rng = np.random.default_rng(seed)
    H, W = albedo.shape[:2]
    rgba = rng.random((H, W, 4)).astype(np.float32)
    rgba[..., :3] = (rng.uniform(0.0, 2.0, (H, W, 3)) * np.maximum(albedo[..., :3].astype(np.float64), 1e-3)).astype(np.float32)
    return rgba


def cam(W, H, yaw=0.0, pos=(0.0, 0.0, 0.0), pitch=0.0):
    """The synthetic tests' camera: 20 degrees of vertical field of view and at most twice that across, so that even at 37 x 23
    a pixel's step in depth along the patches stays well inside the default depth tolerance (at the default 50 degrees it is
    not, and a large part of a small image sits near that threshold)."""
    return engine.push_constants(W, H, cameraAngles=(pitch, yaw, 0.0), pos=pos, fov=20.0, aspectRatio=min(W / H, 2.0)).camInfo


def pixel_yaw(W, H, px):
    """The yaw, in degrees, that moves the image's centre column by `px` pixels."""
    c = camera_of(cam(W, H))
    return float(np.degrees(np.arctan(px * c["pw"] / W / c["bl"][2])))


def paths(W, H):
    """The camera sequences of the synthetic test: four cameras each."""
    sub = pixel_yaw(W, H, 0.37)
    return {
        "unchanged": [cam(W, H, 3.0, (0.1, 0.05, 0.0), 2.0)] * 4,
        "subpixel_pan": [cam(W, H, k * sub) for k in range(4)],
        "yaw_2deg": [cam(W, H, 2.0 * k) for k in range(4)],
        "dolly": [cam(W, H, 1.0, (0.0, 0.0, 0.25 * k)) for k in range(4)],
        "jump": [cam(W, H, 0.0), cam(W, H, 0.0), cam(W, H, 180.0), cam(W, H, 180.0)],
    }


EMISSION_TOY = np.array([0.0, 0.0, 5.0, 0.0])


def planes_of(a):
    p = engine.numpy_to_aovs(a)
    return p["normalDepth"], p["position"], p["albedo"], p["ids"]


def camera_path(W, H, k, **params):
    """Frame k of the rendered tests' path: a small yaw plus a translation, non-progressive, consecutive frameCounts."""
    return engine.push_constants(W, H, cameraAngles=(4.0, 0.6 * k, 0.0), pos=(0.02 * k, -0.5, -3.5 + 0.03 * k), progressive=0,
                                 frameCount=k, **params)
