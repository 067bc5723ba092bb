"""Temporal accumulation that follows moved objects and spheres (rt_temporal_track_motion, rt_temporal_motion_state,
k_tp_accumulate_motion, Renderer.temporal_track_motion, InteractiveSession(track_motion=True)).

The contract is DESIGN.md's "Temporal accumulation" with the addition "Moved objects and spheres": a pixel of F on a moved object
sends P~ = D P and n~ = G n / |G n| through the previous camera and the tap tests in place of P and n, one on a moved sphere
P~ = c' + (P - c) r' / r, one on a replaced object or sphere has no history, and what is stored is the frame's own n, z and ids.
`MotionRestatement` restates that in numpy on top of tests/temporal_float64.py's `Restatement` (which is imported, not edited); it
computes D = Fwd' Inv and G = Inv'^T Fwd^T itself from the fp32 transformMatrix of the two calls (float64: numpy's float64 inverse;
float32: numpy's float32 inverse and products rounded once to fp32, as the library's tables are) and takes nothing from the library.

Inputs. `moved_planes` is `synthetic`'s surface with each of the four patches under its own object matrix and the sphere-bit
bands of patches 1 and 3 under the similarity of spheres 1 and 3: every pixel's ray is taken into the body's own space, intersected
there with the patch, and the nearest body wins, so the planes are those of a real scene and taps do match. The *duality*
sequences take each camera path of `paths(W, H)` and express its planes in camera 0's frame: the camera stays fixed and all four
patches carry the rigid transform that undoes camera k (sphere bits cleared, a sphere cannot turn). The *mixed* sequence moves
patches 0 (rotating, translating and stretching unequally, so G is not D's linear part) and 2, leaves patch 1, re-points patch 3
once, and lets both bands translate and grow; it runs once with a camera that sees patches 0 and 1 and once with one that looks
the other way and sees patches 2 and 3 (no 20-degree camera sees all four).

Tolerances. The rule is tests/test_temporal.py's: T and T_COLOUR are 4 x the worst distance of the float32 restatement from the
float64 one over every input of the GPU tests, rounded up to one significant figure, and where that worst is at or below the
existing file's T_MEASURED / T_COLOUR_MEASURED the existing T / T_COLOUR are used. `MotionChecker` prints both distances beside
every comparison; test_sequences_are_rarely_fragile prints the synthetic ones per size, on the CPU. Measured:
  synthetic (duality and mixed, all sizes): colour 4.7e-4 (at or below the existing 1.12e-3: T_COLOUR stays 5e-3), variance 7.93e-3
  at 130 x 70 (above the existing 7.7e-3; 4 x 7.93e-3 = 3.2e-2 rounds up to the same T = 4e-2); no pixel of them is fragile.
  rendered, moving camera (cornell_spheres and bunny): colour 2.05e-3, variance 2.67e-3. The colour is above the existing 1.12e-3:
  4 x 2.05e-3 = 8.2e-3, so T_COLOUR_RENDERED = 9e-3; the variance is below the existing 7.7e-3: T = 4e-2.
  rendered, fixed camera: colour 5.01e-2 (bunny), variance 1.29e-1 (cornell_spheres): 4 x gives 2.004e-1 and 5.2e-1, hence
  T_COLOUR_FIXED = 3e-1 and T_FIXED = 6e-1. A camera that does not move is the worst input this pass has: every pixel that did not
  move lands within 1e-5 of a pixel of its own centre, fp32 and float64 floor fx to different sides, and a neighbour enters or
  leaves with a weight of 1e-5 (the static file's "unchanged" path, where a neighbour is at most 50 x brighter). In a 1-spp render a
  neighbour's demodulated colour is up to several thousand times the pixel's own (a firefly beside a dark pixel, an albedo near
  0), and 1e-5 of that is the 5e-2; the variance, a difference of squares, takes it twice. The issue asks for these sequences and
  sets the rule, so the bound is what the rule gives; the moving-camera and synthetic sequences keep the tight ones.
On the GPU run these were taken from, the kernel's own distances equalled the float32 restatement's to the three digits printed
in every call but one (bunny, moving, call 1: 8.6e-4 against 5.7e-4), and at most 3 of 19 200 pixels were fragile in a call.
Fragile share. The rendered sequences use a 20-degree camera like the synthetic ones: at the default 50 degrees a fixed camera
made 2.5 % to 2.9 % of F fragile in every call (the depth step from one pixel to the next on the floor and the ceiling is itself
about depthTolerance, and with a fixed camera all four taps of every pixel are candidates), above the 2 % cap; at 20 degrees
the worst call has 0.02 %. (Figures at 50 degrees: the CPU oracle's frames and oracle_trace_rays planes, which reproduce a GPU run's.)
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, devmem, engine, session

from temporal_float64 import (EMISSION_TOY, FRAGILE_CAP, Restatement, T, T_COLOUR, T_COLOUR_MEASURED, T_MEASURED, cam, camera_of, distances, emission_of, filtered_set,
                              paths, planes_of, primary_dirs, rel, synthetic)
from util import EditedScene, cornell_scene, model_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# worst relative distance of the float32 restatement from the float64 one: (colour, variance)
MOTION_MEASURED_SYNTHETIC = (4.7e-4, 7.93e-3)
MOTION_MEASURED_RENDERED = (2.05e-3, 2.67e-3)          # moving camera
MOTION_MEASURED_RENDERED_FIXED = (5.01e-2, 1.29e-1)    # fixed camera
MOTION_T_COLOUR, MOTION_T = T_COLOUR, T                # synthetic
MOTION_T_COLOUR_RENDERED = 9e-3
MOTION_T_COLOUR_FIXED, MOTION_T_FIXED = 3e-1, 6e-1
RENDERED_FOV = 20.0
SIZES = [(1, 1), (67, 1), (1, 67), (37, 23), (130, 70)]


# ---------------------------------------------------------------- placements and the motion between two of them
def placements(objects, n_objects, spheres, n_spheres):
    """The placements of a scene's arrays: M (n, 4, 4) fp32 with M[row, column] (transformMatrix is column-major), bvhIndex, and
    the spheres' (centre, radius) rows."""
    M = np.array([np.array(list(objects[i].transformMatrix), np.float32).reshape(4, 4).T for i in range(n_objects)], np.float32).reshape(-1, 4, 4)
    bvh = np.array([objects[i].bvhIndex for i in range(n_objects)], np.uint32)
    S = np.array([list(spheres[i].position) + [spheres[i].radius] for i in range(n_spheres)], np.float32).reshape(-1, 4)
    return dict(M=M, bvh=bvh, S=S)


def placements_of(e):
    """Of an EditedScene or a session's edited arrays."""
    return placements(e.objects, e.nObjects, e.spheres, e.nSpheres)


def motion_matrices(Mp, Mn, dt):
    """D = Fwd' Inv (rows 0..2, previous-from-current) and G = Inv'^T Fwd^T (3 x 3) of the matrices of the previous call and of
    this one, in `dt`. float32: the inverse in float32 and each product accumulated in float64 and rounded once, as the library's
    tables are made (its inverse is rt_mat4_inverse's, which differs from numpy's by rounding: part of T)."""
    if dt == np.float64:
        Fp, Fn = np.asarray(Mp, np.float64), np.asarray(Mn, np.float64)
        Ip, In = np.linalg.inv(Fp), np.linalg.inv(Fn)
        return (Fp @ In)[:3], Ip[:3, :3].T @ Fn[:3, :3].T
    Ip, In = np.linalg.inv(np.asarray(Mp, np.float32)).astype(np.float64), np.linalg.inv(np.asarray(Mn, np.float32)).astype(np.float64)
    Ip[3], In[3] = (0, 0, 0, 1), (0, 0, 0, 1)
    Fp, Fn = np.asarray(Mp, np.float64), np.asarray(Mn, np.float64)
    return (Fp @ In)[:3].astype(np.float32), (Ip[:3, :3].T @ Fn[:3, :3].T).astype(np.float32)


def motion_of(prev, now, dt):
    """What the contract makes of two placements: per moved object (D, G), per moved sphere (c, r' / r, c'), None for a replaced
    one, nothing for an unmoved one; and the three numbers rt_temporal_motion_state reports."""
    objects, spheres = {}, {}
    for o in range(len(now["M"])):
        if o >= len(prev["M"]) or prev["bvh"][o] != now["bvh"][o]:
            objects[o] = None
        elif not np.array_equal(prev["M"][o].view(np.uint32), now["M"][o].view(np.uint32)):
            objects[o] = motion_matrices(prev["M"][o], now["M"][o], dt)
    for s in range(len(now["S"])):
        if s >= len(prev["S"]):
            spheres[s] = None
        elif not np.array_equal(prev["S"][s].view(np.uint32), now["S"][s].view(np.uint32)):
            c, cp = now["S"][s], prev["S"][s]
            ratio = np.float64(cp[3]) / np.float64(c[3])
            spheres[s] = (c[:3].astype(dt), dt(np.float32(ratio)) if dt == np.float32 else ratio, cp[:3].astype(dt))
    replaced = sum(v is None for v in objects.values()) + max(0, len(prev["M"]) - len(now["M"]))
    state = dict(movedObjects=sum(v is not None for v in objects.values()), replacedObjects=replaced,
                 movedSpheres=len(spheres) + max(0, len(prev["S"]) - len(now["S"])))
    return dict(objects=objects, spheres=spheres, counts=(len(now["M"]), len(now["S"])), state=state)


NO_MOTION = dict(movedObjects=0, replacedObjects=0, movedSpheres=0)


class MotionRestatement(Restatement):
    """The extended contract: `Restatement` with (P~, n~) in place of (P, n) in steps 2 and 3 and the frame's own n stored."""

    def step(self, ci, rgba, nd, position, albedo, ids, emission, motion=None, **kw):
        f = self.dt
        P, n = position[..., :3].astype(f), nd[..., :3].astype(f)
        Pt, nt = P.copy(), n.copy()
        if motion is not None and self.hist is not None:
            hit, sphere = (ids[..., 3] & 1) == 1, ((ids[..., 3] >> 1) & 1) == 1
            nobj, nsph = motion["counts"]
            Pt[hit & np.where(sphere, ids[..., 0] >= nsph, ids[..., 0] >= nobj)] = np.nan   # an index past the count: replaced
            for o, m in motion["objects"].items():
                sel = hit & ~sphere & (ids[..., 0] == o)
                if m is None:
                    Pt[sel] = np.nan        # replaced: no point goes through the previous camera, N = 1
                    continue
                D, G = (np.asarray(a, f) for a in m)
                x, v = P[sel], n[sel]
                Pt[sel] = np.stack([((D[k, 0] * x[:, 0] + D[k, 1] * x[:, 1]) + D[k, 2] * x[:, 2]) + D[k, 3] for k in range(3)], -1)
                g = np.stack([(G[k, 0] * v[:, 0] + G[k, 1] * v[:, 1]) + G[k, 2] * v[:, 2] for k in range(3)], -1)
                nt[sel] = g / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]
            for s, m in motion["spheres"].items():
                sel = hit & sphere & (ids[..., 0] == s)
                if m is None:
                    Pt[sel] = np.nan
                    continue
                c, ratio, cp = m
                Pt[sel] = cp + (P[sel] - c) * f(ratio)
        nd2, pos2 = nd.astype(f), position.astype(f)
        nd2[..., :3], pos2[..., :3] = nt, Pt
        with np.errstate(invalid="ignore"):
            out = super().step(ci, rgba, nd2, pos2, albedo, ids, emission, **kw)
        self.hist["n"] = n
        return out


def med(x):
    """The median, rounded to 1e-3: a weighted mean of equal history lengths may come out an ulp off."""
    return round(float(np.median(x)), 3)


class MotionChecker:
    """One sequence: every call's result against the float64 motion restatement, and the float32 one beside it."""

    def __init__(self, emission, what, t_colour=MOTION_T_COLOUR, t=MOTION_T):
        self.emission, self.what, self.t_colour, self.t = emission, what, t_colour, t
        self.ref, self.f32 = MotionRestatement(np.float64), MotionRestatement(np.float32)
        self.worst_gpu, self.worst_f32, self.worst_fragile = [0.0, 0.0], [0.0, 0.0], 0.0
        self.prev = None

    def reset(self):
        self.ref.reset()
        self.f32.reset()
        self.prev = None

    def restate(self, ci, planes, now, **kw):
        """Both restatements of one call whose placements are `now`; returns the float64 one's (out, moments, F, fragile) and
        the state rt_temporal_motion_state is to report."""
        m64 = motion_of(self.prev, now, np.float64) if self.prev is not None else None
        m32 = motion_of(self.prev, now, np.float32) if self.prev is not None else None
        self.prev = now
        out, m, F, fragile = self.ref.step(ci, *planes, self.emission, motion=m64, **kw)
        o32, mm32, _, _ = self.f32.step(ci, *planes, self.emission, motion=m32, **kw)
        if F.any():
            self.worst_fragile = max(self.worst_fragile, float(fragile.sum()) / float(F.sum()))
        self.worst_f32 = [max(a, b) for a, b in zip(self.worst_f32, distances(o32, mm32, out, m, F & ~fragile))]
        return (out, m, F, fragile), (m64["state"] if m64 is not None else NO_MOTION)

    def check(self, ci, planes, now, got, mom, **kw):
        rgba = planes[0]
        (out, m, F, fragile), state = self.restate(ci, planes, now, **kw)
        cmp = F & ~fragile
        print(f"{self.what}: F {int(F.sum())}, fragile {int(fragile.sum())}, float32 restatement worst: colour {self.worst_f32[0]:.3g} "
              f"variance {self.worst_f32[1]:.3g}", end="")
        assert got.dtype == np.float32 and got.shape == rgba.shape and mom.shape == rgba.shape, self.what
        assert np.array_equal(got[~F].view(np.uint32), rgba[~F].view(np.uint32)), self.what      # kept pixels bit for bit
        assert not mom[~F].view(np.uint32).any(), self.what
        assert np.array_equal(got[F][:, 3].view(np.uint32), rgba[F][:, 3].view(np.uint32)), self.what
        assert np.isfinite(got[F]).all() and np.isfinite(mom[F]).all(), self.what
        now_d = distances(got, mom, out, m, cmp)
        self.worst_gpu = [max(a, b) for a, b in zip(self.worst_gpu, now_d)]
        print(f"; kernel worst: colour {self.worst_gpu[0]:.3g} variance {self.worst_gpu[1]:.3g}")
        assert now_d[0] <= self.t_colour, (self.what, "rgb, m1, m2, N", now_d[0], self.t_colour)
        assert max(now_d) <= self.t, (self.what, "variance", now_d[1], self.t)
        assert self.worst_fragile <= FRAGILE_CAP, (self.what, self.worst_fragile)
        return (out, m, F, fragile), state


# ---------------------------------------------------------------- synthetic planes of moved bodies
SPHERE_BASE = {1: np.array([2.0, 0.0, 6.0, 1.0], np.float32), 3: np.array([2.0, 0.0, -6.0, 1.0], np.float32)}   # bands' own space


def sphere_affine(s, base):
    """The similarity a sphere-bit band follows: X = c + (r / r0) (X0 - c0)."""
    A = np.eye(4)
    k = np.float64(s[3]) / np.float64(base[3])
    A[:3, :3] *= k
    A[:3, 3] = s[:3].astype(np.float64) - k * base[:3].astype(np.float64)
    return A


def moved_planes(ci, W, H, emission, seed, now):
    """`synthetic`'s planes with patch o under now["M"][o] and the band of patch 1 / 3 under sphere 1 / 3 (module docstring).
    Geometry in float64 from the fp32 placements, rounded to fp32; albedo, triangle indices and front-face bits random."""
    rng = np.random.default_rng(seed)
    dark, light = np.flatnonzero(np.asarray(emission) == 0), int(np.argmax(emission))
    o = np.array(list(ci.pos), np.float32).astype(np.float64)
    Dw = primary_dirs(ci, W, H)
    best = np.full((H, W), np.inf)
    patch_of, band_of, light_of = np.zeros((H, W), np.int64), np.zeros((H, W), bool), np.zeros((H, W), bool)
    normal = np.zeros((H, W, 3))
    nB = np.array([0.5, 0.0, -1.0]) / np.sqrt(1.25)
    bodies = [(p, False, now["M"][p].astype(np.float64)) for p in range(4)] + [(p, True, sphere_affine(now["S"][p], SPHERE_BASE[p])) for p in (1, 3)]
    for p, band, A in bodies:
        Ai = np.linalg.inv(A)
        oo, d = Ai[:3, :3] @ o + Ai[:3, 3], Dw @ Ai[:3, :3].T
        sz = 1.0 if p < 2 else -1.0
        with np.errstate(all="ignore"):
            t = (5.0 * sz - oo[2]) / d[..., 2] if p % 2 == 0 else (5.0 - (sz * oo[2] - 0.5 * oo[0])) / (sz * d[..., 2] - 0.5 * d[..., 0])
        ok = np.isfinite(t) & (t > 0)
        P = oo + np.where(ok, t, 0.0)[..., None] * d
        ok &= (P[..., 0] <= 0) if p % 2 == 0 else (P[..., 0] > 0)
        ok &= P[..., 0] >= -1.2
        ok &= ((P[..., 0] > 0.8) == band) if p % 2 == 1 else True
        ok &= t < best
        n_obj = np.array([0.0, 0.0, -sz]) if p % 2 == 0 else nB * np.array([1.0, 1.0, sz])
        n_w = n_obj @ Ai[:3, :3]                      # A^-T n
        best = np.where(ok, t, best)
        patch_of, band_of, light_of = np.where(ok, p, patch_of), np.where(ok, band, band_of), np.where(ok, P[..., 1] > 0.5, light_of)
        normal = np.where(ok[..., None], n_w / np.linalg.norm(n_w), normal)
    hit = np.isfinite(best)
    t = np.where(hit, best, 0.0)
    Pw = o + t[..., None] * Dw
    nd, position, albedo = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    ids = np.zeros((H, W, 4), np.uint32)
    nd[..., :3], nd[..., 3] = np.where(hit[..., None], normal, 0.0), np.where(hit, t, 1e30)
    position[..., :3], position[..., 3] = np.where(hit[..., None], Pw, 0.0), hit
    a = rng.uniform(0.05, 1.0, (H, W, 3))
    a[rng.random((H, W)) < 0.05] = 0.0
    albedo[..., :3], albedo[..., 3] = np.where(hit[..., None], a, 0.0), hit
    ids[..., 0] = np.where(hit, patch_of, 0xFFFFFFFF)
    ids[..., 1] = np.where(hit, rng.integers(0, 1000, (H, W)), 0xFFFFFFFF)
    ids[..., 2] = np.where(hit, np.where(light_of, light, dark[patch_of % len(dark)]), 0xFFFFFFFF)
    ids[..., 3] = np.where(hit, 1 | (band_of.astype(np.int64) << 1) | (rng.integers(0, 2, (H, W)) << 2), 0)
    return nd, position, albedo, ids


def frame_over(albedo, seed):
    """A noisy frame over the planes: rgb = e max(albedo, 1e-3) with e uniform in [0, 2], any alpha."""
    rng = np.random.default_rng(seed)
    H, W = albedo.shape[:2]
    rgba = rng.random((H, W, 4)).astype(np.float32)
    rgba[..., :3] = (rng.uniform(0.0, 2.0, (H, W, 3)) * np.maximum(albedo[..., :3].astype(np.float64), 1e-3)).astype(np.float32)
    return rgba


def matrix_of(**placement):
    """T Rx Ry Rz S of a placement as the library makes it (rt_transform_matrix): fp32, M[row, column]."""
    out = (C.c_float * 16)()
    _capi.lib().rt_transform_matrix(C.byref(engine.placement(**placement)), out)
    return np.array(list(out), np.float32).reshape(4, 4).T


BASE_BVH = np.array([0, 0, 7, 12], np.uint32)   # the roots Cornell's first four objects point at; 13 is another mesh's


def start_placements():
    return dict(M=np.stack([np.eye(4, dtype=np.float32)] * 4), bvh=BASE_BVH.copy(),
                S=np.stack([np.zeros(4, np.float32), SPHERE_BASE[1], np.zeros(4, np.float32), SPHERE_BASE[3]]))


def mixed_sequence(W, H, yaw):
    """Six calls with one camera (yaw 3 sees patches 0 and 1, yaw 183 patches 2 and 3): (camera, placements) each. Patch 0 turns about y, shifts and stretches unequally, patch 2 turns
    about x and shifts, patch 1 stays, patch 3 points at another mesh from call 3 on (replaced in that call alone), the two
    bands translate and grow. The steps are a fraction of a 37 x 23 pixel (0.076 at the patches' distance)."""
    ci = cam(W, H, yaw, (0.1, 0.05, 0.0), 2.0)
    seq = []
    for k in range(6):
        now = start_placements()
        now["M"][0] = matrix_of(position=(0.01 * k, 0.0, 0.02 * k), rotation=(0.0, 0.4 * k, 0.0), scale=(1.0 + 0.01 * k, 1.0, 1.0 - 0.005 * k))
        now["M"][2] = matrix_of(position=(-0.015 * k, 0.01 * k, 0.0), rotation=(0.3 * k, 0.0, 0.0))
        if k >= 3:
            now["bvh"][3] = 13
        now["S"][1] = SPHERE_BASE[1] + np.array([0.01 * k, 0.005 * k, 0.0, 0.01 * k], np.float32)
        now["S"][3] = SPHERE_BASE[3] + np.array([0.0, -0.01 * k, 0.01 * k, 0.02 * k], np.float32)
        seq.append((ci, now))
    return seq


def undo_camera(c0, ck):
    """T with M0^T (T X - pos0) = Mk^T (X - posk): what camera k sees at a pixel, camera 0 sees there after T. float64, 4 x 4."""
    L = np.linalg.inv(c0["M"].T) @ ck["M"].T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = L, c0["pos"] - L @ ck["pos"]
    return T


def carried(planes, A):
    """Planes whose points and normals went through the affine A (float64 in, float64 out; depth and ids kept), sphere bits
    cleared."""
    nd, position, albedo, ids = planes
    nd2, pos2, ids2 = nd.astype(np.float64), position.astype(np.float64), ids.copy()
    hit = (ids[..., 3] & 1) == 1
    pos2[..., :3] = np.where(hit[..., None], position[..., :3].astype(np.float64) @ A[:3, :3].T + A[:3, 3], 0.0)
    g = nd[..., :3].astype(np.float64) @ np.linalg.inv(A[:3, :3])       # A^-T n
    nd2[..., :3] = np.where(hit[..., None], g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-300), 0.0)
    ids2[..., 3] &= ~np.uint32(2)
    return nd2, pos2, albedo, ids2


def duality_sequence(W, H, name, emission):
    """The camera path `name` of paths(W, H) seen from its camera 0: per call (camera 0, placements, fp32 planes, frame). The four
    patches carry fp32(T_k), and the planes are made with that fp32 matrix."""
    cams = paths(W, H)[name]
    c0 = camera_of(cams[0])
    seq = []
    for k, ci in enumerate(cams):
        now = start_placements()
        A = undo_camera(c0, camera_of(ci)).astype(np.float32)
        now["M"][:] = A
        nd, position, albedo, ids = carried(synthetic(ci, W, H, emission, 100 * k + W), A.astype(np.float64))
        planes = (nd.astype(np.float32), position.astype(np.float32), albedo, ids)
        seq.append((cams[0], now, planes, frame_over(albedo, 7 * k + H)))
    return seq


def gpu_sequences(W, H, emission):
    """Every synthetic sequence of the GPU test: name -> [(camera, placements, planes, frame)]."""
    out = {"duality_" + name: duality_sequence(W, H, name, emission) for name in paths(W, H)}
    for name, yaw in (("mixed_front", 3.0), ("mixed_back", 183.0)):
        out[name] = []
        for k, (ci, now) in enumerate(mixed_sequence(W, H, yaw)):
            planes = moved_planes(ci, W, H, emission, 300 * k + W, now)
            out[name].append((ci, now, planes, frame_over(planes[2], 11 * k + H)))
    return out


# ---------------------------------------------------------------- CPU
def test_the_interface_is_there():
    for name in ("rt_temporal_track_motion", "rt_temporal_motion_state"):
        assert name in _capi.SYMBOLS
        assert name in open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert hasattr(engine.Renderer, "temporal_track_motion") and hasattr(engine.Renderer, "temporal_motion_state")
    p = inspect.signature(session.InteractiveSession.__init__).parameters
    assert p["track_motion"].default is False
    assert _capi.lib().rt_temporal_track_motion(None, 1) == -1
    assert _capi.lib().rt_temporal_motion_state(None, None, None, None) == -1


def test_moved_planes_with_nothing_moved_are_synthetic():
    """The generator's geometry is `synthetic`'s when every body is where `synthetic` has it."""
    W, H = 37, 23
    for ci in (cam(W, H, 3.0, (0.1, 0.05, 0.0), 2.0), cam(W, H, 178.0, (0.0, 0.1, 0.2))):
        a, b = synthetic(ci, W, H, EMISSION_TOY, 1), moved_planes(ci, W, H, EMISSION_TOY, 1, start_placements())
        assert (a[3][..., 3] & 1).sum() > 300
        np.testing.assert_allclose(b[0], a[0], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(b[1], a[1], rtol=1e-6, atol=1e-6)
        assert np.array_equal(a[3][..., [0, 2]], b[3][..., [0, 2]]) and np.array_equal(a[3][..., 3] & 3, b[3][..., 3] & 3)


def test_motion_restatement_without_motion_is_the_restatement():
    W, H = 37, 23
    a, b = Restatement(), MotionRestatement()
    for k, ci in enumerate(paths(W, H)["yaw_2deg"]):
        planes = synthetic(ci, W, H, EMISSION_TOY, k)
        rgba = frame_over(planes[2], k)
        ra, rb = a.step(ci, rgba, *planes, EMISSION_TOY), b.step(ci, rgba, *planes, EMISSION_TOY, motion=motion_of(start_placements(), start_placements(), np.float64))
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)


def test_a_translated_sphere_and_a_replaced_object():
    """By hand: a band that moved with its sphere keeps N, the same planes without the motion lose it where the shift exceeds the
    depth test or lands elsewhere; a replaced object starts at N = 1."""
    W, H = 67, 41
    ci = cam(W, H, 3.0, (0.1, 0.05, 0.0), 2.0)
    a, b = start_placements(), start_placements()
    b["S"][1] = SPHERE_BASE[1] + np.array([0.3, 0.0, 0.4, 0.0], np.float32)
    b["bvh"][2] = 13
    pa, pb = moved_planes(ci, W, H, EMISSION_TOY, 1, a), moved_planes(ci, W, H, EMISSION_TOY, 2, b)
    r = MotionRestatement()
    r.step(ci, frame_over(pa[2], 1), *pa, EMISSION_TOY)
    m = motion_of(a, b, np.float64)
    assert m["state"] == dict(movedObjects=0, replacedObjects=1, movedSpheres=1)
    out, mom, F, fragile = r.step(ci, frame_over(pb[2], 2), *pb, EMISSION_TOY, motion=m)
    ids = pb[3]
    band = F & ((ids[..., 3] & 2) == 2) & (ids[..., 0] == 1)
    assert band.sum() > 20 and med(mom[band][:, 3]) == 2.0
    gone = F & ((ids[..., 3] & 2) == 0) & (ids[..., 0] == 2)
    still = F & ((ids[..., 3] & 2) == 0) & (ids[..., 0] == 0)
    assert (mom[gone][:, 3] == 1.0).all() and (mom[still & ~fragile][:, 3] == 2.0).all()
    r2 = MotionRestatement()
    r2.step(ci, frame_over(pa[2], 1), *pa, EMISSION_TOY)
    _, mom2, _, _ = r2.step(ci, frame_over(pb[2], 2), *pb, EMISSION_TOY)
    assert med(mom2[band][:, 3]) == 1.0      # 0.4 of 6 in depth: beyond the 2 % tolerance


@pytest.mark.parametrize("W,H", [(37, 23), (130, 70)])
def test_duality_with_a_moving_camera(W, H):
    """Each camera path of paths(W, H), its planes expressed in camera 0's frame: the camera stays fixed and all four patches
    carry T_k, the rigid transform that undoes camera k. The motion restatement in float64 reproduces the static restatement of
    the original sequence on every non-fragile pixel of F to 1e-9 relative: it is the same arithmetic up to one float64 matrix
    product. T_k stays float64 here (rounded to fp32 it would no longer undo an fp32 camera to better than 1e-7); the GPU test
    runs the same sequences with fp32 matrices and planes made with them. ||T P - o'|| differs from ||P - o'_k|| by the 1e-7
    the fp32 camera rotations are off orthonormal, which can only move a depth or normal decision: such pixels are fragile."""
    for name, cams in paths(W, H).items():
        ref, mot = Restatement(), MotionRestatement()
        c0 = camera_of(cams[0])
        prev = None
        for k, ci in enumerate(cams):
            base = synthetic(ci, W, H, EMISSION_TOY, 100 * k + W)
            base[3][..., 3] &= ~np.uint32(2)
            rgba = frame_over(base[2], 7 * k + H)
            T = undo_camera(c0, camera_of(ci))
            motion = None
            if prev is not None:
                D, G = (prev @ np.linalg.inv(T))[:3], np.linalg.inv(prev)[:3, :3].T @ T[:3, :3].T
                same = np.array_equal(prev, T)
                motion = dict(objects={} if same else {o: (D, G) for o in range(4)}, spheres={}, counts=(4, 4))
            prev = T
            out, mom, F, fragile = ref.step(ci, rgba, *base, EMISSION_TOY)
            o2, m2, F2, fragile2 = mot.step(cams[0], rgba, *carried(base, T), EMISSION_TOY, motion=motion)
            assert np.array_equal(F, F2) and F.sum() > 100
            ok = F & ~fragile & ~fragile2
            assert ok.sum() >= 0.97 * F.sum(), (name, k)
            assert float(rel(o2[ok], out[ok]).max()) <= 1e-9 and float(rel(m2[ok], mom[ok]).max()) <= 1e-9, (name, k)
            if name != "jump" and k == 3:
                assert np.median(mom[F][:, 3]) >= 3.0


@pytest.mark.parametrize("W,H", SIZES)
def test_sequences_are_rarely_fragile(W, H):
    """Every synthetic sequence of the GPU test on the restatement alone: the fragile share within the cap in every call, the
    motion state each call is to report, and the float32 run's distance from the float64 one (the part of T these inputs give)."""
    worst = [0.0, 0.0]
    for name, seq in gpu_sequences(W, H, EMISSION_TOY).items():
        chk = MotionChecker(EMISSION_TOY, (W, H, name))
        for k, (ci, now, planes, rgba) in enumerate(seq):
            (out, mom, F, fragile), state = chk.restate(ci, (rgba,) + planes, now)
            assert F.any() or W * H == 1, (name, k)
            assert fragile.sum() <= FRAGILE_CAP * F.sum(), (name, k, int(fragile.sum()), int(F.sum()))
            if name.startswith("mixed"):
                assert state == (NO_MOTION if k == 0 else dict(movedObjects=2, replacedObjects=int(k == 3), movedSpheres=2))
                if k == 5 and W * H > 500:
                    ids = planes[3]
                    mesh, band = F & ((ids[..., 3] & 2) == 0), F & ((ids[..., 3] & 2) == 2)
                    front = name == "mixed_front"
                    for body in (mesh & (ids[..., 0] == (0 if front else 2)), band & (ids[..., 0] == (1 if front else 3))):
                        assert body.sum() > 10 and np.median(mom[body][:, 3]) >= 4.0, (name, int(body.sum()))    # the moved bodies kept theirs
                    if front:
                        assert med(mom[mesh & (ids[..., 0] == 1)][:, 3]) == 6.0
                    else:
                        p3 = mesh & (ids[..., 0] == 3)
                        assert p3.sum() > 10 and med(mom[p3][:, 3]) == 3.0     # replaced in call 3: 1, 2, 3
        worst = [max(a, b) for a, b in zip(worst, chk.worst_f32)]
    print(f"motion synthetic {W}x{H}: float32 restatement against float64, worst relative difference: colour {worst[0]:.3g} variance {worst[1]:.3g}")
    assert worst[0] <= MOTION_T_COLOUR / 4 and max(worst) <= MOTION_T / 4
    assert worst[0] <= max(MOTION_MEASURED_SYNTHETIC[0], T_COLOUR_MEASURED) and worst[1] <= max(MOTION_MEASURED_SYNTHETIC[1], T_MEASURED)


# ---------------------------------------------------------------- GPU helpers
def _host(r, ci, rgba, nd, position, albedo, ids):
    H, W = rgba.shape[:2]
    b = _capi.RtAovBuffers(normalDepth=nd.ctypes.data, position=position.ctypes.data, albedo=albedo.ctypes.data, ids=ids.ctypes.data)
    out, mom = np.empty_like(rgba), np.empty_like(rgba)
    r._check(r._l.rt_temporal_accumulate_host(r._h, W, H, C.byref(ci), rgba.ctypes.data, C.byref(b), None, out.ctypes.data, mom.ctypes.data),
             "rt_temporal_accumulate_host")
    return out, mom


class _DeviceRoute:
    """rt_temporal_accumulate on device planes the test owns: seven planes of one frame."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.bufs = [devmem.DeviceBuffer(W * H * 16) for _ in range(7)]

    def call(self, r, ci, rgba, nd, position, albedo, ids):
        for b, a in zip(self.bufs, (rgba, nd, position, albedo, ids)):
            b.upload(a)
        v = [b.ptr for b in self.bufs]
        d = _capi.RtAovBuffers(normalDepth=v[1], position=v[2], albedo=v[3], ids=v[4])
        r._check(r._l.rt_temporal_accumulate(r._h, self.W, self.H, C.byref(ci), v[0], C.byref(d), None, v[5], v[6]), "rt_temporal_accumulate")
        r.sync()
        return self.bufs[5].download((self.H, self.W, 4), np.float32), self.bufs[6].download((self.H, self.W, 4), np.float32)

    def close(self):
        for b in self.bufs:
            b.free()


def _place(e, now):
    """The placements `now` into the first objects and spheres of an EditedScene."""
    for o in range(len(now["M"])):
        e.objects[o].transformMatrix[:] = [float(x) for x in now["M"][o].T.ravel()]
        e.objects[o].bvhIndex = int(now["bvh"][o])
    for s in range(len(now["S"])):
        e.spheres[s].position[:] = [float(x) for x in now["S"][s][:3]]
        e.spheres[s].radius = float(now["S"][s][3])


def _push(r, e, prev, now):
    """rt_update_* for what differs, as a host would."""
    _place(e, now)
    if prev is None or not (np.array_equal(prev["M"].view(np.uint32), now["M"].view(np.uint32)) and np.array_equal(prev["bvh"], now["bvh"])):
        e.push(r, "objects")
    if prev is None or not np.array_equal(prev["S"].view(np.uint32), now["S"].view(np.uint32)):
        e.push(r, "spheres")


@pytest.fixture
def tracking(renderer):
    renderer.temporal_track_motion(True)
    yield renderer
    renderer.temporal_track_motion(False)


# ---------------------------------------------------------------- 1. synthetic planes against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_synthetic_planes_against_the_restatement(tracking, W, H):
    """Cornell's first four objects and spheres 1 and 3 take the sequences' placements through rt_update_objects and
    rt_update_spheres, so the library's own tables feed the kernel; the planes go through rt_temporal_accumulate_host and, the
    mixed sequence of the camera that looks back again, through device pointers."""
    r = tracking
    s = cornell_scene(True)
    assert [s.arrays().objects[i].bvhIndex for i in range(4)] == BASE_BVH.tolist()
    e = EditedScene(s)
    emission = emission_of(s)
    r.upload_scene(s)
    kept = {}
    for name, seq in gpu_sequences(W, H, emission).items():
        r.temporal_reset()
        chk = MotionChecker(emission, (W, H, name))
        prev = None
        for k, (ci, now, planes, rgba) in enumerate(seq):
            _push(r, e, prev, now)
            prev = now
            got, mom = _host(r, ci, rgba, *planes)
            (out, m, F, fragile), state = chk.check(ci, (rgba,) + planes, now, got, mom)
            assert r.temporal_motion_state() == state, (name, k)
            kept[name, k] = (got, mom)
        if name == "duality_unchanged":
            assert state == NO_MOTION
    route = _DeviceRoute(W, H)
    try:
        r.temporal_reset()
        prev = None
        for k, (ci, now, planes, rgba) in enumerate(gpu_sequences(W, H, emission)["mixed_back"]):
            _push(r, e, prev, now)
            prev = now
            got, mom = route.call(r, ci, rgba, *planes)
            assert np.array_equal(got.view(np.uint32), kept["mixed_back", k][0].view(np.uint32)) and np.array_equal(mom.view(np.uint32), kept["mixed_back", k][1].view(np.uint32))
            assert r.temporal_motion_state() == (NO_MOTION if k == 0 else dict(movedObjects=2, replacedObjects=int(k == 3), movedSpheres=2))
    finally:
        route.close()


# ---------------------------------------------------------------- 2. rendered sequences against the restatement
def camera_path(W, H, k, moving, **params):
    """Frame k: tests/test_temporal.py's path (a small yaw plus a translation) or its first camera, with a 20-degree field of view
    (module docstring, "Fragile share"); consecutive frameCounts."""
    j = k if moving else 0
    return engine.push_constants(W, H, cameraAngles=(4.0, 0.6 * j, 0.0), pos=(0.02 * j, -0.5, -3.5 + 0.03 * j), progressive=0, frameCount=k,
                                 **dict(dict(fov=RENDERED_FOV), **params))


def _edit(e, name, k, resize=True):
    """Frame k's edit. cornell_spheres: sphere 2 (diffuse) translates 0.01 along x and half that along y per frame and, with
    `resize`, shrinks; bunny: the model (the last object) turns about y and translates."""
    if name == "cornell_spheres":
        e.spheres[2].position[:] = [-0.5 + 0.01 * k, 0.1 + (0.005 * k if resize else 0.0), 0.0]
        e.spheres[2].radius = 0.4 - 0.01 * k if resize else 0.4
        return "spheres"
    e.set_transform(e.nObjects - 1, engine.placement(position=(0.01 * k, 0.53, -0.005 * k), rotation=(0.0, 2.0 * k, 0.0), scale=0.7, samplerIndex=1))
    return "objects"


@pytest.mark.gpu
@pytest.mark.parametrize("moving", [False, True], ids=["fixed_camera", "moving_camera"])
@pytest.mark.parametrize("name", ["cornell_spheres", "bunny"])
def test_rendered_sequences_against_the_restatement(tracking, name, moving):
    r = tracking
    s = cornell_scene(True) if name == "cornell_spheres" else model_scene("bunny.obj", spheres=True)
    e = EditedScene(s)
    W, H = 160, 120
    r.upload_scene(s)
    chk = MotionChecker(emission_of(s), (name, "moving" if moving else "fixed"), *((MOTION_T_COLOUR_RENDERED, MOTION_T) if moving else (MOTION_T_COLOUR_FIXED, MOTION_T_FIXED)))
    for k in range(8):
        if k:
            e.push(r, _edit(e, name, k))
        pc = camera_path(W, H, k, moving, raysPerPixel=1)
        frame = r.render(pc, W, H)
        a = r.render_aovs(pc, W, H)
        got, mom = r.temporal_accumulate(pc, moments=True)
        (out, m, F, fragile), state = chk.check(pc.camInfo, (frame,) + planes_of(a), placements_of(e), got, mom)
        assert r.temporal_motion_state() == state
        assert state == (NO_MOTION if k == 0 else dict(NO_MOTION, movedSpheres=1) if name == "cornell_spheres" else dict(NO_MOTION, movedObjects=1))
        ok = F & ~fragile
        assert (rel(mom[ok][:, 3], m[ok][:, 3]) <= chk.t).all()
    ids = planes_of(a)[3]
    body = F & (((ids[..., 3] & 2) == 2) & (ids[..., 0] == 2) if name == "cornell_spheres" else ((ids[..., 3] & 2) == 0) & (ids[..., 0] == e.nObjects - 1))
    assert body.sum() > 200 and np.median(mom[body][:, 3]) >= 4.0       # the moved body kept its history over most of the eight frames
    assert np.median(mom[F][:, 3]) >= 6.0


# ---------------------------------------------------------------- 3. tracking on, no edit
@pytest.mark.gpu
def test_tracking_without_an_edit_is_tracking_off(renderer):
    r = renderer
    s = cornell_scene(True)
    W, H = 64, 48
    r.upload_scene(s)
    pcs = [camera_path(W, H, k, True, raysPerPixel=1) for k in range(4)]
    state = lambda: (r.counters(), r.ray_cost(), r.last_pipeline(), r.last_parts(), r.last_kernel())  # noqa: E731

    def run():
        res = []
        for pc in pcs:
            frame = r.render(pc, W, H)
            a = r.render_aovs(pc, W, H)
            den = r.denoise()
            before = state()
            res.append(r.temporal_accumulate(pc, moments=True))
            assert r.temporal_motion_state() == NO_MOTION
            assert state() == before
            assert np.array_equal(r.read_rgba().view(np.uint32), frame.view(np.uint32))
            again = r.read_aovs()
            for k in a:
                assert np.array_equal(again[k].view(np.uint8), a[k].view(np.uint8)), k
            last = np.empty((H, W, 4), np.float32)
            r._check(r._l.rt_read_denoised_rgba_f32(r._h, last.ctypes.data_as(C.POINTER(C.c_float)), last.size), "rt_read_denoised_rgba_f32")
            assert np.array_equal(last.view(np.uint32), den.view(np.uint32))
        return res

    r.temporal_reset()
    off = run()
    r.temporal_track_motion(True)
    try:
        on = run()
        r.update_objects(s)      # the same placements again: bitwise equal rows, nothing moved
        r.update_spheres(s)
        more = r.temporal_accumulate(pcs[3], moments=True)
        assert r.temporal_motion_state() == NO_MOTION
    finally:
        r.temporal_track_motion(False)
    assert off[3][1][..., 3].max() > 3.0
    for (a, b), (c, d) in zip(off, on):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(b.view(np.uint32), d.view(np.uint32))
    assert more[1][..., 3].max() > 4.0


# ---------------------------------------------------------------- 4. what the feature buys
@pytest.mark.gpu
def test_a_moving_sphere_keeps_its_history(renderer):
    """Cornell + spheres, 160 x 120, eight 4-spp frames, the diffuse sphere moving 0.5 % of the box (0.01 of its 2) per frame.
    With tracking the median N on the sphere's pixels of F in the last frame is 8; with a reset after every edit, today's session,
    it is 1. Over all of F the accumulated frame is closer to a 1024-spp render of the last pose than the last raw frame is
    (measured ratio: DESIGN.md)."""
    r = renderer
    s = cornell_scene(True)
    W, H = 160, 120

    def run(track):
        e = EditedScene(s)
        r.upload_scene(s)
        r.temporal_track_motion(track)
        for k in range(8):
            if k:
                e.push(r, _edit(e, "cornell_spheres", k, resize=False))
                if not track:
                    r.temporal_reset()
            pc = camera_path(W, H, k, False, raysPerPixel=4)
            frame = r.render(pc, W, H)
            a = r.render_aovs(pc, W, H)
            got, mom = r.temporal_accumulate(pc, moments=True)
        return frame, a, got, mom

    try:
        frame, a, got, mom = run(True)
        clean = r.render(camera_path(W, H, 7, False, singleRender=1, sampleLimit=1024), W, H)
        _, _, _, mom_reset = run(False)
    finally:
        r.temporal_track_motion(False)
    ids = planes_of(a)[3]
    F = filtered_set(ids, emission_of(s))
    sphere = F & ((ids[..., 3] & 2) == 2) & (ids[..., 0] == 2)
    assert sphere.sum() > 300
    assert med(mom[sphere][:, 3]) == 8.0
    assert med(mom_reset[sphere][:, 3]) == 1.0
    c = lambda x: np.clip(np.asarray(x, np.float64)[..., :3], 0.0, 1.0)  # noqa: E731
    mse = lambda x: float(((c(x) - c(clean))[F] ** 2).mean())  # noqa: E731
    ratio = mse(got) / mse(frame)
    print(f"moving sphere: accumulated MSE {mse(got):.4g}, raw MSE {mse(frame):.4g}, ratio {ratio:.3f}; "
          f"on the sphere: {float(((c(got) - c(clean))[sphere] ** 2).mean()) / float(((c(frame) - c(clean))[sphere] ** 2).mean()):.3f}")
    assert ratio < 1.0


# ---------------------------------------------------------------- 5. resets and errors
@pytest.mark.gpu
def test_resets_drop_the_snapshot_and_refusals_keep_it(renderer):
    r = renderer
    s = cornell_scene(True)
    e = EditedScene(s)
    emission = emission_of(s)
    r.upload_scene(s)
    state = dict(now=start_placements(), k=0)
    moved = dict(movedObjects=1, replacedObjects=0, movedSpheres=0)

    def call(W=37, H=23, move=True):
        """One more call, patch 0 a little further along unless told not to: (N on F, the motion state)."""
        now = start_placements()
        state["k"] += 1 if move else 0
        now["M"][0] = matrix_of(position=(0.01 * state["k"], 0.0, 0.0))
        _push(r, e, None, now)
        state["now"] = now
        ci = cam(W, H, 3.0, (0.1, 0.05, 0.0), 2.0)
        planes = moved_planes(ci, W, H, emission, 5, now)
        got, mom = _host(r, ci, frame_over(planes[2], state["k"]), *planes)
        F = filtered_set(planes[3], emission)
        assert F.sum() > 100
        return mom[F][:, 3], r.temporal_motion_state()

    r.temporal_track_motion(True)
    try:
        N, st = call()
        assert (N == 1.0).all() and st == NO_MOTION
        N, st = call()
        assert med(N) == 2.0 and st == moved
        r.temporal_reset()
        N, st = call()
        assert (N == 1.0).all() and st == NO_MOTION          # the snapshot went with the history: nothing to compare with
        N, st = call()
        assert med(N) == 2.0 and st == moved
        r.temporal_track_motion(True)                         # the same value: nothing is forgotten
        N, st = call()
        assert med(N) == 3.0 and st == moved
        r.temporal_track_motion(False)                        # the toggle, both ways
        N, st = call()
        assert (N == 1.0).all() and st == NO_MOTION
        N, st = call(move=False)
        assert med(N) == 2.0 and st == NO_MOTION
        r.temporal_track_motion(True)
        N, st = call()
        assert (N == 1.0).all() and st == NO_MOTION
        N, st = call()
        assert med(N) == 2.0 and st == moved
        r.upload_scene(s)
        N, st = call()
        assert (N == 1.0).all() and st == NO_MOTION
        N, st = call()
        assert med(N) == 2.0 and st == moved
        N, st = call(23, 37)                                  # the same pixel count, another shape
        assert (N == 1.0).all() and st == NO_MOTION
        N, st = call(23, 37)
        assert med(N) == 2.0 and st == moved
        # a refused call leaves the history and the snapshot as they were: the edit made before it is still seen by the next one
        state["k"] += 1
        now = start_placements()
        now["M"][0] = matrix_of(position=(0.01 * state["k"], 0.0, 0.0))
        _push(r, e, None, now)
        ci = cam(23, 37)
        assert r._l.rt_temporal_accumulate(r._h, 23, 37, C.byref(ci), None, None, C.byref(_capi.RtTemporalParams(0, 0.9, 0.02)), None, None) < 0
        assert "maxHistory" in r._l.rt_last_error(r._h).decode()
        assert r._l.rt_temporal_accumulate(r._h, 23, 37, None, None, None, None, None, None) < 0
        assert r.temporal_motion_state() == moved             # still the last accepted call's
        state["k"] -= 1
        N, st = call(23, 37)
        assert med(N) == 3.0 and st == moved
    finally:
        r.temporal_track_motion(False)
    assert r._l.rt_temporal_track_motion(None, 1) == -1
    assert r._l.rt_temporal_motion_state(None, None, None, None) == -1
    assert r._l.rt_temporal_motion_state(r._h, None, None, None) == 0


# ---------------------------------------------------------------- 6. session
@pytest.mark.gpu
@pytest.mark.parametrize("track", [True, False])
def test_session_keeps_the_history_across_an_object_edit(renderer, track):
    s = cornell_scene(True)
    W, H = 64, 48
    ses = session.InteractiveSession(renderer, s, W, H, temporal=True, track_motion=track) if track else session.InteractiveSession(renderer, s, W, H, temporal=True)
    try:
        for k in range(3):
            ses.frame(keys="W", frame_time_ms=2.0)
        assert ses.history_length.max() == pytest.approx(3.0, abs=1e-3)
        # the tall box (object 1: 30 degrees about y, scale (0.3, 0.7, 0.3)) a little to the side
        ses.set_object(1, engine.placement(position=(0.42, -0.2, 0.45), rotation=(0.0, 30.0, 0.0), scale=(0.3, 0.7, 0.3)))
        ses.frame(keys="W", frame_time_ms=2.0)
        ids = engine.numpy_to_aovs(renderer.read_aovs())["ids"]
        F = filtered_set(ids, emission_of(s))
        box = F & ((ids[..., 3] & 2) == 0) & (ids[..., 0] == 1)
        rest = F & ~box
        assert box.sum() > 50 and rest.sum() > 500
        N = ses.history_length
        if track:
            assert renderer.temporal_motion_state() == dict(movedObjects=1, replacedObjects=0, movedSpheres=0)
            assert np.median(N[box]) > 1.0 and np.median(N[rest]) > 1.0
            ses.set_sphere(0, (0.0, 0.12, -0.3), 0.4, 5)
            ses.frame(keys="W", frame_time_ms=2.0)
            assert renderer.temporal_motion_state() == dict(movedObjects=0, replacedObjects=0, movedSpheres=1)
            assert np.median(ses.history_length[F]) > 1.0
            m = ses.material(0)
            m.albedo[0] = 0.25
            ses.set_material(0, m)                    # a material edit still resets
            ses.frame(keys="W", frame_time_ms=2.0)
            assert ses.history_length.max() == 1.0
        else:
            assert N.max() == 1.0
    finally:
        renderer.temporal_track_motion(False)
