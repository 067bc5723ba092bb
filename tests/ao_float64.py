"""TEST INFRASTRUCTURE — the ambient-occlusion plane (rt_render_ao) restated in numpy, float64.

Written from the comments of include/rt_ao_rays.h and from DESIGN.md, "Ray queries" / "Ambient-occlusion plane", not from the
header's code, the AO kernels or the oracle, and sharing no code with them: numpy only. The first hit of every pixel and every
occlusion query is tests/brute_force.py's closest_hit, through tests/paths_float64.py's Estimator (its float64 camera, its `_query`
with the exact and the rounded mode, its Run); the device's planes are no input.

THE RULE  Record i (pixel y W + x of the frame) with a first hit (p, n) shoots `samples` rays. The rt_random state of sample s under
`seed`, in uint32 arithmetic (exact: every product is taken modulo 2^32):
    h = i * 747796405 + 2891336453;  h ^= s;  h = h * 747796405 + 2891336453;  h ^= seed * 2654435769
The direction takes the next two draws r1, r2 of paths_float64.pcg's generator. A draw is float(r) / 4294967295.f in binary32, and
that divisor rounds to 2^32 in binary32, so pcg divides by 2^32 exactly, as rt_random does: the same binary32 number in both modes.
    dir = t (sqrt(r2) cos(phi)) + b (sqrt(r2) sin(phi)) + n sqrt(1 - r2),   phi = 2 pi r1
    axis = x unless |n.x| = 1, then z;   t = normalize(n x axis);   b = n x t
The axis is chosen on the float32 value of n.x, as paths_float64 chooses it: an exact +-1 there is no tie to break (an axis-aligned
wall gives exactly +-1 in float32), a value within 1e-4 of 1 that is not exact is fragile. The origin is p + 1e-5 n. Sample s is
occluded when closest_hit(offset_rays=True) hits with dst < radius (the directions are unit vectors). The plane is 1 where the
camera ray misses and (samples - k) / samples elsewhere, k the number of occluded samples.

A pixel is FRAGILE if its camera query or one of its sample queries is ill-conditioned by brute_force's rules, if a sample's hit
distance lies within 1e-4 (relative) of the radius, if the axis choice is fragile, or if its first hit's identity or one of its
occlusion bits differs between the exact run and any of the four rounded runs (sign seeds 1-4).
"""
import numpy as np

import paths_float64 as pf

MARGIN = 1e-4


def ao_state(i, sample, seed):
    """The rule's state of (record, sample, seed), uint32: products and sums modulo 2^32 (taken in uint64, whose low 32 bits of a
    product of two 32-bit words are exact)."""
    m, M = np.uint64(0xFFFFFFFF), np.uint64(747796405)
    A = np.uint64(2891336453)
    h = (np.asarray(i).astype(np.uint64) * M + A) & m
    h = h ^ np.uint64(int(sample) & 0xFFFFFFFF)
    h = (h * M + A) & m
    h = h ^ np.uint64((int(seed) * 2654435769) & 0xFFFFFFFF)
    return h.astype(np.uint32)


class Occlusion:
    """What one run leaves, per pixel: the first hit's identity, per sample the direction, the hit distance and the occlusion bit,
    the fragile flags of the run's own decisions."""

    def __init__(self, n, samples):
        self.hit = np.zeros(n, bool)
        self.code, self.corners = np.zeros(n, np.int64), np.zeros((n, 9))
        self.position, self.normal = np.zeros((n, 3)), np.zeros((n, 3))
        self.dirs, self.origins = np.zeros((n, samples, 3)), np.zeros((n, samples, 3))
        self.dst, self.occluded = np.full((n, samples), np.inf), np.zeros((n, samples), bool)
        self.ill, self.near_radius, self.axis = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)

    @property
    def k(self):
        return self.occluded.sum(axis=1)

    @property
    def fragile(self):
        return self.ill | self.near_radius | self.axis

    def differs(self, other):
        return (self.code != other.code) | (self.corners != other.corners).any(axis=1) | (self.occluded != other.occluded).any(axis=1)


class AmbientOcclusion:
    def __init__(self, brute, pc, W, H, samples, radius, seed):
        self.est = pf.Estimator(brute, pc, W, H)
        self.W, self.H, self.samples, self.radius, self.seed = int(W), int(H), int(samples), float(np.float32(radius)), int(seed)

    def run(self, rounded=None):
        F = np.float64 if rounded is None else np.float32
        N, S = self.W * self.H, self.samples
        R = pf.Run(N, F, rounded)
        out = Occlusion(N, S)
        with np.errstate(all="ignore"):
            o, d = self.est.camera(F)
            h = self.est._query(o, d, R)
            hit = h["didHit"]
            out.hit, out.ill = hit.copy(), h["ill"].copy()
            out.code = 1 | hit << 1 | (hit & h["isSphere"]) << 2 | (hit & h["front"]) << 3 | np.where(hit, h["object"], 0) << 12
            out.corners = np.where((hit & ~h["isSphere"])[:, None], h["corners"], 0)
            idx = np.flatnonzero(hit)
            p, n = h["p"][idx], h["n"][idx]
            out.position[idx], out.normal[idx] = p, n
            nx32 = np.abs(n[:, 0].astype(np.float32))
            out.axis[idx] = (nx32 != 1) & (np.abs(np.abs(n[:, 0].astype(np.float64)) - 1) < MARGIN)
            axis = np.where((nx32 != 1)[:, None], np.array([1, 0, 0], F), np.array([0, 0, 1], F))
            t = pf._normalize(pf._cross(n, axis))
            b = pf._cross(n, t)
            origin = p + F(0.00001) * n
            for s in range(S):
                state = ao_state(idx, s, self.seed)
                state, r1 = pf.pcg(state)
                state, r2 = pf.pcg(state)
                r1, r2 = r1.astype(F), r2.astype(F)
                phi, s2 = F(2.0 * np.pi) * r1, np.sqrt(r2)
                direction = (t * (s2 * np.cos(phi))[:, None] + b * (s2 * np.sin(phi))[:, None]) + n * np.sqrt(1 - r2)[:, None]
                assert direction.dtype == F and origin.dtype == F
                q = self.est._query(origin, direction, R)
                out.ill[idx] |= q["ill"]
                dst = np.where(q["didHit"], q["dst"], np.inf)
                out.dirs[idx, s], out.origins[idx, s], out.dst[idx, s] = direction, origin, dst
                out.occluded[idx, s] = q["didHit"] & (q["dst"] < F(self.radius))
                out.near_radius[idx] |= q["didHit"] & (np.abs(dst.astype(np.float64) - self.radius) <= MARGIN * self.radius)
        return out


class Study:
    """The exact run, the rounded runs, the fragile pixels, the plane, and the largest angle between a compared pixel's rounded
    and exact directions."""

    def __init__(self, ao, seeds=pf.SIGN_SEEDS):
        self.samples = ao.samples
        self.exact = ao.run(None)
        self.rounded = [ao.run(s) for s in seeds]
        fragile = self.exact.fragile.copy()
        for r in self.rounded:
            fragile |= self.exact.differs(r)
        self.fragile, self.compared = fragile, ~fragile
        self.hit, self.k = self.exact.hit, self.exact.k
        S = np.float32(self.samples)
        self.plane = np.where(self.hit, (S - self.k.astype(np.float32)) / S, np.float32(1)).astype(np.float32)
        self.rounded_angle = max(angle(r.dirs, self.exact.dirs, self.compared & self.hit) for r in self.rounded)

    @property
    def excluded(self):
        return float(self.fragile.mean())

    def per_k(self):
        m = self.compared & self.hit
        return {k: int((self.k[m] == k).sum()) for k in range(self.samples + 1)}


def angle(got, ref, mask):
    """Largest angle (radians) between the directions got and ref, [n, S, 3], over the pixels `mask`."""
    g, r = np.asarray(got, np.float64)[mask].reshape(-1, 3), np.asarray(ref, np.float64)[mask].reshape(-1, 3)
    if not len(g):
        return 0.0
    cross = np.linalg.norm(np.cross(g, r), axis=1)
    a = np.arctan2(cross, (g * r).sum(axis=1))
    return float(np.where(np.isnan(a), np.inf, a).max())
