"""A float64 restatement of the baked-light rule (include/rt_irradiance.h; rt_amd.h, "Baked light at points") by another route:
the generator on Python integers, its own bit reversal (a reversed binary string), numpy's trigonometry, the frame about the normal
and the spherical harmonics from their closed forms in float64. It shares no code with the header. Support module of
tests/test_irradiance_host.py and tests/test_irradiance.py.

The draws are the rule's: u = (float)r / 2^32 with (float)r rounded to fp32 (that rounding defines the draw); everything after
them is float64, so against it the fp32 rule shows its own roundings only. With u = 2^-24 (the unit roundoff of fp32) they are:

  r1 = ((float)s + u1) / (float)S   (float)s, (float)S exact (S < 2^24); the sum <= S rounds once, the quotient <= 1 once:
                                    |dr1| <= 2u
  r2 = v + u2 (- 1)                 v exact (24 bits x 2^-24); the sum < 2 rounds once (<= 2u); the subtraction is exact; where
                                    the two sides wrap differently phi differs by 2 pi, which no direction sees: |dr2| <= 2u
  phi = (2 pi) * r2                 the fp32 constant is 0.47u off (relative), the product rounds once:
                                    |dphi| <= 2 pi (2 + 0.47 + 1) u <= 22u
  rt_sincos                         Cephes' sinf / cosf polynomials, peak error 1.2e-7 = 2u (its documentation), and two rounded
                                    subtractions of the reduction on |r| <= pi / 4 (the first product is exact): 4u in all.
                                    |dsin|, |dcos| <= 22u + 4u = 26u
  sqrt(w) of w known to e           |d| <= e / sqrt(w) where w >= 4e, else 2.5 sqrt(e) (sqrt(w + e) <= sqrt(5e)); + u for its own
                                    rounding: SQ(w, e)
  sphere form                       z = 1 - 2 r1: 2 r1 exact, one rounding: |dz| <= 5u; 1 - z z: 2 |z| dz + 2 roundings <= 12u;
                                    rho = sqrt(max(0, .)): SQ(1 - z^2, 12u); x = rho cos: drho + 26u + u, y likewise, z: 5u
  cosine form                       sqrtR = sqrt(r1): SQ(r1, 2u); z' = sqrt(1 - r1): SQ(1 - r1, 3u); x' = cs sqrtR, y' = sn sqrtR:
                                    26u + dsqrtR + u. cross(n, axis) is exact (products with 0 and 1); normalize: the dot (three
                                    roundings, halved by the root), the root, the reciprocal, the scaling: |dt| <= 5u; b =
                                    cross(n, t): two products and a difference on |n| <= 1: |db| <= 2 (5u + u) + u = 13u;
                                    dir = (t x' + b y') + n z': three products, two sums of at most 1.5:
                                    |ddir| <= dt + db + dx' + dy' + dz' + 6u = 24u + dx' + dy' + dz'
  origin                            p + (n * 1) * bias: the product and the sum round once each: u |n bias| + u |origin|

dir_bound() evaluates these per sample from the float64 values. The gather's sum of S fp32 terms t_s: a partial sum takes
ceil(S / 64) additions, the fold 6, the scale (a product and a quotient, with the fp32 pi 0.47u off) 3 more, each at most u times
the running magnitude <= sum |t_s|: (6 + ceil(S / 64) + 3) u sum |t_s| x scale (gather_bound). A probe's terms L Y_j(dir) carry the
direction's bound into Y_j (bands 1 and 2 are Lipschitz in the components with at most 2.2), four roundings of the polynomial
and the constant (<= 9u) and the product with L (1.1u); the rule's six-digit constants are half a unit of their sixth digit from
the closed forms (5e-7 on a polynomial of at most 2): term_bound()."""
import math

import numpy as np

U = 2.0 ** -24
M32 = 0xFFFFFFFF


def _state(pid, sample, seed):
    h = (pid * 747796405 + 2891336453) & M32
    h ^= sample
    h = (h * 747796405 + 2891336453) & M32
    h ^= (seed * 2654435769) & M32
    return h


def _draw(state):
    s = (state * 747796405 + 2891336453) & M32
    r = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & M32
    r = (r >> 22) ^ r
    return s, float(np.float32(r)) / 4294967296.0


def shift(pid, frame):
    st = _state(int(pid) & M32, 0, int(frame) & M32)
    st, u1 = _draw(st)
    st, u2 = _draw(st)
    return u1, u2


def radical_inverse(s):
    return (int(format(int(s), "032b")[::-1], 2) >> 8) / 16777216.0


def draws(pid, frame, S):
    """(r1 (S,), r2 (S,)) of a point, float64."""
    u1, u2 = shift(pid, frame)
    s = np.arange(S, dtype=np.float64)
    r1 = (s + u1) / float(S)
    r2 = np.array([radical_inverse(k) for k in range(S)]) + u2
    return r1, np.where(r2 >= 1.0, r2 - 1.0, r2)


def _sq(w, e):
    w = np.maximum(w, 0.0)
    return np.where(w >= 4.0 * e, e / np.sqrt(np.maximum(w, 4.0 * e)), 2.5 * math.sqrt(e)) + U


def sphere_dirs(pid, frame, S):
    """The probe form's directions (S, 3) and the bound on each component of the fp32 rule's (S,)."""
    r1, r2 = draws(pid, frame, S)
    z = 1.0 - 2.0 * r1
    w = np.maximum(0.0, 1.0 - z * z)
    rho = np.sqrt(w)
    phi = 2.0 * np.pi * r2
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1), _sq(w, 12.0 * U) + 27.0 * U


def cosine_dirs(normal, pid, frame, S):
    """The irradiance form's directions about `normal` (unit length) and the bound on each component."""
    n = np.asarray(normal, np.float64)
    r1, r2 = draws(pid, frame, S)
    phi = 2.0 * np.pi * r2
    sr, zz = np.sqrt(r1), np.sqrt(np.maximum(1.0 - r1, 0.0))
    x, y = np.cos(phi) * sr, np.sin(phi) * sr
    axis = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 1.0 else np.array([0.0, 0.0, 1.0])
    t = np.cross(n, axis)
    t = t / np.linalg.norm(t)
    b = np.cross(n, t)
    d = x[:, None] * t[None] + y[:, None] * b[None] + zz[:, None] * n[None]
    dxy = 27.0 * U + _sq(r1, 2.0 * U)
    return d, 24.0 * U + 2.0 * dxy + _sq(1.0 - r1, 3.0 * U)


def origins(points, normals, bias):
    """The irradiance form's origins (n, 3) in float64 (bias: the fp32 value) and the bound per component."""
    p, n = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    b = float(np.float32(bias))
    o = p + n * b
    return o, U * np.abs(n * b) + U * np.abs(o) + 1e-45


def sh9(d):
    """The nine real spherical harmonics of bands 0..2 at unit vectors (.., 3), from the closed forms, in the rule's order."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k0, k1 = 0.5 / math.sqrt(math.pi), math.sqrt(3.0 / (4.0 * math.pi))
    k2, k20, k22 = 0.5 * math.sqrt(15.0 / math.pi), 0.25 * math.sqrt(5.0 / math.pi), 0.25 * math.sqrt(15.0 / math.pi)
    return np.stack([k0 * np.ones_like(x), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k20 * (3.0 * z * z - 1.0), k2 * x * z,
                     k22 * (x * x - y * y)], axis=-1)


def gather_roundings(S):
    return 6 + (S + 63) // 64 + 3


def irradiance(radiance, n, S):
    """E (n, 3) = pi mean L of fp32 records (n * S, 4), summed in float64, and gather_bound for it."""
    L = np.asarray(radiance, np.float64).reshape(n, S, 4)[:, :, :3]
    return math.pi * L.sum(axis=1) / S, gather_roundings(S) * U * np.abs(L).sum(axis=1) * math.pi / S + 1e-45


def probes(radiance, ids, frame, n, S):
    """c (n, 9, 3) = 4 pi mean L Y_j(dir) in float64 over the restatement's own directions, and its bound: the sum's roundings on
    sum |t_s| plus each term's own bound."""
    L = np.asarray(radiance, np.float64).reshape(n, S, 4)[:, :, :3]
    c, bound = np.zeros((n, 9, 3)), np.zeros((n, 9, 3))
    for i in range(n):
        d, eps = sphere_dirs(ids[i] if ids is not None else i, frame, S)
        Y = sh9(d)                                                    # (S, 9)
        terms = L[i][:, None, :] * Y[:, :, None]                      # (S, 9, 3)
        per_term = np.abs(L[i])[:, None, :] * (2.2 * eps[:, None, None] + 10.1 * U + 1e-6)
        per_term[:, 0, :] = np.abs(L[i]) * (1.1 * U + 5e-7)           # band 0 is a constant
        c[i] = 4.0 * math.pi * terms.sum(axis=0) / S
        bound[i] = 4.0 * math.pi / S * (gather_roundings(S) * U * (np.abs(terms).sum(axis=0) + per_term.sum(axis=0)) + per_term.sum(axis=0))
    return c, bound + 1e-45
