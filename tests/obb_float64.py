"""The oriented box queries restated in numpy float64: which surfaces of a scene a closed box { p : lo <= F p <= hi } touches, by
brute force, and the placed boxes the tests ask about. Nothing here is shared with include/rt_obb_overlap.h, the exhaustive host
loop or the kernel: ObbScene is this module's own reader of Scene.numpy() (object-space corners, the forward matrix, both in
float64), the frame F is read as float64 from the fp32 numbers, the corners are taken through M and then F in float64, and the box
test on the frame coordinates is overlap_float64's (triangles_touch, spheres_touch). A sphere is tested by the declared formula,
centre F c and radius r |first column of F|, whatever the frame ("Oriented box queries").

The bound beta of one pair (box, primitive), in frame coordinates
-----------------------------------------------------------------
u = 2^-24. z = F w + s is the exact frame corner of the exact world corner w = M v + t. float32 does this, to first order in u:

  1. world corner (placed objects only; an identity object's corner is used as it is), a row of three products and three sums:
     |w^ - w| <= 4 u a per component, a = |M||v| + |t|.
  2. frame corner z^ = fl(F w^ + s), the same row: |z^ - (F w^ + s)| <= 4 u (|F||w| + |s|), and F w^ + s = z + F (w^ - w) with
     |F (w^ - w)| <= 4 u |F| a: the world step amplified by |F|. Together, per component,
         e_z = 4 u (|F||w| + |s| + |F| a)        (a = 0 for an identity object),
     and the pair's e_z is the largest over its corners and components.
  From here rt_box_triangle runs on z^ as overlap_float64's docstring counts it, but counted relative to what each operation
  produces, not to its operands: the frame coordinates of a box about an origin 10^3 away are 10^3 in size while the box and the
  corners relative to its centre are not, and fl(x - y) errs by u |x - y|.
  3. centre m = fl(lo/2 + hi/2): u |box|; half-extent h = fl(hi/2 - lo/2): u H, H the largest half-extent.
  4. corners relative to the centre, v^ = fl(z^ - m): u V, V the largest |corner - centre| component. So v^ is within
     e_z + u |box| + u V of the true relative corner and h within u H of the true half-extent. Stage 1 compares z^'s own numbers
     with lo and hi: no further error.
  5. The nine edge axes: that docstring's item 5 with |v| <= V: |dp| <= 3 u |a|_1 V, |dr| <= 3 u |a|_1 H: 3 u (V + H).
  So stages 1 and 3 are exact for a box within
         first = e_z + u |box| + 4 u (V + H)
  of the given one (1 + 3 for V, 1 + 3 for H), and beta takes SAFETY = 2 times that for the second-order terms, as that module
  takes 32 for its counted 15.
  6. The plane axis: that docstring's item 6 unchanged, on the frame-coordinate triangle: P = 4 u |Nbar|_1 (2 V + H) / |n|_1,
     bounded on the member side by the triangle's width w: beta_in = SAFETY first + min(P, w), beta_out = SAFETY first + P.
  A sphere: the centre as item 2 (no world step), e_c = 4 u (|F||c| + |s|) per component, sqrt(3) e_c on a distance; the scale
  s = fl(sqrt((m0 m0 + m1 m1) + m2 m2)) has 3 u on the square, 1.5 u + 0.5 u on the root, fl(r s) one more: 3 u R on the radius
  R; rt_box_sphere itself, that docstring's count relative to the results: three differences, squares and two sums, 2.25 u on each
  distance, 0.5 u more on R: 3 u (D + R), D the farthest distance. beta = SAFETY (sqrt(3) e_c + 3 u R + 3 u (D + R)).

A pair is unambiguous when the float64 test gives one answer for the local box grown by beta_in and shrunk by beta_out on every
axis. No box and no primitive is exempt: `case_obbs` steers as overlap_float64.case_boxes does, the local half-extents growing by
1/64 of their seeded size per step, at most MAX_STEPS steps.

The boxes: overlap_float64's seeded half-extents about the points of point_query_cases' four sets, in its three classes by the
point's index mod 3, each under one of four frame kinds by index mod 4:
  0  a seeded rotation R (from a unit quaternion; orthonormal to rounding) about the point: F p = R^T (p - q);
  1  a rotation times a uniform scale g in [0.25, 4]: F p = g R^T (p - q), the local half-extents g times the seeded ones;
  2  the inverse matrix (engine.object_frames: rt_mat4_inverse) of one of the scene's placed objects, seeded, the scaled and the
     sheared ones included; the local box is about F q with the seeded half-extents times the length of F's rows. Where the
     scene has no placed object, a seeded shear about the point instead;
  3  a rotation about an origin 10^3 away from the scene's middle in a seeded direction: F p = R^T (p - o). The local
     coordinates are 10^3 in size, where fp32 numbers lie 2^-14 to 2^-13 apart: e_z is about 4 u 10^3 = 2.4e-4 whatever the box,
     beta about 6e-4, and the steering moves a face by 1/64 of the half-extent a step. A half-extent below 64 beta could not take
     a face out of one pair's zone in a step, so this kind's seeded half-extents are at least FAR_FLOOR = 2^-4 (about 100 beta).
SEED, the seed of the frames, was chosen so that every box of every scene is unambiguous within MAX_STEPS: about one seed in six
is; under the others one to three of the 1 664 boxes of the densest scene (four bunnies) stay ambiguous, all of the far kind.
"""
import numpy as np

import overlap_float64 as of
from nearest_float64 import U32

SAFETY = 2.0
MAX_STEPS = 8
KINDS = ("rotation", "similarity", "object", "far")
FAR = 1000.0
FAR_FLOOR = 2.0 ** -4
SEED = 41000   # chosen so that every box of every scene is unambiguous within MAX_STEPS (about one seed in six is)

_obbs = {}
_scenes = {}


class ObbScene:
    """The surfaces of Scene.numpy() in float64: spheres (sph_c, sph_r, sph_index) and one row per (object, triangle) pair in the
    order of the key (by object, then by triangle): V object-space corners, W world corners, A = |M||v| + |t| per corner (0 for an
    object whose matrix rows are the identity's: its corners are used as they are), obj, tri; placed: the objects with a matrix."""

    def __init__(self, arrays):
        sp = arrays["spheres"]
        self.sph_c, self.sph_r, self.sph_index = np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int64)
        if len(sp):
            f = sp.view(np.float32).reshape(len(sp), -1).astype(np.float64)
            keep = f[:, 3] > 0
            self.sph_c, self.sph_r, self.sph_index = f[keep, 0:3], f[keep, 3], np.flatnonzero(keep)
        self.W, self.A = np.zeros((0, 3, 3)), np.zeros((0, 3, 3))
        self.obj, self.tri, self.placed = np.zeros(0, np.int64), np.zeros(0, np.int64), []
        ob = arrays["objects"]
        if not len(ob):
            return
        points = arrays["triPoints"].view(np.float32).reshape(-1, 8)[:, 0:3].astype(np.float64)
        corners = arrays["triangles"].view(np.uint32).reshape(len(arrays["triangles"]), -1)[:, 0:3].astype(np.int64)
        nodes = arrays["bvhNodes"].view(np.uint32).reshape(len(arrays["bvhNodes"]), -1)[:, 6:8]
        mats = ob.view(np.float32).reshape(len(ob), -1)[:, 0:16].astype(np.float64)
        roots = ob.view(np.uint32).reshape(len(ob), -1)[:, 17]
        W, A, oi, ti = [], [], [], []
        for i in range(len(ob)):
            todo, tris = [int(roots[i])], []
            while todo:
                index, count = (int(x) for x in nodes[todo.pop()])
                if count:
                    tris += list(range(index, index + count))
                else:
                    todo += [index, index + 1]
            t = np.array(sorted(tris), np.int64)
            M = mats[i].reshape(4, 4).T                                        # column-major: m[c * 4 + r]
            v = points[corners[t]]                                             # [T, corner, 3]
            if np.array_equal(M[:3], np.eye(4)[:3]):
                W.append(v); A.append(np.zeros_like(v))
            else:
                self.placed.append(i)
                W.append(v @ M[:3, :3].T + M[:3, 3]); A.append(np.abs(v) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3]))
            oi.append(np.full(len(t), i, np.int64)); ti.append(t)
        self.W, self.A, self.obj, self.tri = np.concatenate(W), np.concatenate(A), np.concatenate(oi), np.concatenate(ti)

    def middle(self):
        pts = [self.W.reshape(-1, 3)] if len(self.W) else []
        if len(self.sph_c):
            pts += [self.sph_c - self.sph_r[:, None], self.sph_c + self.sph_r[:, None]]
        p = np.concatenate(pts)
        return (p.min(axis=0) + p.max(axis=0)) / 2


def scene(name):
    import point_query_cases as pq
    if name not in _scenes:
        _scenes[name] = ObbScene(pq.case(name)["arrays"])
    return _scenes[name]


def frame_parts(frames):
    """(n, 16) float32 -> the linear part A [n, 3, 3] and the translation s [n, 3], float64 (the four other floats are not read)."""
    f = np.asarray(frames, np.float32).astype(np.float64).reshape(-1, 4, 4)    # [n, column, row]
    return np.transpose(f[:, :3, :3], (0, 2, 1)), f[:, 3, :3]


def pack_frames(A, s):
    """Linear parts [n, 3, 3] and translations [n, 3] -> (n, 16) float32, column-major, the last row (0, 0, 0, 1)."""
    f = np.zeros((len(A), 4, 4))
    f[:, :3, :3] = np.transpose(A, (0, 2, 1))
    f[:, 3, :3] = s
    f[:, 3, 3] = 1.0
    return np.ascontiguousarray(f.reshape(-1, 16).astype(np.float32))


def classify(os_, A, s, lo, hi):
    """member [P, N] (the float64 answer for the local box shrunk by beta_out), clear [P, N] (the box grown by beta_in gives the
    same answer) and beta_out [P, N], for the boxes lo, hi [P, 3] (float64) under the frames A [P, 3, 3], s [P, 3]."""
    P, S, T = len(lo), len(os_.sph_c), len(os_.W)
    size = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    H = half.max(axis=1)
    absA = np.abs(A)
    b_in, b_out = np.zeros((P, S + T)), np.zeros((P, S + T))
    member, grown = np.zeros((P, S + T), bool), np.zeros((P, S + T), bool)
    if S:
        cz = np.einsum("pij,nj->pni", A, os_.sph_c) + s[:, None, :]
        ec = 4.0 * U32 * (np.einsum("pij,nj->pni", absA, np.abs(os_.sph_c)) + np.abs(s)[:, None, :]).max(axis=-1)
        R = os_.sph_r[None, :] * np.linalg.norm(A[:, :, 0], axis=1)[:, None]
        D = np.linalg.norm(np.maximum(cz - lo[:, None, :], hi[:, None, :] - cz), axis=-1)
        beta = SAFETY * (np.sqrt(3.0) * ec + 3.0 * U32 * R + 3.0 * U32 * (D + R))
        b_in[:, :S], b_out[:, :S] = beta, beta
        for grow, into in ((-beta, member), (beta, grown)):
            g = grow[..., None]
            into[:, :S] = of.spheres_touch((lo[:, None, :] - g).reshape(-1, 3), (hi[:, None, :] + g).reshape(-1, 3), cz.reshape(-1, 3), R.reshape(-1)).reshape(P, S)
    if T:
        Z = np.einsum("pij,ncj->pnci", A, os_.W) + s[:, None, None, :]                         # [P, T, corner, axis]
        mag = np.einsum("pij,ncj->pnci", absA, np.abs(os_.W) + os_.A) + np.abs(s)[:, None, None, :]
        ez = 4.0 * U32 * mag.max(axis=(2, 3))
        V = np.abs(Z - centre[:, None, None, :]).max(axis=(2, 3))
        first = SAFETY * (ez + U32 * size[:, None] + 4.0 * U32 * (V + H[:, None]))
        # the pairs whose triangle's own frame box misses the box grown by what beta_in can be at most fail the three box axes
        # for the grown box and for the shrunk one inside it: no member, unambiguously. The 13 axes run on the rest.
        e0, e1, e2 = Z[:, :, 1] - Z[:, :, 0], Z[:, :, 2] - Z[:, :, 1], Z[:, :, 0] - Z[:, :, 2]
        longest = np.maximum(np.maximum(np.linalg.norm(e0, axis=-1), np.linalg.norm(e1, axis=-1)), np.linalg.norm(e2, axis=-1))
        n = np.cross(e0, e1)
        width = np.where(longest > 0, np.linalg.norm(n, axis=-1) / np.where(longest > 0, longest, 1.0), 0.0)
        a0, a1 = np.abs(e0), np.abs(e1)
        nbar = (a0[..., 1] * a1[..., 2] + a1[..., 1] * a0[..., 2]) + (a0[..., 2] * a1[..., 0] + a1[..., 2] * a0[..., 0]) + (a0[..., 0] * a1[..., 1] + a1[..., 0] * a0[..., 1])
        n1 = np.abs(n).sum(axis=-1)
        equal = (e0 == 0).all(axis=-1) | (e1 == 0).all(axis=-1) | (e2 == 0).all(axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            Pl = np.where(equal, 0.0, 4.0 * U32 * nbar * (2.0 * V + H[:, None]) / n1)
        Pl = np.where(np.isnan(Pl), np.inf, Pl)
        t_in, t_out = first + np.minimum(Pl, width), first + Pl
        b_in[:, S:], b_out[:, S:] = t_in, t_out
        zlo, zhi = Z.min(axis=2), Z.max(axis=2)
        near = ((zhi >= lo[:, None, :] - t_in[..., None]) & (zlo <= hi[:, None, :] + t_in[..., None])).all(axis=-1)
        rows, cols = np.nonzero(near)
        for grow, into in ((-t_out, member), (t_in, grown)):
            g = grow[rows, cols][:, None]
            into[rows, S + cols] = of.triangles_touch(lo[rows] - g, hi[rows] + g, Z[rows, cols])
    return member, member == grown, b_out


class Obbs:
    """frames [P, 16] float32; lo, hi [P, 3] float32 (local); cls, kind [P]; half [P, 3] (float64, of the float32 box); steps [P];
    clear [P]: every primitive is unambiguous; beta_max [P]: the largest beta_out of the row; member [P, N] bool, spheres first."""


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def seed_frames(name, key):
    """The frames [P, 16] float32 of a point set, the kind [P] of each, and the seeded LOCAL centres and half-extents [P, 3]
    (float64): the frame is fixed before any steering, the local box is about F q with the half-extents of its kind."""
    import point_query_cases as pq
    from ray_tracer_amd import engine
    c = pq.case(name)
    os_ = scene(name)
    q = c["sets"][key].astype(np.float64)
    half, cls = of.seed_half(name, key)
    P = len(q)
    rng = np.random.default_rng(SEED + 16 * pq.SCENES.index(name) + list(c["sets"]).index(key))
    kind = np.arange(P) % 4
    R = _rotations(rng, P)
    Rt = np.transpose(R, (0, 2, 1))
    gain = np.exp(rng.uniform(np.log(0.25), np.log(4.0), P))
    A = Rt.copy()
    A[kind == 1] *= gain[kind == 1, None, None]
    s = -np.einsum("pij,pj->pi", A, q)
    direction = rng.normal(size=(P, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    origin = os_.middle() + FAR * direction
    far = kind == 3
    s[far] = -np.einsum("pij,pj->pi", A[far], origin[far])
    frames = pack_frames(A, s)
    own = kind == 2
    if os_.placed:
        pick = np.array(os_.placed)[rng.integers(0, len(os_.placed), int(own.sum()))]
        frames[own] = engine.object_frames(c["scene"].arrays(), pick)
    else:
        sh = np.tile(np.eye(3), (int(own.sum()), 1, 1))
        sh[:, 0, 1], sh[:, 0, 2], sh[:, 1, 2] = rng.uniform(-0.5, 0.5, (3, int(own.sum())))
        frames[own] = pack_frames(sh, -np.einsum("pij,pj->pi", sh, q[own]))
    A, s = frame_parts(frames)
    centre = np.einsum("pij,pj->pi", A, q) + s
    half = half.copy()
    half[far] = np.maximum(half[far], FAR_FLOOR)
    half[kind == 1] *= gain[kind == 1, None]
    half[own] *= np.linalg.norm(A[own], axis=2)
    return frames, kind, cls, centre, half


def seed_obbs(name, key):
    """The seeded placed boxes (frames [P, 16], lo, hi [P, 3] float32) before any growth step: what the GPU tests ask about, where
    the device is held to the exhaustive loop and nothing needs to be unambiguous."""
    frames, _, _, centre, half = seed_frames(name, key)
    return frames, (centre - half).astype(np.float32), (centre + half).astype(np.float32)


def case_obbs(name, key, chunk=32):
    """The Obbs of point set `key` of scene `name` of tests/point_query_cases.py, once per session."""
    if (name, key) in _obbs:
        return _obbs[(name, key)]
    os_ = scene(name)
    frames, kind, cls, centre, seed = seed_frames(name, key)
    A, s = frame_parts(frames)
    P, N = len(centre), len(os_.sph_c) + len(os_.W)
    b = Obbs()
    b.frames, b.kind, b.cls, b.steps, b.clear = frames, kind, cls, np.zeros(P, np.int64), np.zeros(P, bool)
    b.lo, b.hi = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    b.member, b.beta_max = np.zeros((P, N), bool), np.zeros(P)
    todo = np.arange(P)
    for step in range(MAX_STEPS + 1):
        half = seed[todo] * (1.0 + step / 64.0)
        lo, hi = (centre[todo] - half).astype(np.float32), (centre[todo] + half).astype(np.float32)
        ok = np.zeros(len(todo), bool)
        for at in range(0, len(todo), chunk):
            rows = slice(at, at + chunk)
            idx = todo[rows]
            member, clear, b_out = classify(os_, A[idx], s[idx], lo[rows].astype(np.float64), hi[rows].astype(np.float64))
            ok[rows] = clear.all(axis=1)
            b.member[idx], b.beta_max[idx] = member, b_out.max(axis=1) if N else 0.0
        b.lo[todo], b.hi[todo], b.steps[todo], b.clear[todo] = lo, hi, step, ok
        todo = todo[~ok]
        if not len(todo):
            break
    b.half = (b.hi.astype(np.float64) - b.lo.astype(np.float64)) / 2
    _obbs[(name, key)] = b
    return b
