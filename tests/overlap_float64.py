"""The box queries restated in numpy float64: which surfaces of a scene a closed axis-aligned box touches, by brute force, and
the boxes the tests ask about. Nothing here is shared with include/rt_box_overlap.h, the exhaustive host loop or the kernel: the
world corners are nearest_float64.NearestScene's (its own reader of Scene.numpy(), the forward matrix applied in float64), the
triangle test is the 13-axis separating-axis test written on all three corners' projections (the header projects two), and the
sphere test compares distances, not squares.

Semantics restated ("Box queries"): the surfaces are every sphere with radius > 0 (its shell) and every triangle of
every object under the object's forward matrix; boxes are closed, touching counts; the members are reported spheres first, then
by object and triangle index.

The bound beta of one pair (box, primitive)
------------------------------------------
u = 2^-24. |box| is the largest |coordinate| of the box, mag = |M||[v;1]| the largest component over the triangle's corners
(|c| + r for a sphere), s = |box| + mag: the size every rounding below scales with. float32 does this (rt_xform_point,
rt_box_triangle), to first order in u:

  1. world corners, a row of three products and three sums: <= 4 u mag per component.
  2. centre m = fl(lo/2 + hi/2) and half-extent h = fl(hi/2 - lo/2): the halvings are exact, one rounding each: u |box|.
  3. corners relative to the centre, v^ = fl(a - m): u (|a| + |m|) <= u s. With 1 and 2: every component of v^ is within
     e_v = 6 u s of the true corner relative to the true centre, and h within u |box| of the true half-extent.
  From here on take the triangle T^ of the computed v^ and the box [-h, h] as exact objects. T^ is the true triangle with every
  corner moved by at most e_v per axis, so if T^ touches a box, the true triangle touches that box grown by e_v on every axis (a
  common point p^ = sum l_i v^_i has the true point sum l_i v_i within e_v of it), and if T^ is separated from a box, the true
  triangle is separated from that box shrunk by e_v.
  4. Stage 1, the box axes: comparisons of v^'s own numbers (the header compares a_i with lo_i; the difference to comparing
     v^_i with h_i is inside e_v). No further error.
  5. The nine edge axes a = e x unit_i, e^ = fl(v^_1 - v^_0): each component of e^ is the exact difference of T^'s corners
     times (1 + d), |d| <= u. Both projected corners are p = e^_z v_y - e^_y v_z: the relative errors of e^'s components, of
     the two products and of the difference give |dp| <= 3 u |a|_1 |v| with |a|_1 = |e_y| + |e_z| and |v| <= 2 s; the radius
     r = fl(h_y |e^_z| + h_z |e^_y|) likewise |dr| <= 3 u |a|_1 |h|. Growing the box by x on every axis grows r by x |a|_1, so
     the decision on such an axis is the exact decision of T^ against the box grown or shrunk by at most 3 u (2 s) + 3 u s
     = 9 u s. (The third corner needs no term: on the exact axis of T^ it projects where the edge's other corner does.)
  So stages 1 and 3 are exact for a box within (6 + 9) u s = 15 u s of the given one: C = 32.
  6. The plane axis n = e0 x e1 is the one term that is no multiple of s. A component n_x = e0_y e1_z - e1_y e0_z is a
     difference of two products: |dn_x| <= 4 u (|e0_y| |e1_z| + |e1_y| |e0_z|) =: 4 u Nbar_x, and for a thin triangle the
     products cancel, so n^ has no relative accuracy: the normal of a sliver is ill-conditioned where the slab tests are not.
     d = n . v0 and r = h . |n| move by at most |dn|_1 (|v| + |h|) (and, on the axis n^ taken as it is, the three corners
     project within |dn|_1 |e| of each other, |e| <= 2 |v|), against r's growth of x |n|_1 for a box grown by x:
         P = 4 u |Nbar|_1 (2 V + H) / |n|_1,   V = max |v|, H = max h,
     which for a triangle of longest edge L and width w is about 4 u L (2 V + H) / w. It enters as a term of its own, with a
     count of its own (4), not C's.
     Its defect on the member side is bounded by the triangle's width: a triangle lies within w = |n|_2 / L of its longest
     edge, and the nine edge axes hold the three of that edge, which with the three box axes are the complete test of the
     segment. If float32 keeps the triangle, stages 1 and 3 kept it, so the segment's six axes do not separate it from the box
     grown by 15 u s + w, hence the segment, hence the triangle, touches that box. So a float32 member touches the box grown by
         beta_in = C u s + min(P, w),
     and a float32 non-member is separated from the box shrunk by
         beta_out = C u s + P
     (P is 0 for a triangle with two equal corners: e and n are exactly 0 and separate nothing).
  A sphere: d2min and d2max are three exact-to-u differences, three squares and two sums, 4.5 u relative on the square, 2.25 u on
  the distance, fl(r r) 0.5 u on r; the distances are at most sqrt(3) (|box| + |c|): 8 u s covers it, and a box grown by x has
  its nearest distance reduced and its farthest increased by at least x. beta = C u s with the same C.

A pair is unambiguous when the float64 test gives one answer for the box grown by beta_in and for the box shrunk by beta_out on
every axis; that answer is then the float32 rule's. No box and no primitive is exempt: `case_boxes` steers instead. Each seeded
box grows its half-extents by 1/64 of their seeded size per step until every primitive of the scene is unambiguous for it; the
tests assert that every box got there within MAX_STEPS steps and that every half-extent exceeds the largest beta_out of its row.

The boxes: centres are the points of point_query_cases' four sets, the class is the point's index mod 3: small cubes whose
half-extent is 1.05 times the distance to the second nearest surface (about 2 members); 1 : 4 : 16 boxes (h/4, h, 4 h) with h
1.05 times the distance to the ninth nearest (more than 8 where the scene has them); large boxes of 0.3 to 1 times the scene's
half-extent. Every seeded half-extent is at least 2^-7 of the scene's largest half-extent.
"""
import numpy as np

from nearest_float64 import U32

C = 32.0
MAX_STEPS = 8
CLASSES = ("cube", "slab", "large")

_boxes = {}


def triangles_touch(lo, hi, W):
    """lo, hi [M, 3] (a box per pair), W [M, 3, 3] -> [M] bool: the closed box touches the closed triangle, in float64."""
    c, h = (lo + hi) / 2, (hi - lo) / 2
    v = W - c[:, None, :]                                               # [M, corner, axis]
    out = (v.min(axis=1) > h).any(axis=-1) | (v.max(axis=1) < -h).any(axis=-1)
    e = np.stack([W[:, 1] - W[:, 0], W[:, 2] - W[:, 1], W[:, 0] - W[:, 2]], axis=1)   # [M, edge, axis]
    axes = [np.cross(e[:, 0], e[:, 1])]
    for j in range(3):
        for i in range(3):
            axes.append(np.cross(e[:, j], np.eye(3)[i]))
    for a in axes:                                                      # [M, 3]
        p = (v * a[:, None, :]).sum(axis=-1)                            # [M, corner]
        r = (h * np.abs(a)).sum(axis=-1)
        out |= (p.min(axis=-1) > r) | (p.max(axis=-1) < -r)
    return ~out


def spheres_touch(lo, hi, centre, radius):
    """lo, hi [M, 3], centre [M, 3], radius [M] -> [M] bool: the closed box touches the shell."""
    near = np.maximum(np.maximum(lo - centre, 0.0), centre - hi)
    far = np.maximum(centre - lo, hi - centre)
    return (np.linalg.norm(near, axis=-1) <= radius) & (radius <= np.linalg.norm(far, axis=-1))


class Geometry:
    """What the bound needs of a scene's triangles, once: |Nbar|_1, |n|_1, the width, and which are segments or points."""

    def __init__(self, ns):
        W = ns.W
        e0, e1, e2 = W[:, 1] - W[:, 0], W[:, 2] - W[:, 1], W[:, 0] - W[:, 2]
        a0, a1 = np.abs(e0), np.abs(e1)
        self.nbar = (a0[:, 1] * a1[:, 2] + a1[:, 1] * a0[:, 2]) + (a0[:, 2] * a1[:, 0] + a1[:, 2] * a0[:, 0]) + (a0[:, 0] * a1[:, 1] + a1[:, 0] * a0[:, 1])
        n = np.cross(e0, e1)
        self.n1 = np.abs(n).sum(axis=1)
        longest = np.maximum(np.maximum(np.linalg.norm(e0, axis=1), np.linalg.norm(e1, axis=1)), np.linalg.norm(e2, axis=1))
        self.width = np.where(longest > 0, np.linalg.norm(n, axis=1) / np.where(longest > 0, longest, 1.0), 0.0)
        self.equal = ((e0 == 0).all(axis=1) | (e1 == 0).all(axis=1) | (e2 == 0).all(axis=1))


def betas(ns, geo, lo, hi, c=C):
    """beta_in, beta_out [P, N] for the boxes lo, hi [P, 3] against every primitive (spheres first, then the rows of ns.W)."""
    size = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)               # |box|
    sph = c * U32 * (size[:, None] + (np.abs(ns.sph_c).max(axis=1) + ns.sph_r)[None, :]) if len(ns.sph_c) else np.zeros((len(lo), 0))
    if not len(ns.W):
        return sph, sph
    first = c * U32 * (size[:, None] + ns.mag[None, :])
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    V = np.abs(ns.W[None] - centre[:, None, None, :]).max(axis=(2, 3))  # [P, N]
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(geo.equal[None, :], 0.0, 4.0 * U32 * geo.nbar[None, :] * (2.0 * V + half.max(axis=1)[:, None]) / geo.n1[None, :])
    P = np.where(np.isnan(P), np.inf, P)
    return np.concatenate([sph, first + np.minimum(P, geo.width[None, :])], axis=1), np.concatenate([sph, first + P], axis=1)


def classify(ns, geo, lo, hi, c=C):
    """member [P, N] (the float64 answer for the box shrunk by beta_out), clear [P, N] (the box grown by beta_in gives the same
    answer) and beta_out [P, N]."""
    b_in, b_out = betas(ns, geo, lo, hi, c)
    s = len(ns.sph_c)

    # The pairs whose triangle's own box misses the box grown by beta_in fail the three box axes for the grown box and for the
    # shrunk one inside it: no member, unambiguously. The 13 axes run on the rest.
    tlo, thi = ns.W.min(axis=1), ns.W.max(axis=1)
    near = np.zeros(b_in.shape, bool)
    near[:, :s] = True
    if len(ns.W):
        g = b_in[:, s:, None]
        near[:, s:] = ((thi[None] >= lo[:, None, :] - g) & (tlo[None] <= hi[:, None, :] + g)).all(axis=-1)
    rows, cols = np.nonzero(near)

    def touch(grow):
        g = grow[rows, cols][:, None]
        l, h = lo[rows] - g, hi[rows] + g
        out = np.zeros(b_in.shape, bool)
        sph = cols < s
        if sph.any():
            out[rows[sph], cols[sph]] = spheres_touch(l[sph], h[sph], ns.sph_c[cols[sph]], ns.sph_r[cols[sph]])
        if (~sph).any():
            out[rows[~sph], cols[~sph]] = triangles_touch(l[~sph], h[~sph], ns.W[cols[~sph] - s])
        return out

    small, big = touch(-b_out), touch(b_in)
    return small, small == big, b_out


class Boxes:
    """lo, hi [P, 3] float32; cls [P] (index into CLASSES); half [P, 3] (float64, of the float32 box); steps [P]; clear [P]: every
    primitive is unambiguous; beta_max [P]: the largest beta_out of the row; member [P, N] bool, spheres first."""


def seed_half(name, key):
    """The seeded half-extents [P, 3] of a point set, by its class rule, from the float64 distances alone."""
    import point_query_cases as pq
    import within_float64 as wf
    c = pq.case(name)
    d = np.sort(wf.case_distances(name, key).d, axis=1)
    P, N = d.shape
    lo, hi = c["ns"].box()
    scene = float(((hi - lo) / 2).max())
    rng = np.random.default_rng(9000 + 16 * pq.SCENES.index(name) + list(c["sets"]).index(key))
    cls = np.arange(P) % 3
    half = np.zeros((P, 3))
    h2, h9 = 1.05 * d[:, min(1, N - 1)], 1.05 * d[:, min(8, N - 1)]
    half[cls == 0] = h2[cls == 0, None]
    half[cls == 1] = h9[cls == 1, None] * np.array([0.25, 1.0, 4.0])[rng.permuted(np.tile(np.arange(3), (int((cls == 1).sum()), 1)), axis=1)]
    half[cls == 2] = scene * rng.uniform(0.3, 1.0, (int((cls == 2).sum()), 3))
    return np.maximum(half, scene / 128), cls


def seed_boxes(name, key):
    """The seeded boxes (lo, hi [P, 3] float32) before any growth step: what the GPU tests ask about, where the device is held to
    the exhaustive loop and nothing needs to be unambiguous."""
    import point_query_cases as pq
    q = pq.case(name)["sets"][key].astype(np.float64)
    half, _ = seed_half(name, key)
    return (q - half).astype(np.float32), (q + half).astype(np.float32)


def case_boxes(name, key, chunk=32):
    """The Boxes of point set `key` of scene `name` of tests/point_query_cases.py, once per session."""
    import point_query_cases as pq
    if (name, key) in _boxes:
        return _boxes[(name, key)]
    c = pq.case(name)
    ns, geo = c["ns"], Geometry(c["ns"])
    q = c["sets"][key].astype(np.float64)
    seed, cls = seed_half(name, key)
    P, N = len(q), len(ns.sph_c) + len(ns.W)
    b = Boxes()
    b.cls, b.steps, b.clear = cls, np.zeros(P, np.int64), np.zeros(P, bool)
    b.lo, b.hi = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    b.member, b.beta_max = np.zeros((P, N), bool), np.zeros(P)
    todo = np.arange(P)
    for step in range(MAX_STEPS + 1):
        half = seed[todo] * (1.0 + step / 64.0)
        lo, hi = (q[todo] - half).astype(np.float32), (q[todo] + half).astype(np.float32)
        ok = np.zeros(len(todo), bool)
        for at in range(0, len(todo), chunk):
            rows = slice(at, at + chunk)
            member, clear, b_out = classify(ns, geo, lo[rows].astype(np.float64), hi[rows].astype(np.float64))
            ok[rows] = clear.all(axis=1)
            idx = todo[rows]
            b.member[idx], b.beta_max[idx] = member, b_out.max(axis=1) if N else 0.0
        b.lo[todo], b.hi[todo], b.steps[todo], b.clear[todo] = lo, hi, step, ok
        todo = todo[~ok]
        if not len(todo):
            break
    b.half = (b.hi.astype(np.float64) - b.lo.astype(np.float64)) / 2
    _boxes[(name, key)] = b
    return b


def expected_records(ns, member, k):
    """The records [P, k, 4] uint32 (found, isSphere, objectIndex, triIndex) of the member sets in the order of the key: the
    columns are already in it (spheres by index, then ns.W's rows: by object, then by triangle)."""
    s = len(ns.sph_c)
    first = np.concatenate([ns.sph_index, ns.obj]).astype(np.uint32)
    tri = np.concatenate([np.zeros(s, np.int64), ns.tri]).astype(np.uint32)
    sphere = (np.arange(member.shape[1]) < s).astype(np.uint32)
    out = np.zeros((member.shape[0], k, 4), np.uint32)
    for i in range(member.shape[0]):
        cols = np.flatnonzero(member[i])[:k]
        out[i, :len(cols)] = np.stack([np.ones(len(cols), np.uint32), sphere[cols], first[cols], tri[cols]], axis=1)
    return out
