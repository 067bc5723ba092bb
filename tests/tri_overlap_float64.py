"""The triangle queries restated in numpy float64: which surfaces of a scene a closed query triangle touches, by brute force, and
the query triangles the tests ask about. Nothing here is shared with include/rt_tri_overlap.h, the exhaustive host loop or the
kernel: the world corners are nearest_float64.NearestScene's (its own reader of Scene.numpy(), the forward matrix applied in
float64); touching is not decided by a list of axes but by geometry: an edge of one triangle pierces the face of the other; and
apartness by the distance between the two triangles (the least of six corner-to-triangle and nine edge-to-edge distances).

Semantics restated ("Triangle queries"): the surfaces are every sphere with radius > 0 (its shell) and every triangle
of every object under the object's forward matrix; triangles are closed, touching counts; the members are reported spheres
first, then by object and triangle index.

The bound of one pair (query, primitive)
---------------------------------------
u = 2^-24. mag = |M||[v;1]| is the largest component over the scene triangle's corners (|c| + r for a sphere), R the largest
distance of the pair's six corners from the centre of the query's box, s = mag + R the size every rounding below scales with.
float32 does this (rt_xform_point, rt_tri_prepare, rt_tri_triangle_prepared), to first order in u:

  1. world corners, a row of three products and three sums: <= 4 u mag per component. The query's corners are given in float32.
  2. m^ = fl(lo/2 + hi/2) of the query's box. Whatever its rounding, it is one point that all six corners are taken relative
     to, and no decision below depends on where the origin is: take m^ as exact (this is why an origin 1e3 away costs nothing).
  3. corners relative to m^, fl(a - m^): one rounding of the difference itself, per component u R_Q for the query's corners
     (R_Q <= R their largest distance from the centre) and u R for the scene triangle's. So a relative corner of the query is
     within e_Q = u R_Q of the true one per component, one of the scene triangle within e_T = 4 u mag + u R, sqrt(3) times that
     as vectors.
  From here on take the two triangles Q^, T^ of the computed relative corners as exact objects: on any unit direction the gap or
  the overlap of their two intervals differs from the true triangles' by at most sqrt(3) (e_Q + e_T) <= (6.9 mag + 3.5 R) u.
  4. Stage 1 compares the corners' own numbers: no error beyond 1.
  5. An axis a^ of stage 2 is computed from the relative corners; whatever its error, it is a direction, and two closed convex
     sets whose intervals on ANY direction are strictly apart are disjoint. A projection is three products and two sums: its
     error is at most 3 u |a^|_1 |v|_inf <= 3 sqrt(3) u |a^|_2 R. A decision compares two of them: 6 sqrt(3) u R = 10.4 u R on
     the unit axis.
  3 and 5 together: (6.9 mag + 13.9 R) u <= 14 u s. C = 32 is twice that.

  Touching. If float32 calls the pair apart, the intervals of the true triangles on some direction overlap by less than 14 u s.
  Let an edge of one triangle pierce the other's face at x, at an angle theta to its plane, its ends at heights h1, h2 > 0 on
  opposite sides, and x at least rho inside the face's outline. On a unit direction d with in-plane part a and normal part b,
  the face's interval holds x.d +- rho a and the edge's holds x.d + h1 (b - a cot theta) and x.d - h2 (b - a cot theta) where
  b > a cot theta: the intervals overlap by at least min(rho, h1, h2) (a + max(b - a cot theta, 0)) >= min(rho, h1, h2) sin theta
  (the minimum over a^2 + b^2 = 1 lies at b = a cot theta). So with
      beta_touch = C u s / sin theta
  a pair in which such an edge has rho, h1, h2 > beta_touch is a float32 member: UNAMBIGUOUSLY TOUCHING. 1 / sin theta is the
  term of an ill-conditioned normal on this side: a grazing edge proves little.

  Apart. Let D be the float64 distance of the pair. The 17 directions of the rule and the three box axes, as unit vectors of
  the float64 triangles, see a gap g_k <= D each (g_k = D for the direction of the closest points, which is a face normal when
  a corner is nearest a face and an edge cross when two edges are nearest). float32 finds the pair apart on axis k when g_k
  exceeds what it loses there: the 14 u s of 3 and 5, and the turn of the computed axis: a^ = a + da moves a unit projection of
  a corner at distance R by at most 2 R |da| / |a|, a gap by twice that. An edge e of the query is off by at most
  |de| = sqrt(3) (2 e_Q + u |e|), an edge f of the scene triangle by |df| = sqrt(3) (2 e_T + u |f|), and the cross product's
  own three operations by 2 u: for a = e x f, |da| <= |de| |f| + |e| |df| + 6 u |e| |f|; for n x e with n itself a cross
  product, |dn| |e| + |n| |de| + 6 u |n| |e|. A box axis has da = 0. So
      beta_k = C u s + 4 R |da_k| / |a_k|,
  the second term the one of an ill-conditioned normal (nearly parallel edges, a sliver's face, a short edge seen from far), and
  the pair is UNAMBIGUOUSLY APART when D > beta = min over k with g_k > 0 of beta_k D / g_k: the distance against the bound, the
  bound scaled by how obliquely the rule's best direction sees the gap. (No g_k > 0: beta is +inf.)
  A pair whose boxes lie more than 64 u (|Q| + mag) apart on a box axis (|Q| the query's largest |coordinate|) is unambiguously
  apart by 4 alone; only the others are measured.

  A sphere: member iff dmin <= r <= dmax. rt_point_triangle's distance carries nearest_float64's bound b = 64 u (|c| + |Q|) +
  F(c, t) (its docstring, with the barycentric term F of the QUERY's shape, which a sliver makes first order near the face),
  the corner distances 8 u s, fl(r r) half a u of r. beta = 64 u (|Q| + |c| + r) + F; unambiguous when |dmin - r| and |dmax - r|
  exceed it.

No query and no primitive is exempt: `case_triangles` steers instead. A seeded query with an ambiguous pair is moved along its
own normal by 1/64 of its size (its longest edge) per step; the tests assert that every query got there within MAX_STEPS steps.

The queries go around the points of point_query_cases' four sets, the class is the point's index mod 4: small triangles whose
circumradius is 1.05 times the distance to the second nearest surface (about 2 members); slivers 1 : 16; large triangles of 0.3
to 1 times the scene's half-extent, every other one with an edge along the scene's longest axis (the long thin scenes are
crossed lengthwise); copies of the scene's own triangles turned about their centroid by a seeded rotation of 20 to 160 degrees
(small ones where the scene has no triangle). Every seeded size is at least 2^-7 of the scene's largest half-extent.
"""
import numpy as np

from nearest_float64 import U32
from overlap_float64 import expected_records   # noqa: F401  (the records of a member set: the key is the box queries')

C = 32.0
SPHERE_C = 64.0
MAX_STEPS = 8
CLASSES = ("small", "sliver", "large", "copy")

_cases = {}


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _safe(x):
    return np.where(x > 0, x, 1.0)


def point_triangle(p, t):
    """Distance from points p [M, 3] to triangles t [M, 3, 3]: the foot of the perpendicular where it falls inside (three signed
    areas), else the nearest of the three edges."""
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    ok = nn > 0
    h = _dot(p - a, n) / _safe(nn)
    foot = p - h[:, None] * n
    inside = ok & (_dot(np.cross(b - a, foot - a), n) >= 0) & (_dot(np.cross(c - b, foot - b), n) >= 0) & (_dot(np.cross(a - c, foot - c), n) >= 0)
    d = np.minimum(np.minimum(point_segment(p, a, b), point_segment(p, b, c)), point_segment(p, c, a))
    return np.where(inside, np.abs(h) * np.sqrt(nn), d)


def point_segment(p, a, b):
    ab = b - a
    den = _dot(ab, ab)
    t = np.clip(np.where(den > 0, _dot(p - a, ab) / _safe(den), 0.0), 0.0, 1.0)
    return _norm(p - (a + t[:, None] * ab))


def segment_segment(p1, q1, p2, q2):
    """Distance between segments p1-q1 and p2-q2 [M, 3] (the closed form with clamping; parallel segments by their ends)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
    b, c = _dot(d1, d2), _dot(d1, r)
    den = a * e - b * b
    s = np.clip(np.where(den > 1e-300, (b * f - c * e) / _safe(den), 0.0), 0.0, 1.0)
    t = np.where(e > 0, (b * s + f) / _safe(e), 0.0)
    s = np.where(t < 0, np.clip(np.where(a > 0, -c / _safe(a), 0.0), 0.0, 1.0), np.where(t > 1, np.clip(np.where(a > 0, (b - c) / _safe(a), 0.0), 0.0, 1.0), s))
    t = np.clip(t, 0.0, 1.0)
    d = _norm((p1 + s[:, None] * d1) - (p2 + t[:, None] * d2))
    ends = np.minimum(np.minimum(point_segment(p1, p2, q2), point_segment(q1, p2, q2)), np.minimum(point_segment(p2, p1, q1), point_segment(q2, p1, q1)))
    return np.minimum(d, ends)


def pierce(seg0, seg1, t):
    """Edges seg0-seg1 [M, 3] against faces t [M, 3, 3]: (crosses [M] bool: the ends lie on opposite sides or on the plane and the
    crossing point lies in the closed face; margin [M]: min(rho, h1, h2) sin theta where it crosses strictly, else 0)."""
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    n = np.cross(b - a, c - a)
    ln = _norm(n)
    ok = ln > 0
    n = n / _safe(ln)[:, None]
    h0, h1 = _dot(seg0 - a, n), _dot(seg1 - a, n)
    opposite = ok & (h0 * h1 < 0)
    f = h0 / np.where(opposite, h0 - h1, 1.0)
    x = seg0 + f[:, None] * (seg1 - seg0)
    rho = np.full(len(t), np.inf)
    for v, w in ((a, b), (b, c), (c, a)):
        e = w - v
        inward = np.cross(n, e)
        rho = np.minimum(rho, _dot(x - v, inward) / _safe(_norm(inward)))
    length = _norm(seg1 - seg0)
    sin = np.abs(h0 - h1) / _safe(length)
    crosses = opposite & (rho >= 0)
    margin = np.where(opposite, np.minimum(np.minimum(np.abs(h0), np.abs(h1)), rho) * sin, 0.0)
    return crosses, np.maximum(margin, 0.0), sin


def triangle_distance(q, t):
    """Distance between triangles q and t [M, 3, 3]: 0 where an edge of one crosses the other's face, else the least of the six
    corner-to-triangle and the nine edge-to-edge distances."""
    d = np.full(len(q), np.inf)
    hit = np.zeros(len(q), bool)
    for i in range(3):
        d = np.minimum(d, np.minimum(point_triangle(q[:, i], t), point_triangle(t[:, i], q)))
        hit |= pierce(q[:, i], q[:, (i + 1) % 3], t)[0] | pierce(t[:, i], t[:, (i + 1) % 3], q)[0]
        for j in range(3):
            d = np.minimum(d, segment_segment(q[:, i], q[:, (i + 1) % 3], t[:, j], t[:, (j + 1) % 3]))
    return np.where(hit, 0.0, d)


def _pair_size(q, t):
    """R [M]: the largest distance of the six corners from the centre of the query's box."""
    m = (q.min(axis=1) + q.max(axis=1)) / 2
    return _norm(np.concatenate([q, t], axis=1) - m[:, None, :]).max(axis=1)


def _cross_axis(e, de, f, df):
    """a = e x f with the bound of its float32 error |da| (module docstring, "Apart"), given the bounds of its factors'."""
    le, lf = _norm(e), _norm(f)
    return np.cross(e, f), de * lf + le * df + 6.0 * U32 * le * lf


def apart_bound(q, t, mag):
    """beta [M] of the docstring's "Apart" for the pairs q, t [M, 3, 3] with the scene triangles' magnitudes mag [M], and D [M]."""
    D = triangle_distance(q, t)
    R = _pair_size(q, t)
    s = mag + R
    eQ, eT = U32 * _pair_size(q, q), 4.0 * U32 * mag + U32 * R
    eq = [q[:, 1] - q[:, 0], q[:, 2] - q[:, 1], q[:, 0] - q[:, 2]]
    et = [t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]]
    deq = [np.sqrt(3.0) * (2.0 * eQ + U32 * _norm(e)) for e in eq]
    det = [np.sqrt(3.0) * (2.0 * eT + U32 * _norm(f)) for f in et]
    nq, dnq = _cross_axis(eq[0], deq[0], eq[1], deq[1])
    nt, dnt = _cross_axis(et[0], det[0], et[1], det[1])
    axes = [(nq, dnq), (nt, dnt)] + [_cross_axis(eq[i], deq[i], et[j], det[j]) for i in range(3) for j in range(3)]
    axes += [_cross_axis(nq, dnq, eq[i], deq[i]) for i in range(3)] + [_cross_axis(nt, dnt, et[j], det[j]) for j in range(3)]
    for i in range(3):
        axes.append((np.broadcast_to(np.eye(3)[i], nq.shape), np.zeros(len(q))))
    ratio = np.full(len(q), np.inf)
    for a, da in axes:
        la = _norm(a)
        unit = a / _safe(la)[:, None]
        pq_, pt_ = (q * unit[:, None, :]).sum(axis=-1), (t * unit[:, None, :]).sum(axis=-1)
        gap = np.maximum(pt_.min(axis=1) - pq_.max(axis=1), pq_.min(axis=1) - pt_.max(axis=1))
        beta_k = C * U32 * s + 4.0 * R * da / _safe(la)
        ratio = np.where((la > 0) & (gap > 0), np.minimum(ratio, beta_k / _safe(gap)), ratio)
    with np.errstate(invalid="ignore"):
        beta = np.where(np.isinf(ratio), np.inf, ratio * D)
    return beta, D


def touch_margin(q, t, mag):
    """The largest min(rho, h1, h2) sin theta - C u s over the six edges of the pair against the other's face ([M]; > 0: unambiguously
    touching)."""
    best = np.full(len(q), -np.inf)
    s = mag + _pair_size(q, t)
    for i in range(3):
        for seg, face in (((q[:, i], q[:, (i + 1) % 3]), t), ((t[:, i], t[:, (i + 1) % 3]), q)):
            _, margin, _ = pierce(seg[0], seg[1], face)
            best = np.maximum(best, margin - C * U32 * s)     # (margin carries sin theta)
    return best


def _shape(q):
    """kappa and L of nearest_float64's bound for the triangles q [P, 3, 3]."""
    ab, ac, bc = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], q[:, 2] - q[:, 1]
    e1, e2, nn = _norm(ab), _norm(ac), (np.cross(ab, ac) ** 2).sum(axis=1)
    return np.where(nn > 0, e1 * e2 * (e1 + e2) / _safe(nn), 0.0), np.maximum(np.maximum(e1, e2), _norm(bc))


def classify(ns, q):
    """member [P, N] (spheres first, then the rows of ns.W) and clear [P, N] for the queries q [P, 3, 3] (float64 of float32)."""
    P, S, N = len(q), len(ns.sph_c), len(ns.sph_c) + len(ns.W)
    member, clear = np.zeros((P, N), bool), np.ones((P, N), bool)
    size = np.abs(q).max(axis=(1, 2))
    if S:
        rows, cols = np.repeat(np.arange(P), S), np.tile(np.arange(S), P)
        c, r = ns.sph_c[cols], ns.sph_r[cols]
        dmin = point_triangle(c, q[rows])
        dmax = _norm(q[rows] - c[:, None, :]).max(axis=1)
        kappa, longest = _shape(q)
        t = np.minimum(longest[rows], 94.0 * U32 * kappa[rows] * dmax * dmax)
        F = t * np.where(dmin > 0, np.minimum(1.0, t / (2.0 * _safe(dmin))), 1.0)
        beta = SPHERE_C * U32 * (size[rows] + np.abs(c).max(axis=1) + r) + F
        member[rows, cols] = (dmin <= r) & (r <= dmax)
        clear[rows, cols] = (np.abs(dmin - r) > beta) & (np.abs(dmax - r) > beta)
    if len(ns.W):
        s_all = size[:, None] + ns.mag[None, :]
        g = (SPHERE_C * U32 * s_all)[:, :, None]
        tlo, thi = ns.W.min(axis=1), ns.W.max(axis=1)
        qlo, qhi = q.min(axis=1), q.max(axis=1)
        near = ((thi[None] >= qlo[:, None, :] - g) & (tlo[None] <= qhi[:, None, :] + g)).all(axis=-1)
        rows, cols = np.nonzero(near)
        if len(rows):
            qq, tt, mag = q[rows], ns.W[cols], ns.mag[cols]
            touching = touch_margin(qq, tt, mag) > 0
            beta, D = apart_bound(qq, tt, mag)
            apart = D > beta
            member[rows, S + cols] = touching
            clear[rows, S + cols] = touching | apart
    return member, clear


class Triangles:
    """corners [P, 9] float32; cls [P] (index into CLASSES); steps [P]; clear [P]: every primitive is unambiguous; member [P, N]
    bool, spheres first."""


def _rotations(rng, n):
    """n seeded rotation matrices [n, 3, 3], uniform by QR of a normal matrix."""
    m, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    m = m * np.sign(np.einsum("nii->ni", r))[:, None, :]
    m[:, :, 2] *= np.sign(np.linalg.det(m))[:, None]
    return m


def _axis_angle(axis, angle):
    axis = axis / _norm(axis)[:, None]
    K = np.zeros((len(axis), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return np.eye(3)[None] + np.sin(angle)[:, None, None] * K + (1 - np.cos(angle))[:, None, None] * (K @ K)


def seed_triangles(name, key):
    """The seeded queries (corners [P, 3, 3] float64, cls [P]) of a point set, before any steering, from the float64 scene alone."""
    import point_query_cases as pq
    import within_float64 as wf
    c = pq.case(name)
    ns = c["ns"]
    p = c["sets"][key].astype(np.float64)
    d = np.sort(wf.case_distances(name, key).d, axis=1)
    P, N = d.shape
    lo, hi = ns.box()
    scene = float(((hi - lo) / 2).max())
    longest_axis = np.eye(3)[int(np.argmax(hi - lo))]
    rng = np.random.default_rng(9300 + 16 * pq.SCENES.index(name) + list(c["sets"]).index(key))
    cls = np.arange(P) % 4
    if not len(ns.W):
        cls[cls == 3] = 0
    rot = _rotations(rng, P)
    # a unit equilateral triangle about the origin in the plane z = 0 (circumradius 1), and a 1 : 16 sliver of half-length 1
    unit = np.array([[1.0, 0.0, 0.0], [-0.5, np.sqrt(0.75), 0.0], [-0.5, -np.sqrt(0.75), 0.0]])
    sliver = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0625, 0.0], [-1.0, -0.0625, 0.0]])
    rad = np.zeros(P)
    rad[cls == 0] = 1.05 * d[cls == 0, min(1, N - 1)]
    rad[cls == 1] = 1.05 * d[cls == 1, min(8, N - 1)]
    rad[cls == 2] = scene * rng.uniform(0.3, 1.0, int((cls == 2).sum()))
    rad = np.maximum(rad, scene / 128)
    base = np.where((cls == 1)[:, None, None], sliver[None], unit[None])
    q = p[:, None, :] + rad[:, None, None] * np.einsum("pij,pkj->pki", rot, base)
    along = np.flatnonzero(cls == 2)[::2]            # every other large one: its first edge along the scene's longest axis
    if len(along):
        w = rot[along, :, 1]
        w = w - _dot(w, longest_axis)[:, None] * longest_axis
        w = w / _safe(_norm(w))[:, None]
        r = rad[along, None]
        q[along] = p[along, None, :] + np.stack([r * longest_axis, -r * longest_axis, 0.5 * r * w], axis=1) - (0.5 * r * w / 3)[:, None, :]
    copy = np.flatnonzero(cls == 3)
    if len(copy):
        t = ns.W[rng.integers(0, len(ns.W), len(copy))]
        centre = t.mean(axis=1)
        R = _axis_angle(rng.normal(size=(len(copy), 3)), np.radians(rng.uniform(20, 160, len(copy))))
        q[copy] = centre[:, None, :] + np.einsum("pij,pkj->pki", R, t - centre[:, None, :])
    return q, cls


def _normal_and_size(q):
    n = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    n = n / _safe(_norm(n))[:, None]
    size = np.maximum(np.maximum(_norm(q[:, 1] - q[:, 0]), _norm(q[:, 2] - q[:, 1])), _norm(q[:, 0] - q[:, 2]))
    return n, size


def seed_corners(name, key):
    """The seeded queries as the entry points take them ([P, 9] float32), before any steering: what the GPU tests ask about, where
    the device is held to the exhaustive loop and nothing needs to be unambiguous."""
    return seed_triangles(name, key)[0].reshape(-1, 9).astype(np.float32)


def case_triangles(name, key, chunk=64):
    """The Triangles of point set `key` of scene `name` of tests/point_query_cases.py, once per session."""
    import point_query_cases as pq
    if (name, key) in _cases:
        return _cases[(name, key)]
    ns = pq.case(name)["ns"]
    seed, cls = seed_triangles(name, key)
    normal, size = _normal_and_size(seed)
    P, N = len(seed), len(ns.sph_c) + len(ns.W)
    b = Triangles()
    b.cls, b.steps, b.clear = cls, np.zeros(P, np.int64), np.zeros(P, bool)
    b.corners, b.member = np.zeros((P, 9), np.float32), np.zeros((P, N), bool)
    todo = np.arange(P)
    for step in range(MAX_STEPS + 1):
        moved = seed[todo] + (step / 64.0) * (size[todo, None] * normal[todo])[:, None, :]
        corners = moved.reshape(-1, 9).astype(np.float32)
        ok = np.zeros(len(todo), bool)
        for at in range(0, len(todo), chunk):
            rows = slice(at, at + chunk)
            member, clear = classify(ns, corners[rows].astype(np.float64).reshape(-1, 3, 3))
            ok[rows] = clear.all(axis=1)
            b.member[todo[rows]] = member
        b.corners[todo], b.steps[todo], b.clear[todo] = corners, step, ok
        todo = todo[~ok]
        if not len(todo):
            break
    _cases[(name, key)] = b
    return b
