"""The cut queries restated in numpy float64: the segment along which a closed query triangle crosses a triangle of the scene, by
brute force, and the query triangles the tests ask about. Nothing here is shared with include/rt_tri_cut.h, the exhaustive host
loop or the kernel: the world corners are nearest_float64.NearestScene's, and the cut of a pair is not found by heights, spans
and a tie order but by geometry: it is the two points where an edge of one triangle pierces the closed face of the other
(tri_overlap_float64.pierce). Spheres are never members.

When a pair is unambiguous
--------------------------
u = 2^-24; s = mag + R is tri_overlap_float64's pair magnitude (the scene triangle's |M||[v;1]| plus the pair's size about the
centre of the query's box). A pair is UNAMBIGUOUS when
  (i)   it is unambiguously apart by tri_overlap_float64.apart_bound: the gate of the rule refuses it, no cut; or
  (ii)  exactly two of its six edges pierce the other's face, each with its margin min(rho, h1, h2) sin theta above the
        touching bound 32 u s of that module (so the gate keeps the pair); every one of the six corners is farther from the
        other's plane than the height bound below (so float32 sees the same four edges cross the planes); and the four points
        where those edges cross are ordered along the common line by more than the sum of their position bounds (so float32 picks
        the same two, in the same order, under the same feature codes); or
  (iii) it is exactly coplanar (every float64 height is 0: the scene's own axis-aligned triangle as the query): no cut.
Everything else is ambiguous, and `case_cuts` steers the query away from it.

The position bound of an end point
----------------------------------
The end x lies on an edge lo-hi of one triangle, where it crosses the plane of the other at the angle theta. float32 does this
(rt_tri_cut_prepared, steps 2 to 5 of the rule), to first order in u, in units of u s, as tri_overlap_float64 counts:
  1. the world corners (4 roundings a component) and the corners relative to m (1): as vectors sqrt(3) (e_Q + e_T)
     <= (6.9 mag + 3.5 R) u. They move the two heights of the edge's ends over the other's plane ...                     7
  2. ... and they move the edge itself sideways, the point with it (sqrt(3) e_T <= 6.9 mag u + 1.7 R u) ...              7
  3. a height is the difference of two projections on the computed normal, three products and two sums each, as a
     decision of the triangle rule is: 6 sqrt(3) u R = 10.4 u R on the unit normal; with 1 and rounded up, that module's 14;
     here only the 7 left of it ...                                                                                      7
  4. the difference of the two projections is itself rounded ...                                                         1
  5. f = s_lo / (s_lo - s_hi): a difference and a quotient, relative 2 u, times the edge |hi - lo| <= 2 R ...             4
  6. lo + (hi - lo) f: a difference and a product on |hi - lo| <= 2 R, a sum on at most R ...                            5
                                                                                                                 counted: 31
  A height error dh moves the point along the edge by dh / sin theta; 2, 5 and 6 move it by themselves, and are put under the
  same 1 / sin theta >= 1. C_cut = 62 is twice the count, the project's practice (32 against 14 there). The turn of the
  computed normal n^ = n + dn of the other triangle moves the height of a corner X by at most |X - A| |dn| / |n|, A the corner
  the rule takes that triangle's heights from (its first) and |dn| that module's bound for a cross product of two rounded
  edges ("Apart"); it is taken twice, as there. It is the term of a sliver's normal.
      height bound   H(X) = C_cut u s + 2 |X - A| |dn| / |n|
      position bound B = max(H(lo), H(hi)) / sin theta + u |x|    (the last: step 5 of the rule, fl(X + m), as a vector)
  The rule orders the candidates by rt_dot(D, x), three products and two sums on the computed common line: 3 sqrt(3) u R = 5.2 u R
  on the unit line, and the turn of D moves the projection of a point that lies within B of the line by a part of B: both lie
  within the 31 u s that C_cut leaves over the count.

The tests hold the loop to this on unambiguous pairs: its member set and counts are the pairs of (ii); featA / featB name the two
piercing edges (0..2 the query's edge from corner i, 3..5 the scene triangle's edge from corner j); both ends lie within B of the
float64 points, a with a and b with b in the order of the rule's common line nQ x nT when the cut is longer than twice the
bounds, and in either order when it is shorter.

The queries are tri_overlap_float64.seed_triangles': its four classes around the points of point_query_cases' four sets on its
six scenes, the large ones turned by 3 degrees (`seed_triangles` says why). No query and no primitive is exempt: a query with an ambiguous pair is moved along its own normal by 1/64 of its size
a step, and the tests assert on this side alone that every one gets there within MAX_STEPS steps.
"""
import numpy as np

import tri_overlap_float64 as tf
from nearest_float64 import U32

C_CUT = 62.0
MAX_STEPS = 8

_cases = {}


def _unit(v):
    return v / tf._safe(tf._norm(v))[:, None]


def _normals(q, t, mag):
    """The float64 normals nq, nt [M, 3] of the pairs by the rule's own products (eQ0 x eQ1, eT0 x eT1), and |dn| / |n| of the
    float32 ones (tri_overlap_float64's bound of a cross product of two rounded edges)."""
    R = tf._pair_size(q, t)
    eQ, eT = U32 * tf._pair_size(q, q), 4.0 * U32 * mag + U32 * R
    out = []
    for tri, e in ((q, eQ), (t, eT)):
        e0, e1 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1]
        d0, d1 = np.sqrt(3.0) * (2.0 * e + U32 * tf._norm(e0)), np.sqrt(3.0) * (2.0 * e + U32 * tf._norm(e1))
        n, dn = tf._cross_axis(e0, d0, e1, d1)
        out.append((n, dn / tf._safe(tf._norm(n))))
    return out[0], out[1], R


def cut_pairs(q, t, mag):
    """The pairs q, t [M, 3, 3] (scene magnitudes mag [M]) that tri_overlap_float64 found unambiguously touching:
    ok [M] (case (ii) holds), a, b [M, 3] (the two piercing points, a first on nQ x nT), fa, fb [M] (their edges' codes),
    ba, bb [M] (their position bounds), coplanar [M] (case (iii))."""
    M = len(q)
    (nq, turn_q), (nt, turn_t), R = _normals(q, t, mag)
    s = mag + R
    uq, ut = _unit(nq), _unit(nt)
    hq = ((q - t[:, :1]) * ut[:, None, :]).sum(axis=-1)      # the query's corners over the scene triangle's plane [M, 3]
    ht = ((t - q[:, :1]) * uq[:, None, :]).sum(axis=-1)      # the scene triangle's corners over the query's plane
    coplanar = (hq == 0).all(axis=1) & (ht == 0).all(axis=1)
    # a height over nT is taken from the scene triangle's first corner, one over nQ from the query's: the turn acts on that arm
    arm_q, arm_t = tf._norm(q - t[:, :1]), tf._norm(t - q[:, :1])
    Hq = C_CUT * U32 * s[:, None] + 2.0 * arm_q * turn_t[:, None]      # [M, 3]: the query's corners over nT
    Ht = C_CUT * U32 * s[:, None] + 2.0 * arm_t * turn_q[:, None]
    heights_clear = (np.abs(hq) > Hq).all(axis=1) & (np.abs(ht) > Ht).all(axis=1)
    touch = tf.C * U32 * s
    pts, bound, code, crosses_plane, pierces, strong = [], [], [], [], [], []
    for tri, other, h, H, first in ((q, t, hq, Hq, 0), (t, q, ht, Ht, 3)):
        for e in range(3):
            x0, x1, h0, h1 = tri[:, e], tri[:, (e + 1) % 3], h[:, e], h[:, (e + 1) % 3]
            opposite = h0 * h1 < 0
            f = h0 / np.where(opposite, h0 - h1, 1.0)
            x = x0 + f[:, None] * (x1 - x0)
            sin = np.abs(h0 - h1) / tf._safe(tf._norm(x1 - x0))
            crosses, margin, _ = tf.pierce(x0, x1, other)
            pts.append(x); code.append(np.full(M, first + e)); crosses_plane.append(opposite)
            bound.append(np.maximum(H[:, e], H[:, (e + 1) % 3]) / np.where(sin > 0, sin, 1.0) + U32 * tf._norm(x))
            pierces.append(crosses); strong.append(margin > touch)
    pts, bound, code = np.stack(pts, axis=1), np.stack(bound, axis=1), np.stack(code, axis=1)
    crosses_plane, pierces, strong = np.stack(crosses_plane, axis=1), np.stack(pierces, axis=1), np.stack(strong, axis=1)
    two = (pierces.sum(axis=1) == 2) & ((pierces & strong).sum(axis=1) == 2)
    four = (crosses_plane[:, :3].sum(axis=1) == 2) & (crosses_plane[:, 3:].sum(axis=1) == 2)
    ok = two & four & heights_clear
    a, b = np.zeros((M, 3)), np.zeros((M, 3))
    fa, fb, ba, bb = np.zeros(M, np.int64), np.zeros(M, np.int64), np.zeros(M), np.zeros(M)
    line = _unit(np.cross(nq, nt))
    for i in np.flatnonzero(ok):
        idx = np.flatnonzero(crosses_plane[i])
        d = pts[i, idx] @ line[i]
        order = idx[np.argsort(d, kind="stable")]
        d = np.sort(d)
        bo = bound[i, order]
        if not (np.diff(d) > bo[:-1] + bo[1:]).all() or not (pierces[i, order[1]] and pierces[i, order[2]]):
            ok[i] = False
            continue
        a[i], b[i], fa[i], fb[i], ba[i], bb[i] = pts[i, order[1]], pts[i, order[2]], code[i, order[1]], code[i, order[2]], bo[1], bo[2]
    return ok, a, b, fa, fb, ba, bb, coplanar


def classify(ns, q):
    """For the queries q [P, 3, 3] (float64 of float32): member [P, T] (the pair has a cut; T the rows of ns.W), clear [P, T],
    and the cuts of the members as a dict of flat arrays (row, col, a, b, fa, fb, ba, bb) in (row, col) order."""
    S = len(ns.sph_c)
    touching, tri_clear = tf.classify(ns, q)
    touching, tri_clear = touching[:, S:], tri_clear[:, S:]
    member, clear = np.zeros_like(touching), tri_clear & ~touching          # (i): apart
    rows, cols = np.nonzero(touching & tri_clear)
    cuts = dict(row=rows, col=cols, a=np.zeros((0, 3)), b=np.zeros((0, 3)), fa=np.zeros(0, np.int64), fb=np.zeros(0, np.int64), ba=np.zeros(0), bb=np.zeros(0))
    if len(rows):
        ok, a, b, fa, fb, ba, bb, coplanar = cut_pairs(q[rows], ns.W[cols], ns.mag[cols])
        member[rows, cols] = ok
        clear[rows, cols] = ok | coplanar
        cuts = dict(row=rows[ok], col=cols[ok], a=a[ok], b=b[ok], fa=fa[ok], fb=fb[ok], ba=ba[ok], bb=bb[ok])
    return member, clear, cuts


class Cuts:
    """corners [P, 9] float32; cls [P]; steps [P]; clear [P]: every scene triangle is unambiguous; member [P, T] bool over
    ns.W's rows; cuts: dict of flat arrays over the member pairs in (query, row of ns.W) order, which is the key's order."""


def seed_triangles(name, key):
    """tri_overlap_float64.seed_triangles' queries (corners [P, 3, 3] float64, cls [P]), the large ones turned about their
    centroid by 3 degrees about a seeded axis. As seeded there, every other large triangle has an edge along the scene's longest
    axis and its third corner straight beside the point it was made around: on a point of an axis-aligned wall that corner lies
    exactly in the wall's plane, and moving the query along its own normal, which is parallel to the wall, never takes it out
    (cornell/surface: 23 queries were still ambiguous after 8 steps). Turned, they still cross the long scenes lengthwise."""
    import point_query_cases as pq
    q, cls = tf.seed_triangles(name, key)
    q = q.copy()
    large = np.flatnonzero(cls == 2)
    if len(large):
        rng = np.random.default_rng(9700 + 16 * pq.SCENES.index(name) + list(pq.case(name)["sets"]).index(key))
        centre = q[large].mean(axis=1)
        R = tf._axis_angle(rng.normal(size=(len(large), 3)), np.full(len(large), np.radians(3.0)))
        q[large] = centre[:, None, :] + np.einsum("pij,pkj->pki", R, q[large] - centre[:, None, :])
    return q, cls


def case_cuts(name, key, chunk=64):
    """The Cuts of point set `key` of scene `name` of tests/point_query_cases.py, once per session."""
    import point_query_cases as pq
    if (name, key) in _cases:
        return _cases[(name, key)]
    ns = pq.case(name)["ns"]
    seed, cls = seed_triangles(name, key)
    normal, size = tf._normal_and_size(seed)
    P, T = len(seed), len(ns.W)
    c = Cuts()
    c.cls, c.steps, c.clear = cls, np.zeros(P, np.int64), np.zeros(P, bool)
    c.corners, c.member = np.zeros((P, 9), np.float32), np.zeros((P, T), bool)
    kept = {}      # query -> its cuts at the step it came clear (or the last)
    todo = np.arange(P)
    for step in range(MAX_STEPS + 1):
        moved = seed[todo] + (step / 64.0) * (size[todo, None] * normal[todo])[:, None, :]
        corners = moved.reshape(-1, 9).astype(np.float32)
        ok = np.zeros(len(todo), bool)
        for at in range(0, len(todo), chunk):
            rows = slice(at, at + chunk)
            if T:
                member, clear, cuts = classify(ns, corners[rows].astype(np.float64).reshape(-1, 3, 3))
                ok[rows] = clear.all(axis=1)
                c.member[todo[rows]] = member
                for local in range(len(member)):
                    sel = cuts["row"] == local
                    kept[int(todo[at + local])] = {k: v[sel] for k, v in cuts.items()}
            else:
                ok[rows] = True
        c.corners[todo], c.steps[todo], c.clear[todo] = corners, step, ok
        todo = todo[~ok]
        if not len(todo):
            break
    empty = dict(row=np.zeros(0, np.int64), col=np.zeros(0, np.int64), a=np.zeros((0, 3)), b=np.zeros((0, 3)), fa=np.zeros(0, np.int64), fb=np.zeros(0, np.int64), ba=np.zeros(0), bb=np.zeros(0))
    per = [kept.get(i, empty) for i in range(P)]
    c.cuts = {k: np.concatenate([p[k] for p in per]) if P else empty[k] for k in empty}
    c.cuts["row"] = np.concatenate([np.full(len(p["col"]), i, np.int64) for i, p in enumerate(per)]) if P else empty["row"]
    _cases[(name, key)] = c
    return c


def expected_keys(ns, member, k):
    """The keys [P, k, 3] uint32 (found, objectIndex, triIndex) of the member sets in the key's order: ns.W's rows are in it (by
    object, then by triangle)."""
    out = np.zeros((member.shape[0], k, 3), np.uint32)
    for i in range(member.shape[0]):
        cols = np.flatnonzero(member[i])[:k]
        out[i, :len(cols)] = np.stack([np.ones(len(cols), np.uint32), ns.obj[cols].astype(np.uint32), ns.tri[cols].astype(np.uint32)], axis=1)
    return out


def seed_corners(name, key):
    """The seeded queries as the entry points take them ([P, 9] float32), before any steering: what the GPU tests ask about."""
    return seed_triangles(name, key)[0].reshape(-1, 9).astype(np.float32)


# ---- closure: not float64, but shared by the CPU and the GPU tests
def closure_queries(name, n=384):
    """Small seeded query triangles about points of the closed mesh `name` of tests/side_cases.py: (scene, corners [n, 9])."""
    import nearest_float64 as nf
    import point_query_cases as pq
    import side_cases
    scene = side_cases.build_scene(name)
    ns = nf.NearestScene.from_numpy(pq.arrays_to_numpy(scene.arrays()))
    rng = np.random.default_rng(9800 + side_cases.SCENES.index(name))
    t = ns.W[rng.integers(0, len(ns.W), n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    centre = (t * w[:, :, None]).sum(axis=1)
    edge = np.linalg.norm(t[:, 1] - t[:, 0], axis=1)
    shape = rng.normal(size=(n, 3, 3))
    shape /= np.linalg.norm(shape, axis=2, keepdims=True)
    return scene, (centre[:, None, :] + rng.uniform(0.3, 1.2, (n, 1, 1)) * edge[:, None, None] * shape).reshape(-1, 9).astype(np.float32)


def check_closure(recs, counts):
    """On the queries with 1..8 cuts: every end on a scene edge whose partner end carries another feature occurs exactly twice,
    bit for bit, among the query's cuts, and chain_cuts joins the cuts into chains that end on the query's own edges only.
    Returns how many queries and shared ends were looked at."""
    looked, shared = 0, 0
    for i in np.flatnonzero((counts > 0) & (counts <= 8)):
        r = recs[i, :counts[i]]
        assert (r["found"] == 1).all()
        ends = np.concatenate([r["a"], r["b"]]).view(np.uint32)
        feats = np.concatenate([r["featA"], r["featB"]])
        partner = np.concatenate([r["featB"], r["featA"]])
        for e in np.flatnonzero((feats >= 3) & (partner != feats)):
            same = int((ends == ends[e]).all(axis=1).sum())
            assert same == 2, f"query {int(i)}: the end {ends[e].view(np.float32).tolist()} on a scene edge occurs {same} times"
            shared += 1
        from ray_tracer_amd import engine
        loops, chains = engine.chain_cuts(r)
        assert sorted(x for c in loops + chains for x in c) == list(range(len(r)))
        for chain in chains:
            ce = np.concatenate([r["a"][chain], r["b"][chain]]).view(np.uint32)
            cf_ = np.concatenate([r["featA"][chain], r["featB"][chain]])
            for e in range(len(ce)):
                if int((ce == ce[e]).all(axis=1).sum()) == 1:    # a loose end of the chain
                    assert cf_[e] < 3, f"query {int(i)}: a chain ends inside the query, on scene edge {int(cf_[e]) - 3}"
        looked += 1
    return looked, shared
