"""The radius point queries restated in numpy float64: for every point the distance to EVERY surface of a scene, the member set
of a reach, and the rule that chooses reaches no primitive is ambiguous under. Support module of tests/test_point_within_host.py
(CPU) and tests/test_point_within.py (GPU). The distances and the per-primitive error bound b(q, t) (C = 64) are
tests/nearest_float64.py's own (sphere_closest, triangle_closest, NearestScene.bound): nothing here is shared with
include/rt_point_within.h, the exhaustive host loop or the kernels.

Semantics restated ("Radius point queries"): a primitive is a member of point q's set under the reach R iff its
distance is < R; the list is the members by ascending distance; the count is their number.

The radius rule
---------------
A float32 distance lies within b of the float64 one, and the float32 test compares squared values against fl(R * R) (a relative
u / 2 on R, far below b). A primitive whose float64 distance lies within its bound of R could fall on either side, so reaches are
chosen where that happens to NO primitive. For a target of m members: sort the point's float64 distances; take the smallest
m' >= m for which R = fl32(midpoint of the m'-th and the (m'+1)-th) is > 0, leaves exactly m' primitives below it, and leaves
every primitive of the scene with |d - R| > 4 b; beyond the last primitive R = fl32(2 d_max + 1), which always qualifies. With
this rule the float64 member set is THE answer for every point: no point is exempt, and the tests assert that
(Reach.clear). Median m' lies between m and m + 3 except on the far sets, where a reach swallows whole objects.
"""
import numpy as np

import nearest_float64 as nf

MARGIN = 4.0      # |d - R| > MARGIN b for every primitive
REC = 48          # sizeof(RtNearest)
MISS_DST = np.float32(99999999.0)

_dist = {}


def case_distances(name, key):
    """The Distances of point set `key` of scene `name` of tests/point_query_cases.py, once per session."""
    import point_query_cases as pq
    if (name, key) not in _dist:
        c = pq.case(name)
        _dist[(name, key)] = Distances(c["ns"], c["sets"][key])
    return _dist[(name, key)]


def raw(recs, n, k):
    """The bytes [n, k, 48] of n * k RtNearest records (a ctypes array, or anything with the buffer protocol)."""
    return np.frombuffer(recs, np.uint8).reshape(n, k, REC) if n * k else np.zeros((n, k, REC), np.uint8)


def is_not_found(record_bytes):
    """Which rows of record bytes [..., 48] are the not-found record: dst = RT_MISS_DST, everything else 0."""
    return (record_bytes[..., :4].copy().view(np.float32)[..., 0] == MISS_DST) & ~record_bytes[..., 4:].any(axis=-1)


class Distances:
    """d [P, N], b [P, N] for the N primitives of a scene (spheres first, then the rows of scene.W), and who they are:
    sphere [N] bool, first [N] (sphere or object index), tri [N]."""

    def __init__(self, scene, points, chunk=128):
        q_all = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
        ns, nt = len(scene.sph_c), len(scene.W)
        self.sphere = np.arange(ns + nt) < ns
        self.first = np.concatenate([scene.sph_index.astype(np.int64), scene.obj.astype(np.int64)])
        self.tri = np.concatenate([np.zeros(ns, np.int64), scene.tri.astype(np.int64)])
        self.d = np.zeros((len(q_all), ns + nt))
        self.b = np.zeros((len(q_all), ns + nt))
        for k in range(0, len(q_all), chunk):
            q = q_all[k:k + chunk]
            qa = np.abs(q).max(axis=1)
            if ns:
                self.d[k:k + chunk, :ns] = nf.sphere_closest(q, scene.sph_c, scene.sph_r)[0]
                self.b[k:k + chunk, :ns] = nf.NEAREST_C * nf.U32 * (qa[:, None] + (np.abs(scene.sph_c).max(axis=1) + scene.sph_r)[None, :])
            if nt:
                d = nf.triangle_closest(q, scene.W)[0]
                self.d[k:k + chunk, ns:] = d
                self.b[k:k + chunk, ns:] = scene.bound(q, d)
        self.W = np.concatenate([np.zeros((ns, 3, 3)), scene.W]) if ns + nt else np.zeros((0, 3, 3))
        self._column = {(bool(s), int(f), int(t)): c for c, (s, f, t) in enumerate(zip(self.sphere, self.first, self.tri))}
        self._cuts = None

    def columns(self, is_sphere, first, tri):
        """The column of each named primitive (flat arrays)."""
        return np.array([self._column[(bool(s), int(f), int(t))] for s, f, t in zip(is_sphere, first, tri)], np.int64).reshape(np.shape(first))

    def cuts(self):
        """For every point and every m' in 0..N: the candidate reach of the rule and whether it qualifies. Computed once."""
        if self._cuts is None:
            P, N = self.d.shape
            order = np.argsort(self.d, axis=1, kind="stable")
            ds, bs = np.take_along_axis(self.d, order, 1), np.take_along_axis(self.b, order, 1)
            R = np.zeros((P, N + 1), np.float32)
            ok = np.zeros((P, N + 1), bool)
            if N:
                R[:, 1:N] = ((ds[:, :-1] + ds[:, 1:]) / 2).astype(np.float32)
                R[:, N] = (2 * ds[:, -1] + 1).astype(np.float32)
                R64 = R.astype(np.float64)
                below = np.maximum.accumulate(ds + MARGIN * bs, axis=1)                       # the highest upper end among the first m'
                above = np.minimum.accumulate((ds - MARGIN * bs)[:, ::-1], axis=1)[:, ::-1]   # the lowest lower end among the rest
                ok[:, 1:N] = (R64[:, 1:N] > 0) & (below[:, :-1] < R64[:, 1:N]) & (R64[:, 1:N] < above[:, 1:])
                ok[:, N] = below[:, -1] < R64[:, N]
                assert ok[:, N].all()
            self._cuts = (R, ok)
        return self._cuts


class Reach:
    """The reaches of the rule for a target of m members: R [P] float32, count [P] (= m'), member [P, N] bool, and clear [P]: no
    primitive within MARGIN bounds of the reach (the rule promises all True)."""

    def __init__(self, dist, m):
        R_all, ok = dist.cuts()
        P, N = dist.d.shape
        if N == 0:
            self.R, self.count = np.ones(P, np.float32), np.zeros(P, np.int64)
        else:
            m = min(m, N)
            self.count = m + np.argmax(ok[:, m:], axis=1)
            self.R = R_all[np.arange(P), self.count]
        R64 = self.R.astype(np.float64)[:, None]
        self.member = dist.d < R64
        self.clear = (np.abs(dist.d - R64) > MARGIN * dist.b).all(axis=1) & (self.R > 0)


def check_listed(dist, points, rec, have, k, what):
    """The float64 rules of point_query_cases.check_records for every LISTED record (rec: nearest_to_numpy of n * k records; have
    [n]: how many of a point's k slots are listed), each against the primitive it names: dst within that primitive's own bound of the
    float64 distance to it; | |point - q| - dst | within it; barycentrics inside the triangle; a sphere's uv and triangle 0; point
    the combination of the named triangle's float64 corners. Returns the column [n, k] of every listed primitive (-1: not listed)."""
    n = len(points)
    listed = np.arange(k)[None, :] < have[:, None]
    r = {key: v.reshape((n, k) + v.shape[1:]) for key, v in rec.items()}
    assert (r["found"][listed] == 1).all() and (r["found"][~listed] == 0).all(), f"{what}: found does not follow the count"
    col = np.full((n, k), -1, np.int64)
    if not listed.any():
        return col
    sph = r["isSphere"][listed].astype(bool)
    col[listed] = dist.columns(sph, r["objectIndex"][listed], r["triIndex"][listed])
    row = np.nonzero(listed)[0]
    d, b = dist.d[row, col[listed]], dist.b[row, col[listed]]
    q = np.asarray(points, np.float32).astype(np.float64)[row]
    dst = r["dst"][listed].astype(np.float64)
    err = np.abs(dst - d)
    assert (err <= b).all(), f"{what}: |dst - float64| up to {float((err / b).max()):.3g} bounds of the named primitive"
    p = r["point"][listed].astype(np.float64)
    gap = np.abs(np.linalg.norm(p - q, axis=1) - dst)
    assert (gap <= b).all(), f"{what}: | |point - q| - dst | up to {float((gap / b).max()):.3g} bounds"
    u, v = r["uv"][listed][:, 0].astype(np.float64), r["uv"][listed][:, 1].astype(np.float64)
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1 + 4 * nf.U32).all(), f"{what}: barycentrics outside the triangle"
    assert (r["uv"][listed][sph] == 0).all() and (r["triIndex"][listed][sph] == 0).all()
    W = dist.W[col[listed]]
    rebuilt = (1 - u - v)[:, None] * W[:, 0] + u[:, None] * W[:, 1] + v[:, None] * W[:, 2]
    off = np.linalg.norm(rebuilt - p, axis=1)[~sph]
    assert (off <= b[~sph]).all(), f"{what}: point is not w a + u b + v c of the named triangle"
    return col


def check_relations(nearest, within, counts, k, what):
    """The stated consequences, bit for bit: `nearest` [n, 48] the bytes of rt_query_nearest's records under the limits R, `within`
    [n, k, 48] (k > 0) and `counts` the radius query's under the same R. count > 0 iff found; out[i k].dst has the bits of the
    nearest query's dst; with count <= k its primitive is in the list; and wherever its primitive is listed, the record is its
    record byte for byte."""
    n = len(nearest)
    found = nearest[:, 4] != 0
    assert np.array_equal(counts > 0, found), f"{what}: count > 0 is not rt_query_nearest's found"
    assert np.array_equal(within[:, 0, :4], nearest[:, :4]), f"{what}: out[i k].dst has not the bits of rt_query_nearest's dst"
    same = (within[:, :, 8:20] == nearest[:, None, 8:20]).all(axis=2) & (within[:, :, 4] == 1)      # isSphere, objectIndex, triIndex
    listed = same.any(axis=1)
    assert listed[found & (counts <= k)].all(), f"{what}: rt_query_nearest's primitive is not in the list"
    at = np.argmax(same, axis=1)
    assert np.array_equal(within[np.arange(n), at][listed], nearest[listed]), f"{what}: rt_query_nearest's record is not the list's, byte for byte"
