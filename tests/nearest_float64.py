"""The point queries restated in numpy float64: the distance from a point to every surface of a scene, by brute force. Nothing here
is shared with include/rt_point_query.h, the exhaustive host loop or the kernel: it reads Scene.numpy() with a reader of its own,
places every corner with the object's forward matrix in float64, and measures a triangle by another route than the header's region
classification: the foot of the perpendicular where it falls inside the triangle (three signed areas), else the nearest of the three
edges, each a clamped projection.

Semantics restated ("Point queries"): the surfaces are every sphere with radius > 0 and every triangle of every object
under the object's forward matrix; Euclidean world distance; no frontOnly, materials or alpha maps; with a limit T the answer
exists iff the distance is < T.

The error bound of the float32 answer
-------------------------------------
u = 2^-24. Write |q| for the largest |coordinate| of the point and |M||[v;1]| for the largest component of |M| |[v; 1]| over the
corners v of a triangle (|c| + r for a sphere): the magnitudes the roundings scale with. Only the forward matrix enters: the
inverse is used for pruning alone. For one triangle, float32 does this (rt_xform_point, rt_point_triangle), to first order in u:

  1. world corners, a row of three products and three sums each: |fl(M v) - M v| <= 3 u |M||[v;1]| per component, sqrt(3) times
     that as a vector: 5.2 u |M||[v;1]|. Moving a triangle's corners by e moves its distance from q by at most e.
  2. the barycentrics (u, v) by the region tests: whatever their error, they satisfy u, v >= 0 and u + v <= 1 up to 2 u, so the point
     p^ = (1 - u - v) a + u b + v c they stand for lies in the triangle (or 2 u |corners| outside): |q - p^| >= d - 2 u |M||[v;1]|.
  3. p = fl(w a + u b + v c) with w = fl(fl(1 - u) - v): w carries 2 u, each product 1 u, the two sums 1 u each of a partial sum
     no larger than the corners: <= 6 u |M||[v;1]| per component, sqrt(3) * 6 = 10.4 u as a vector.
  4. |q - p|^2: the subtraction 1 u (|q| + |p|) per component, sqrt(3) as a vector: 1.8 u (|q| + |M||[v;1]|); three squares and two
     sums 2.5 u relative on the square, the root halves that and adds 0.5 u: 1.75 u d, and d <= sqrt(3) (|q| + |p|): 3.1 u (...).
  So from below the float32 distance misses d by at most 5.2 + 2 + 10.4 + 1.8 + 3.1 = 22.5 u (|q| + |M||[v;1]|): p^ is a point of
  the triangle, wherever. (This side is all the traversal's pruning needs: DESIGN.md.)
  5. From above, p^ also has to be near the true closest point p*. In a vertex region it is the vertex. In an edge region
     t = d1 / (d1 - d3) with d1 = ab . ap, d3 = ab . bp: the differences carry 1 u per component, a dot 3 more on its products and
     2 on its sums: |delta d| <= 5 u |ab| |ap|, so |delta t| |ab| <= 10 u R with R the largest distance from q to a corner,
     and the same again for a point that the rounding of d1, d3 puts into a neighbouring vertex region: 20 u R, R <= sqrt(3)
     (|q| + |M||[v;1]|): 35 u (|q| + |M||[v;1]|).
  C = 64 >= 22.5 + 35 covers every region but the face; a sphere needs 10 (a difference, a dot, a root, a difference).
  6. In the face region u = vb / (va + vb + vc), each v* a difference of two products of two dots: 11 u |ab| |ac| R^2 a product,
     23 u |ab| |ac| R^2 a v*, 71 u the sum (= |n|^2, n = ab x ac), so |delta u|, |delta v| <= 94 u |ab| |ac| R^2 / |n|^2 and
     p^ lies within t = min(L, 94 u k R^2) of p*, k = |ab| |ac| (|ab| + |ac|) / |n|^2, L the longest edge (p^ is in the triangle).
     That is no multiple of u (|q| + |M||[v;1]|): the barycentrics of a thin triangle are ill-conditioned where the distance is not.
     Off the plane it enters at second order, |q - p^| = sqrt(d^2 + t^2) <= d + t min(1, t / 2 d). The bound carries it as a term of
     its own, F(q, t) = t min(1, t / 2 d), beside the multiple of u: a count of its own (94), not C's.

  b(q, t) = C u (|q| + |M||[v;1]|) + F(q, t), C = 64 (F is 0 for spheres and zero-area triangles; for the well-shaped triangles of
  the test scenes it is below a tenth of the first term except on the surface sets, where d ~ 0 and it is first order).
  C is derived, not fitted: tests/test_point_queries_host.py prints the largest observed |d_float32 - d_float64| / (b / C) per
  point set and asserts C >= twice the worst, that is, that no error is above half its bound. Observed with
  rt_nearest_exhaustive_host: OBSERVED below (the worst of a scene is on its far set each time, where the root of a squared
  distance of 1e6 carries most of the error; on the surface sets, where F matters, the worst is 1.05).

The float32 answer is min over primitives of a value within b(q, t) of the true d(q, t), so it lies in
[min_t (d - b), min_t (d + b)]: `bound` is the larger distance of those two ends from min_t d, and a primitive can be the reported one
iff d(q, t) - b(q, t) <= min_t (d + b). No point is excluded as ill-conditioned: a distance is a Lipschitz function of the point.
"""
import numpy as np

U32 = 2.0 ** -24
NEAREST_C = 64.0
# largest |d32 - d64| / bound(C = 1) of rt_nearest_exhaustive_host, per scene over its four point sets (uniform, surface, vertices, far)
OBSERVED = {"cornell": 1.47, "spheres": 1.97, "cornell_bunny": 1.16, "instances": 1.93, "placed150": 1.91, "deep": 1.54}


class NearestScene:
    def __init__(self):
        self.sph_c = np.zeros((0, 3)); self.sph_r = np.zeros(0); self.sph_index = np.zeros(0, np.int64)
        self.W = np.zeros((0, 3, 3))          # world corners of every (object, triangle) pair
        self.mag = np.zeros(0)                # |M||[v;1]| of the pair
        self.kappa = np.zeros(0); self.longest = np.zeros(0)   # k and L of (6) in the module docstring
        self.obj = np.zeros(0, np.int64); self.tri = np.zeros(0, np.int64)
        self.tri_count = 0                    # triangles of the scene's arrays

    @classmethod
    def from_numpy(cls, arrays):
        s = cls()
        sp = arrays["spheres"]
        if len(sp):
            f = sp.view(np.float32).reshape(len(sp), -1).astype(np.float64)
            keep = f[:, 3] > 0                                                 # the zeroed slots of the table are no surface
            s.sph_c, s.sph_r, s.sph_index = f[keep, 0:3], f[keep, 3], np.nonzero(keep)[0]
        ob = arrays["objects"]
        if not len(ob):
            return s
        tp = arrays["triPoints"].view(np.float32).reshape(-1, 8)[:, 0:3].astype(np.float64)
        tr = arrays["triangles"].view(np.uint32).reshape(len(arrays["triangles"]), -1)[:, 0:3].astype(np.int64)
        s.tri_count = len(tr)
        nodes = arrays["bvhNodes"].view(np.uint32).reshape(len(arrays["bvhNodes"]), -1)[:, 6:8]
        of, ou = ob.view(np.float32).reshape(len(ob), -1), ob.view(np.uint32).reshape(len(ob), -1)
        W, mag, oi, ti, by_root = [], [], [], [], {}
        for i in range(len(ob)):
            root = int(ou[i, 17])
            if root not in by_root:
                tris, stack = [], [root]
                while stack:
                    index, count = nodes[stack.pop()]
                    if count:
                        tris.extend(range(int(index), int(index) + int(count)))
                    else:
                        stack += [int(index), int(index) + 1]
                by_root[root] = np.array(sorted(tris), np.int64)
            t = by_root[root]
            M = of[i, 0:16].astype(np.float64).reshape(4, 4).T                # column-major m[c * 4 + r]
            v = tp[tr[t]]                                                      # [T, 3 corners, 3]
            W.append(v @ M[:3, :3].T + M[:3, 3])
            mag.append((np.abs(v) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])).max(axis=(1, 2)))
            oi.append(np.full(len(t), i, np.int64)); ti.append(t)
        s.W, s.mag, s.obj, s.tri = np.concatenate(W), np.concatenate(mag), np.concatenate(oi), np.concatenate(ti)
        ab, ac, bc = s.W[:, 1] - s.W[:, 0], s.W[:, 2] - s.W[:, 0], s.W[:, 2] - s.W[:, 1]
        e1, e2, nn = np.linalg.norm(ab, axis=1), np.linalg.norm(ac, axis=1), (np.cross(ab, ac) ** 2).sum(axis=1)
        s.kappa = np.where(nn > 0, e1 * e2 * (e1 + e2) / np.where(nn > 0, nn, 1.0), 0.0)
        s.longest = np.maximum(np.maximum(e1, e2), np.linalg.norm(bc, axis=1))
        return s

    def bound(self, q, d, rows=None, C=None):
        """b(q, t) for points q [P, 3] and the triangles `rows` (all: [P, T]; else one row per point: [P]), d their distances."""
        C = NEAREST_C if C is None else C
        qa = np.abs(q).max(axis=1)
        if rows is None:
            R = np.linalg.norm(q[:, None, None, :] - self.W[None], axis=-1).max(axis=-1)
            mag, kappa, longest, qa = self.mag[None, :], self.kappa[None, :], self.longest[None, :], qa[:, None]
        else:
            R = np.linalg.norm(q[:, None, :] - self.W[rows], axis=-1).max(axis=-1)
            mag, kappa, longest = self.mag[rows], self.kappa[rows], self.longest[rows]
        t = np.minimum(longest, 94.0 * U32 * kappa * R * R)
        second = np.where(d > 0, np.minimum(1.0, t / (2.0 * np.where(d > 0, d, 1.0))), 1.0)
        return C * U32 * (qa + mag) + t * second


    def box(self):
        """The box of every surface (lo, hi)."""
        pts = [self.W.reshape(-1, 3)] if len(self.W) else []
        if len(self.sph_c):
            pts += [self.sph_c - self.sph_r[:, None], self.sph_c + self.sph_r[:, None]]
        p = np.concatenate(pts)
        return p.min(axis=0), p.max(axis=0)


def _segment(q, a, b):
    """Closest point of segments a-b [T, 3] to points q [P, 1, 3]: a clamped projection. A segment that is a point gives it."""
    ab = b - a
    den = np.einsum("tk,tk->t", ab, ab)
    t = np.einsum("ptk,tk->pt", q - a, ab) / np.where(den > 0, den, 1.0)
    t = np.clip(np.where(den > 0, t, 0.0), 0.0, 1.0)
    return a + t[..., None] * ab


def triangle_closest(q, W):
    """Distance [P, T] and closest point [P, T, 3] from points q [P, 3] to triangles W [T, 3, 3]."""
    a, b, c = W[:, 0], W[:, 1], W[:, 2]
    qq = q[:, None, :]
    best_p = _segment(qq, a, b)
    best = np.linalg.norm(qq - best_p, axis=-1)
    for s0, s1 in ((a, c), (b, c)):
        p = _segment(qq, s0, s1)
        d = np.linalg.norm(qq - p, axis=-1)
        closer = d < best
        best, best_p = np.where(closer, d, best), np.where(closer[..., None], p, best_p)
    n = np.cross(b - a, c - a)
    nn = np.einsum("tk,tk->t", n, n)
    ok = nn > 0
    nsafe = np.where(ok, nn, 1.0)
    h = np.einsum("ptk,tk->pt", qq - a, n) / nsafe                    # q = foot + h n
    foot = qq - h[..., None] * n
    # the foot is inside iff the three sub-triangles turn the way the triangle does
    sa = np.einsum("ptk,tk->pt", np.cross(b - foot, c - foot), n)
    sb = np.einsum("ptk,tk->pt", np.cross(c - foot, a - foot), n)
    sc = np.einsum("ptk,tk->pt", np.cross(a - foot, b - foot), n)
    inside = ok & (sa >= 0) & (sb >= 0) & (sc >= 0)
    dface = np.abs(h) * np.sqrt(nsafe)
    use = inside & (dface < best)
    return np.where(use, dface, best), np.where(use[..., None], foot, best_p)


def sphere_closest(q, c, r):
    d = q[:, None, :] - c
    l = np.linalg.norm(d, axis=-1)
    unit = np.where(l[..., None] > 0, d / np.where(l > 0, l, 1.0)[..., None], np.array([1.0, 0.0, 0.0]))
    return np.abs(l - r), c + r[:, None] * unit


def nearest(scene, points, C=NEAREST_C, chunk=256):
    """Per point: dst (the minimum distance), point (the closest point), kind / index of a minimiser (1: sphere index, 0: row of
    scene.W), bound (see the module docstring), unit (b / C of the minimiser: what the observed ratios are taken against), upper (min_t d + b) and candidates (how many primitives can be the reported one)."""
    q_all = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    P = len(q_all)
    res = dict(dst=np.full(P, np.inf), point=np.zeros((P, 3)), sphere=np.zeros(P, bool), index=np.zeros(P, np.int64),
               bound=np.zeros(P), unit=np.zeros(P), upper=np.full(P, np.inf), candidates=np.zeros(P, np.int64))
    for k in range(0, P, chunk):
        q = q_all[k:k + chunk]
        qa = np.abs(q).max(axis=1)
        ds, ps, bs, sph = [], [], [], []
        if len(scene.sph_c):
            d, p = sphere_closest(q, scene.sph_c, scene.sph_r)
            ds.append(d); ps.append(p); sph.append(np.ones(d.shape[1], bool))
            bs.append(C * U32 * (qa[:, None] + (np.abs(scene.sph_c).max(axis=1) + scene.sph_r)[None, :]))
        if len(scene.W):
            d, p = triangle_closest(q, scene.W)
            ds.append(d); ps.append(p); sph.append(np.zeros(d.shape[1], bool))
            bs.append(scene.bound(q, d, C=C))
        if not ds:
            continue
        d, p, b, is_sph = np.concatenate(ds, 1), np.concatenate(ps, 1), np.concatenate(bs, 1), np.concatenate(sph)
        j = d.argmin(axis=1)
        rows = np.arange(len(q))
        ref, lower, upper = d[rows, j], (d - b).min(axis=1), (d + b).min(axis=1)
        sl = slice(k, k + len(q))
        res["dst"][sl], res["point"][sl], res["sphere"][sl] = ref, p[rows, j], is_sph[j]
        res["index"][sl] = np.where(is_sph[j], j, j - int(is_sph.sum()))
        res["bound"][sl], res["upper"][sl] = np.maximum(ref - lower, upper - ref), upper
        res["unit"][sl] = b[rows, j] / C                      # bound(C = 1) of the minimiser: what the observed ratios are taken against
        res["candidates"][sl] = (d - b <= upper[:, None]).sum(axis=1)
    return res


def distance_to_reported(scene, points, is_sphere, object_index, tri_index, C=NEAREST_C):
    """The float64 distance from each point to the primitive a record names, that primitive's own bound b(q, t), its world corners
    [P, 3, 3] (zeros for a sphere) and its mag."""
    q = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    P = len(q)
    d, b, W = np.zeros(P), np.zeros(P), np.zeros((P, 3, 3))
    qa = np.abs(q).max(axis=1)
    key = {(int(o), int(t)): r for r, (o, t) in enumerate(zip(scene.obj, scene.tri))}
    slot = {int(i): r for r, i in enumerate(scene.sph_index)}
    for i in range(P):
        if is_sphere[i]:
            r = slot[int(object_index[i])]
            d[i] = sphere_closest(q[i:i + 1], scene.sph_c[r:r + 1], scene.sph_r[r:r + 1])[0][0, 0]
            b[i] = C * U32 * (qa[i] + np.abs(scene.sph_c[r]).max() + scene.sph_r[r])
        else:
            r = key[(int(object_index[i]), int(tri_index[i]))]
            d[i] = triangle_closest(q[i:i + 1], scene.W[r:r + 1])[0][0, 0]
            b[i] = scene.bound(q[i:i + 1], d[i:i + 1], np.array([r]), C=C)[0]
            W[i] = scene.W[r]
    return d, b, W
