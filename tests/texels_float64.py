"""A float64 restatement of the lightmap texel rule by another route ("Lightmap texels"), to hold
rt_texels_exhaustive_host to: no snapping and no integers, but point-in-triangle by signed distances in texel units from the
unsnapped uvs, and the record's point and normal by float64 interpolation and transform.

Coverage. In texel units a uv corner is P = (u W, (1 - v) H) and the centre of texel (x, y) is (x + 0.5, y + 0.5). The rule snaps
each corner to the nearest point of a grid of pitch 1 / 256: both products are exact in a double (24 bits by at most 21; 1 - v is
rounded once, to within 2^-53), so the only error is that rounding, at most 1 / 512 along each axis, sqrt(2) / 512 = 0.00276 texel
as a distance. Every point of a snapped edge is then within that distance of the true edge, so the true triangle shrunk by it lies
inside the snapped one and the snapped one inside the true one grown by it. With m = 1 / 256 = 0.0039 > 0.00276:
  - a centre more than m inside a triangle (all three signed line distances > m) is strictly inside its snapped triangle: covered;
  - a centre more than m away from a triangle is outside its snapped triangle, edges included: not covered by it;
  - anything else is ambiguous for that triangle.
A texel is IN when some triangle certainly covers it, OUT when every non-skipped triangle certainly does not, and ambiguous
otherwise; the owner of any covered texel must be a triangle that does not certainly miss it, and no triangle with a lower index
may certainly cover it. Skipped here: a uv that is not finite or beyond 2^27 sub-texels. A triangle without area is never IN (its
signed distances are not used), only near or far.

The record. With the record's fp32 barycentrics (u, v) and w = 1 - u - v in float64:
  - uv: the exact barycentrics of the centre in the snapped triangle reproduce the centre; with the true corners in their place the
    point moves by a convex combination of the corners' snapping moves, at most sqrt(2) / 512 < 1 / 256 texel; the record's u and v
    are each rounded once to fp32 (the double quotient's own error is 2^-29 of that), so the point moves by at most a further
    U (u |P1 - P0| + v |P2 - P0|) <= U (|P1 - P0| + |P2 - P0|), U = 2^-24. Bound: 1 / 256 + U (|P1 - P0| + |P2 - P0|) texel.
  - point: a world corner is rt_xform_point: three products and three sums, at most 4 U S per component, S = sum |m_ij| |a_j| + |t_i|
    (to first order); w = (1 - u) - v in fp32 adds 2 U; the combination w a + u b + v c is three products and two sums: 3 U S.
    A convex combination does not grow S. Bound per component: 10 U S_max over the three corners (9 counted, 1 for second order).
  - normal: n_i = (n0 w + n1 u) + n2 v per component: 2 U for w, three products, two sums: e_n <= 6 U (|n0| + |n1| + |n2|);
    g = fwd x n_i: e_g <= |M| e_n + 3 U |M| |n_i|; normalising (dot: 3 roundings, sqrt, reciprocal, scale: 6 U of relative error
    on the length at most) gives |normal - g / |g|| <= 2 |e_g| / |g| + 6 U. Texels whose float64 |g| is below 1e-3 of |M| |n| are left
    out (the bound says nothing there; the soup's zero-sum triangle has some).
"""
import numpy as np

U = 2.0 ** -24
M_TEXEL = 1.0 / 256.0
IN, NEAR, FAR = 2, 1, 0


def corners(uv, width, height):
    """(n, 3, 2) fp32 uvs -> corners in texel units (float64) and the mask of triangles the rule does not skip for their values"""
    uv = np.asarray(uv, np.float32).astype(np.float64)
    P = np.stack([uv[..., 0] * width, (1.0 - uv[..., 1]) * height], -1)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(P).all(axis=(1, 2)) & (np.abs(P) * 256 < 2.0 ** 27 - 1).all(axis=(1, 2))
    return P, ok


def _segment_distance(c, a, b):
    ab = b - a
    L2 = float(ab @ ab)
    t = np.clip(((c - a) @ ab) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(c))
    return np.linalg.norm(c - (a + t[:, None] * ab), axis=1)


def classify(P, ok, width, height):
    """-> (n_triangles, n_texels) uint8 of IN / NEAR / FAR per triangle and texel centre (skipped triangles: FAR)"""
    ys, xs = np.divmod(np.arange(width * height), width)
    c = np.stack([xs + 0.5, ys + 0.5], -1)
    cls = np.zeros((len(P), len(c)), np.uint8)
    for t in np.flatnonzero(ok):
        a, b, d = P[t]
        area = (b[0] - a[0]) * (d[1] - a[1]) - (d[0] - a[0]) * (b[1] - a[1])
        dist = np.minimum(np.minimum(_segment_distance(c, a, b), _segment_distance(c, b, d)), _segment_distance(c, d, a))
        depth = np.full(len(c), -1.0)
        scale = max(np.abs(P[t]).max(), 1.0) ** 2
        if abs(area) > 1e-12 * scale:
            s = 1.0 if area > 0 else -1.0
            sd = []
            for p, q in ((a, b), (b, d), (d, a)):
                e = q - p
                sd.append(s * (e[0] * (c[:, 1] - p[1]) - e[1] * (c[:, 0] - p[0])) / np.linalg.norm(e))
            depth = np.minimum(np.minimum(sd[0], sd[1]), sd[2])
        cls[t] = np.where(depth > M_TEXEL, IN, np.where((depth <= 0) & (dist > M_TEXEL), FAR, NEAR))
    return cls


def record_bounds(P, uvw, tri, pos, nrm, matrix, identity):
    """For covered texels with owners `tri` (indices into the object's triangles) and fp32 barycentrics uvw (k, 2): the float64
    uv point in texel units with its bound, the point with its bound, the normal with its bound (nan where |g| is too small)."""
    u, v = uvw[:, 0].astype(np.float64), uvw[:, 1].astype(np.float64)
    w = 1.0 - u - v
    T = P[tri]
    where = w[:, None] * T[:, 0] + u[:, None] * T[:, 1] + v[:, None] * T[:, 2]
    b_uv = M_TEXEL + U * (np.linalg.norm(T[:, 1] - T[:, 0], axis=1) + np.linalg.norm(T[:, 2] - T[:, 0], axis=1))
    M3, t3 = matrix[:3, :3], matrix[:3, 3]
    a = pos[tri].astype(np.float64)                                     # (k, 3 corners, 3)
    world = a if identity else a @ M3.T + t3
    S = np.abs(a) if identity else np.abs(a) @ np.abs(M3).T + np.abs(t3)
    point = w[:, None] * world[:, 0] + u[:, None] * world[:, 1] + v[:, None] * world[:, 2]
    b_point = 10 * U * S.max(axis=1)
    n = nrm[tri].astype(np.float64)
    ni = w[:, None] * n[:, 0] + u[:, None] * n[:, 1] + v[:, None] * n[:, 2]
    g = ni @ M3.T
    e_n = 6 * U * np.abs(n).sum(axis=1)
    e_g = e_n @ np.abs(M3).T + 3 * U * (np.abs(ni) @ np.abs(M3).T)
    glen = np.linalg.norm(g, axis=1)
    size = np.linalg.norm(np.abs(n).sum(axis=1) @ np.abs(M3).T, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = g / glen[:, None]
        b_normal = 2 * np.linalg.norm(e_g, axis=1) / glen + 6 * U
    short = ~(glen > 1e-3 * size)
    normal[short] = np.nan
    b_normal[short] = np.nan
    return where, b_uv, point, b_point, normal, b_normal


def tex_index(coord, size):
    """rt_tex_index under REPEAT in fp32: floor(coord * size) mod size"""
    f = (np.asarray(coord, np.float32) * np.float32(size)).astype(np.float32)
    return np.mod(np.floor(f).astype(np.int64), size)


def hit_uv(uv, tri, bu, bv, bw):
    """hit_uv's arithmetic in fp32: (bw uv0 + bu uv1) + bv uv2 per component"""
    T = np.asarray(uv, np.float32)[tri]
    bu, bv, bw = (np.asarray(x, np.float32)[:, None] for x in (bu, bv, bw))
    return ((bw * T[:, 0]).astype(np.float32) + (bu * T[:, 1]).astype(np.float32)).astype(np.float32) + (bv * T[:, 2]).astype(np.float32)
