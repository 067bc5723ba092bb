"""The sphere sweeps restated in numpy float64: the first time a ball whose centre moves along o + t d comes within R of a surface
of the scene, by brute force. Nothing here is shared with include/rt_sweep.h, the exhaustive host loop or the kernel: the scene is
nearest_float64.NearestScene (its own reader, corners placed in float64), and the time comes by another route than the header's
slab, balls and cylinders:

  - a triangle is a convex set, so g(t) = dist(o + t d, triangle) is a convex function of t, differentiable outside the triangle
    with g'(t) = d . (c - p) / |c - p| (p the closest point). g(0) <= R: the time is 0. Else Newton's iteration on g(t) = R from
    t = 0: the tangent of a convex function lies below it, so no step passes the first root, the iterates rise towards it, and an
    iterate with g > R and g' >= 0 proves that there is none. The distance itself is measured as nearest_float64 measures it (the
    foot of the perpendicular where it falls inside, else the nearest of the three clamped edge projections);
  - a sphere of radius r is a shell: the contact times are those with r - R <= |o + t d - c| <= r + R, two textbook quadratics about o.

Triangles whose bounding ball the line passes by more than R, or that lie behind the origin, are left out before the iteration.

The bracket, and its two bounds
-------------------------------
The first-contact time never increases with the radius. So for a bound delta on everything that separates the fp32 rule's idea
of "within R" from the exact one, the fp32 answer must be found where float64 finds a contact at R - delta, must not be found
where float64 finds none at R + delta, and its t must lie in [t64(R + delta) - tau, t64(R - delta) + tau].

u = 2^-24. S = |o|_inf + M + R is the scale of a ray: M the largest |M||[v;1]| of the scene (nearest_float64's magnitude; |c| + r of
a sphere), so a contact's centre has |coordinates| <= M + R, its step t d = centre - o has <= S, and every magnitude below is <= S.

delta = 100 u S:
   48 u S  sigma itself: an accepted centre's fp32 distance is at most R + sigma, sigma = RT_SWEEP_SIGMA x (the largest
           |coordinate| of the centre, the corners and t d) <= 48 u S;
   45 u S  the fp32 distance falls below the exact distance of the exact triangle by at most 22.5 u (|q| + |M||[v;1]|)
           (nearest_float64's items 1 to 4, the side the pruning uses), |q| and |M||[v;1]| each <= S;
    7 u S  the centre fl(o + t d) against o + t d: one product and one sum per component, u (|t d| + |c|), sqrt(3) as a vector:
           3.5 u (|t d| + |c|).
   From the other side (a true contact at R - delta is found): the candidate's chain is counted in DESIGN.md ("Sphere sweeps") at
   12 u S as a distance, rt_point_triangle's answer exceeds the exact distance by at most 35 u (|q| + |M||[v;1]|) <= 70 u S off the
   face region (nearest_float64's item 5) and the centre moves by the same 7 u S: the fp32 distance at the candidate is at most
   R - delta + 89 u S < R + sigma, so it is accepted. The face term F(q, t) of item 6 stands aside: it is second order off the
   plane, and the well-shaped triangles of the test scenes keep it below the rest.
tau = 8 u (t + (R + E) / |d|), E the scene's extent: t = fl(s -+ half) is one subtraction of two terms no larger than t + the half
   chord, and a half chord is at most (R + E) / |d|; s and the half chord carry 3 roundings each that move the centre ALONG the
   line (what moves it across is in delta).

OBSERVED holds the largest (t - t64(R - delta)) / tau and (t64(R + delta) - t) / tau of rt_sweep_exhaustive_host per scene over its
four ray sets (0: inside the bracket without tau; the value itself is reached by starts in contact, where all three times are 0),
and the largest (gap - R) / delta (0.48 is sigma over delta).
"""
import numpy as np

U32 = 2.0 ** -24
DELTA_C = 100.0
TAU_C = 8.0
# (late, early, gap): the largest (t - t64(R - delta)) / tau, (t64(R + delta) - t) / tau and (gap - R) / delta of rt_sweep_exhaustive_host
OBSERVED = {"cornell": (0, 0, 0.266), "spheres": (0, 0, 0.0255), "cornell_bunny": (0, 0, 0.463), "instances": (0, 0, 0.463), "placed150": (0, 0, 0.408), "deep": (0, 0, 0.478)}


def _segment(q, a, b):
    ab = b - a
    den = np.einsum("nk,nk->n", ab, ab)
    t = np.einsum("nk,nk->n", q - a, ab) / np.where(den > 0, den, 1.0)
    t = np.clip(np.where(den > 0, t, 0.0), 0.0, 1.0)
    return a + t[:, None] * ab


def triangle_closest_pairs(q, W):
    """Distance [N] and closest point [N, 3] from point q[i] to triangle W[i]."""
    a, b, c = W[:, 0], W[:, 1], W[:, 2]
    best_p = _segment(q, a, b)
    best = np.linalg.norm(q - best_p, axis=1)
    for s0, s1 in ((a, c), (b, c)):
        p = _segment(q, s0, s1)
        d = np.linalg.norm(q - p, axis=1)
        closer = d < best
        best, best_p = np.where(closer, d, best), np.where(closer[:, None], p, best_p)
    n = np.cross(b - a, c - a)
    nn = np.einsum("nk,nk->n", n, n)
    ok = nn > 0
    nsafe = np.where(ok, nn, 1.0)
    h = np.einsum("nk,nk->n", q - a, n) / nsafe
    foot = q - h[:, None] * n
    sa = np.einsum("nk,nk->n", np.cross(b - foot, c - foot), n)
    sb = np.einsum("nk,nk->n", np.cross(c - foot, a - foot), n)
    sc = np.einsum("nk,nk->n", np.cross(a - foot, b - foot), n)
    inside = ok & (sa >= 0) & (sb >= 0) & (sc >= 0)
    dface = np.abs(h) * np.sqrt(nsafe)
    use = inside & (dface < best)
    return np.where(use, dface, best), np.where(use[:, None], foot, best_p)


def _newton(o, d, R, W, iters=400):
    """First t >= 0 with dist(o + t d, W) <= R per pair, +inf where there is none."""
    N = len(o)
    t, out, act = np.zeros(N), np.full(N, np.inf), np.arange(N)
    for _ in range(iters):
        if not len(act):
            break
        c = o[act] + t[act, None] * d[act]
        g, p = triangle_closest_pairs(c, W[act])
        tol = 1e-13 * (1.0 + np.abs(o[act]).max(axis=1) + np.abs(c).max(axis=1))     # float64's own noise on g
        hit = g <= R[act] + tol
        out[act[hit]] = t[act[hit]]
        gp = np.einsum("nk,nk->n", c - p, d[act]) / np.where(g > 0, g, 1.0)
        go = ~hit & (gp < 0)
        t[act[go]] += ((g - R[act]) / -np.where(go, gp, -1.0))[go]
        act = act[go]
    assert not len(act), f"{len(act)} pairs did not settle"
    return out


def first_contact(ns, origins, dirs, radius, chunk=64):
    """t64(R) per ray: the first t >= 0 at which o + t d is within R of a surface of `ns`, +inf where it never is."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    R = np.asarray(radius, np.float64).reshape(-1)
    P = len(o)
    best = np.full(P, np.inf)
    dd = np.einsum("pk,pk->p", d, d)
    for c, r in zip(ns.sph_c, ns.sph_r):
        m = o - c
        b, mm = np.einsum("pk,pk->p", m, d), np.einsum("pk,pk->p", m, m)
        disc = b * b - dd * (mm - (r + R) ** 2)
        sq = np.sqrt(np.maximum(disc, 0.0))
        a0, a1 = (-b - sq) / dd, (-b + sq) / dd
        disci = b * b - dd * (mm - (r - R) ** 2)
        sqi = np.sqrt(np.maximum(disci, 0.0))
        b0, b1 = (-b - sqi) / dd, (-b + sqi) / dd
        inside = (r > R) & (disci > 0) & (b0 < 0) & (b1 > 0)
        t = np.where((disc < 0) | (a1 < 0), np.inf, np.where(a0 >= 0, a0, np.where(inside, b1, 0.0)))
        best = np.minimum(best, t)
    if len(ns.W):
        cen = ns.W.mean(axis=1)
        rad = np.linalg.norm(ns.W - cen[:, None, :], axis=2).max(axis=1)
        dn = d / np.sqrt(dd)[:, None]
        for k in range(0, P, chunk):
            sl = slice(k, min(k + chunk, P))
            m = cen[None, :, :] - o[sl, None, :]
            s = np.einsum("ptk,pk->pt", m, dn[sl])
            mm = np.einsum("ptk,ptk->pt", m, m)
            reach = R[sl, None] + rad[None, :]
            keep = (mm - s * s <= reach * reach + 1e-9 * mm + 1e-12) & (s >= -reach * 1.000001)
            pi, ti = np.nonzero(keep)
            if not len(pi):
                continue
            t = _newton(o[sl][pi], d[sl][pi], R[sl][pi], ns.W[ti])
            np.minimum.at(best, pi + k, t)
    return best


def magnitude(ns):
    m = [ns.mag.max()] if len(ns.mag) else []
    if len(ns.sph_c):
        m.append((np.abs(ns.sph_c).max(axis=1) + ns.sph_r).max())
    return float(max(m))


def extent(ns):
    lo, hi = ns.box()
    return float((hi - lo).max())


def delta(ns, origins, radius):
    """The bound on what separates the fp32 rule's "within R" from the exact one, per ray (module docstring)."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    return DELTA_C * U32 * (np.abs(o).max(axis=1) + magnitude(ns) + np.asarray(radius, np.float64))


def tau(ns, dirs, radius, t):
    """The bound on the rounding of t itself, per ray, at the time t."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    return TAU_C * U32 * (np.asarray(t, np.float64) + (np.asarray(radius, np.float64) + extent(ns)) / np.linalg.norm(d, axis=1))


def bracket(ns, origins, dirs, radius):
    """dict(delta, lo = t64(R + delta), hi = t64(R - delta)): +inf where there is no contact."""
    dl = delta(ns, origins, radius)
    R = np.asarray(radius, np.float64)
    assert (R - dl > 0).all(), "a radius within its own bound"
    return dict(delta=dl, lo=first_contact(ns, origins, dirs, R + dl), hi=first_contact(ns, origins, dirs, R - dl))
