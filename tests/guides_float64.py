"""TEST INFRASTRUCTURE — the contract of the mirror-following guide planes (rt_render_guides) restated in numpy, float64.

Written from DESIGN.md, "Mirror-following guide planes" (the contract paragraph), not from k_guide_follow, from
tests/guides_cases.py's `follow` or from the oracle, and sharing no code with them: numpy only. It is a user of
tests/paths_float64.py's Estimator (its camera, its `_query`, its Run), as tests/test_radiance_float64.py's RayEstimator is, and every
closest hit is tests/brute_force.py's (offset_rays=True; maps=True where textures are bound): no BVH, no oracle.

THE CHAIN  Segment 0 is the pixel's camera ray. A segment that hits a mirror while j < max_bounces continues: the next direction is
d - 2 (n.d) n, the next origin p + 1e-5 n, with (p, n) the hit's point and normal. A mirror is a material whose reflectance != 0, or,
with maps, brute_force's `mirror` (the metalness texel's red byte != 0 on a triangle hit whose material binds a map). The chain
ends at the first segment that does not continue. L is the number of segments before it, `cut` says that the final hit is itself a
mirror (j reached max_bounces). The record is the final segment's; `depth` is the sum of the segments' dst, ((d0 + d1) + d2) + ...,
on a final hit and RT_MISS_DST on a final miss; `ray_dir` is the final segment's direction; `albedo` the final surface's (the
material's, times the albedo texel with maps), 0 on a miss. `first` is segment 0's record, what rt_render_aovs writes.

TWO MODES, as paths_float64 has them: `exact`, float64 throughout (closest_hit reads its rays as float32 holds them), and `rounded`,
the chain's arithmetic in np.float32 and every hit moved to the edge of brute_force's dst_bound, point_bound and normal_bound under
a seeded sign (Estimator._query: the hit point within the tangent plane, an exact +-1 normal left alone).

SIGNATURE of a pixel: per segment whether it ran, didHit, isSphere, the object, the triangle's nine corners, frontFace, mirror; plus
L and cut. A pixel is FRAGILE if one of its queries is ill-conditioned by brute_force's rules or if its signature differs between
the exact run and any of the four rounded runs (sign seeds 1-4). Fragile pixels are left out of every comparison.
"""
import numpy as np

import paths_float64 as pf

MISS_DST = float(np.float32(99999999.0))     # RT_MISS_DST as float32 holds it
FLOOR = pf.FLOOR                             # |got - ref| <= T * max(|ref|, FLOOR), per component
TOLERANCED = ("depth", "position", "normal", "ray_dir", "albedo")
EXACT = ("sphere", "front_face", "object", "material")


def _record(n):
    return dict(hit=np.zeros(n, bool), sphere=np.zeros(n, bool), front_face=np.zeros(n, bool), object=np.zeros(n, np.int64),
                material=np.zeros(n, np.int64), corners=np.zeros((n, 9)), depth=np.zeros(n), position=np.zeros((n, 3)),
                normal=np.zeros((n, 3)), ray_dir=np.zeros((n, 3)), albedo=np.zeros((n, 3)))


class Chains:
    """What one run leaves: the final record, segment 0's record, L, cut, and per pixel the signature and the ill flag."""

    def __init__(self, n, segments):
        self.final, self.first = _record(n), _record(n)
        self.bounces, self.cut, self.ill = np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n, bool)
        self.codes, self.corners = np.zeros((n, segments), np.int64), np.zeros((n, segments, 9))

    def differs(self, other):
        return ((self.codes != other.codes).any(axis=1) | (self.corners != other.corners).any(axis=(1, 2)) |
                (self.bounces != other.bounces) | (self.cut != other.cut))


class GuideEstimator(pf.Estimator):
    """The chains of a W x H frame's camera rays (`rows`: of these image rows only, in this order), or of the caller's `rays`
    (origins, dirs)."""

    def __init__(self, brute, pc, W, H, max_bounces, maps=False, rows=None, rays=None):
        super().__init__(brute, pc, W, H, maps)
        self.max_bounces = int(max_bounces)
        self.rows = None if rows is None else np.asarray(rows, np.int64)
        self.rays = rays

    def camera(self, F):
        if self.rays is not None:
            return np.asarray(self.rays[0], np.float32).astype(F).reshape(-1, 3), np.asarray(self.rays[1], np.float32).astype(F).reshape(-1, 3)
        o, d = super().camera(F)
        if self.rows is not None:
            keep = (self.rows[:, None] * self.W + np.arange(self.W)[None, :]).reshape(-1)
            o, d = o[keep], d[keep]
        return o, d

    def follow(self, rounded=None):
        """One run: `rounded` is None (exact) or the sign seed."""
        F = np.float64 if rounded is None else np.float32
        o, d = self.camera(F)
        o, d = o.copy(), d.copy()
        n, mb = len(o), self.max_bounces
        R = pf.Run(n, F, rounded)
        C = Chains(n, mb + 1)
        tbl = self.bs.material_table
        mirror_of, albedo_of = tbl["reflectance"] != 0, tbl["albedo"].astype(F)
        length = np.zeros(n, F)
        alive = np.arange(n)
        with np.errstate(all="ignore"):
            for j in range(mb + 1):
                if not len(alive):
                    break
                h = self._query(o[alive], d[alive], R)
                hit = h["didHit"]
                mat = np.where(hit, h["mat"], 0)
                mirror = hit & (h["mirror"] if self.maps else mirror_of[mat])
                C.ill[alive] |= h["ill"]
                C.codes[alive, j] = (1 | hit << 1 | (hit & h["isSphere"]) << 2 | (hit & h["front"]) << 3 | mirror.astype(np.int64) << 4 |
                                     np.where(hit, h["object"], 0) << 12)
                C.corners[alive, j] = np.where((hit & ~h["isSphere"])[:, None], h["corners"], 0)
                albedo = np.where(hit[:, None], h["albedo"] if self.maps else albedo_of[mat], F(0))
                go = mirror & (j < mb)
                for rec, sel, depth in ([(C.first, np.ones(len(alive), bool), h["dst"])] if j == 0 else []) + [(C.final, ~go, length[alive] + h["dst"])]:
                    i, s = alive[sel], sel
                    rec["hit"][i], rec["sphere"][i], rec["front_face"][i] = hit[s], (hit & h["isSphere"])[s], (hit & h["front"])[s]
                    rec["object"][i], rec["material"][i] = np.where(hit, h["object"], 0)[s], mat[s]
                    rec["corners"][i] = np.where((hit & ~h["isSphere"])[:, None], h["corners"], 0)[s]
                    rec["depth"][i] = np.where(hit, depth, MISS_DST)[s]
                    rec["position"][i] = np.where(hit[:, None], h["p"], 0)[s]
                    rec["normal"][i] = np.where(hit[:, None], h["n"], 0)[s]
                    rec["ray_dir"][i], rec["albedo"][i] = d[alive][s], albedo[s]
                C.bounces[alive[~go]], C.cut[alive[~go]] = j, mirror[~go]
                c, nrm, p, rd = alive[go], h["n"][go], h["p"][go], d[alive[go]]
                length[c] = length[c] + h["dst"][go]
                d[c] = rd - (F(2) * pf._dot(nrm, rd))[:, None] * nrm
                o[c] = p + F(0.00001) * nrm
                assert d.dtype == F and o.dtype == F and length.dtype == F
                alive = c
        return C


def distance(got, ref, mask):
    """Largest |got - ref| / max(|ref|, FLOOR) over the components of the rows `mask` (inf if one is not a number). |ref| is the
    magnitude of the quantity: of a vector plane its Euclidean length, which every component of the difference is held to. (Against
    its own component a position on the image's centre column, whose x is exactly 0, would be held to the floor: there the rounded
    run's displacement of 1e-4 within the tangent plane alone is 0.1 of it, and the tolerance would say nothing elsewhere.)"""
    g, r = np.asarray(got, np.float64)[mask], np.asarray(ref, np.float64)[mask]
    if not g.size:
        return 0.0
    with np.errstate(all="ignore"):
        size = np.abs(r) if r.ndim == 1 else np.sqrt((r * r).sum(axis=1, keepdims=True))
        e = np.abs(g - r) / np.maximum(size, FLOOR)
    return float(np.where(np.isnan(e), np.inf, e).max())


class Study:
    """The exact run, the four rounded runs, the fragile pixels and per plane the rounded-to-exact distance over the compared
    pixels (of the final record and of segment 0's)."""

    def __init__(self, est, seeds=pf.SIGN_SEEDS):
        self.exact = est.follow(None)
        self.rounded = [est.follow(s) for s in seeds]
        fragile = self.exact.ill.copy()
        for r in self.rounded:
            fragile |= self.exact.differs(r)
        self.fragile, self.compared = fragile, ~fragile
        self.bounces, self.cut = self.exact.bounces, self.exact.cut
        self.rounded_distance = {k: max(max(distance(r.final[k], self.exact.final[k], self.compared),
                                            distance(r.first[k], self.exact.first[k], self.compared)) for r in self.rounded) for k in TOLERANCED}

    @property
    def excluded(self):
        return float(self.fragile.mean())

    def count(self, mask):
        return int((mask & self.compared).sum())

    def per_L(self):
        return {int(L): self.count(self.bounces == L) for L in np.unique(self.bounces)}


def flat(planes):
    """A dict of render_guides' (rows, W[, 3]) arrays as (n[, 3]) arrays."""
    return {k: np.asarray(v).reshape((-1,) + np.asarray(v).shape[2:]) for k, v in planes.items()}


def disagreements(got, ref, compared, corners_of, chain=None):
    """`got` (flat()'s dict) against a record `ref` of a Chains on the pixels `compared`: the names of the exact fields that
    differ somewhere, and per toleranced plane the distance. `chain`: the Chains whose L and cut go with the record, or None."""
    hit = ref["hit"] & compared
    bad = []
    if not np.array_equal(got["hit"][compared], ref["hit"][compared]):
        bad.append("hit")
    both = hit & got["hit"]
    for k in EXACT:
        if not np.array_equal(np.asarray(got[k])[both].astype(np.int64), ref[k][both].astype(np.int64)):
            bad.append(k)
    tri = both & ~ref["sphere"] & ~np.asarray(got["sphere"], bool)
    corners = np.asarray(corners_of(got["object"][tri], got["triangle"][tri]), np.float64).reshape(-1, 9)
    if not np.array_equal(corners, ref["corners"][tri]):
        bad.append("triangle")
    miss = compared & ~ref["hit"]
    if not np.all(np.asarray(got["depth"], np.float64)[miss] == MISS_DST):
        bad.append("a miss's depth")
    if chain is not None:
        bad += [k for k, v in (("bounces", chain.bounces), ("cut", chain.cut)) if not np.array_equal(np.asarray(got[k])[compared].astype(np.int64), v[compared].astype(np.int64))]
    return bad, {k: distance(got[k], ref[k], compared) for k in TOLERANCED}
