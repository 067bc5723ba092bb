"""The scenes and ray sets of the sphere-sweep tests (tests/test_sweep_host.py on the CPU, tests/test_sweep.py on the GPU), made once
per session from the float64 scene alone, each with its float64 bracket (tests/sweep_float64.py) where a test asks for it.

Scenes: the six of tests/point_query_cases.py (imported, not edited): the Cornell box with its spheres; spheres only; Cornell + the
bunny; four bunny instances with non-uniform scale and shear; 150 placed small objects; and the comb of depth 29, which is what
reaches k_sweep_spheres<64, false>.
Ray sets, 1024 rays a scene: `aimed`, origins uniform in twice the scene's box (no side of it below half the extent), aimed at random surface points; `contact`, origins
on surfaces and at mesh vertices (sphere poles where there is no mesh), so that the sweep starts in contact; `grazing`, rays whose
line passes an edge (a sphere's silhouette where there is no mesh) at 0 to 3 radii; `far`, origins ~1e3 away, aimed at the scene.
Directions are not unit: their lengths run from 0.5 to 2. Radii run log-uniformly from 1/200 to 1/5 of the scene's extent; the far
set's from 1/20 to 1/5, so that its radii stay well above their own bound delta ~ 6e-3 (sweep_float64.delta at |o| ~ 1e3) and the
float64 reference alone keeps the bracket narrow and decided."""
import numpy as np

import brute_force as bf
import nearest_float64 as nf
import point_query_cases as pq
import sweep_float64 as sf

SCENES = pq.SCENES
SETS = (("aimed", 512), ("contact", 128), ("grazing", 256), ("far", 128))

_cases, _brackets = {}, {}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def surface_points(ns, rng, n):
    """n points on the surfaces: triangles by barycentric samples, spheres by directions; both where the scene has both."""
    out = np.zeros((n, 3))
    mesh = np.ones(n, bool) if not len(ns.sph_c) else (rng.random(n) < 0.75 if len(ns.W) else np.zeros(n, bool))
    m = int(mesh.sum())
    if m:
        out[mesh] = np.einsum("pk,pkd->pd", rng.dirichlet((1, 1, 1), m), ns.W[rng.integers(0, len(ns.W), m)])
    if n - m:
        k = rng.integers(0, len(ns.sph_c), n - m)
        out[~mesh] = ns.sph_c[k] + ns.sph_r[k, None] * _unit(rng, n - m)
    return out


def ray_sets(ns, seed):
    """name -> dict(o, d [n, 3] float32, R [n] float32)."""
    rng = np.random.default_rng(seed)
    lo, hi = ns.box()
    mid, half, ext = (lo + hi) / 2, (hi - lo) / 2, float((hi - lo).max())
    n = dict(SETS)
    radii = lambda k, least: ext * np.exp(rng.uniform(np.log(least), np.log(1 / 5), k))
    lengths = lambda k: rng.uniform(0.5, 2.0, (k, 1))
    out = {}

    # (twice the box, no side of it taken below half the extent: under a flat scene most origins would start in contact)
    o = mid + rng.uniform(-2, 2, (n["aimed"], 3)) * np.maximum(half, ext / 4)
    d = surface_points(ns, rng, n["aimed"]) - o
    out["aimed"] = (o, d / np.linalg.norm(d, axis=1, keepdims=True) * lengths(n["aimed"]), radii(n["aimed"], 1 / 200))

    k = n["contact"]
    o = surface_points(ns, rng, k)
    if len(ns.W):
        o[k // 2:] = ns.W[rng.integers(0, len(ns.W), k - k // 2), rng.integers(0, 3, k - k // 2)]
    else:
        j = rng.integers(0, len(ns.sph_c), k - k // 2)
        o[k // 2:] = ns.sph_c[j] + ns.sph_r[j, None] * np.eye(3)[rng.integers(0, 3, k - k // 2)] * rng.choice([-1.0, 1.0], (k - k // 2, 1))
    out["contact"] = (o, _unit(rng, k) * lengths(k), radii(k, 1 / 200))

    k = n["grazing"]
    R = radii(k, 1 / 200)
    dn = _unit(rng, k)
    if len(ns.W):
        t, e = rng.integers(0, len(ns.W), k), rng.integers(0, 3, k)
        a, b = ns.W[t, e], ns.W[t, (e + 1) % 3]
        p = a + rng.uniform(0.1, 0.9, (k, 1)) * (b - a)
        side = np.cross(b - a, dn)                               # the common perpendicular of the edge and the ray
    else:
        j = rng.integers(0, len(ns.sph_c), k)
        side = np.cross(_unit(rng, k), dn)
        p = ns.sph_c[j] + ns.sph_r[j, None] * side / np.linalg.norm(side, axis=1, keepdims=True)
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    o = p + side * (R * rng.uniform(0, 3, k))[:, None] - dn * rng.uniform(1, 2, (k, 1)) * ext
    out["grazing"] = (o, dn * lengths(k), R)

    k = n["far"]
    o = mid + _unit(rng, k) * rng.uniform(800, 1200, (k, 1))
    d = surface_points(ns, rng, k) - o
    out["far"] = (o, d / np.linalg.norm(d, axis=1, keepdims=True) * lengths(k), radii(k, 1 / 20))
    return {key: dict(o=o.astype(np.float32), d=d.astype(np.float32), R=R.astype(np.float32)) for key, (o, d, R) in out.items()}


def case(name):
    """dict(scene, ns (NearestScene), sets: name -> dict(o, d, R))."""
    if name not in _cases:
        scene = pq.build_scene(name)
        ns = nf.NearestScene.from_numpy(pq.arrays_to_numpy(scene.arrays()))
        _cases[name] = dict(scene=scene, ns=ns, sets=ray_sets(ns, 9000 + SCENES.index(name)))
    return _cases[name]


def bracket(name, key):
    """sweep_float64.bracket of one set, made once."""
    if (name, key) not in _brackets:
        c = case(name)
        s = c["sets"][key]
        _brackets[(name, key)] = sf.bracket(c["ns"], s["o"], s["d"], s["R"])
    return _brackets[(name, key)]


def ray_query_bound(ns, s, hit):
    """What rt_query_closest's own dst may differ from the float64 distance by, per ray of the set `s`, for the hits `hit`
    (hits_to_numpy), and which hits are on surfaces at all: (bound [n], surface [n]).
      - a sphere: brute_force.sphere_dst_bound, the operation count of the shader's quadratic about the origin (+inf where its
        first-order count gives none: from ~1e3 away the cancellation in |oc|^2 - r^2 leaves the root of the discriminant
        without a bound);
      - a triangle: a position error of 64 u S (nearest_float64's count for a point against a placed triangle; S is
        sweep_float64's scale of the ray) is a distance error of that over |d| cos(incidence);
      - a zeroed slot of the sphere table (centre 0, radius 0) is no surface, but from ~1e3 away the same cancellation lets the
        shader's arithmetic report it: such a hit names nothing the sweep's surface set holds."""
    o, d = s["o"].astype(np.float64), s["d"].astype(np.float64)
    n = len(o)
    bound, surface = np.zeros(n), np.ones(n, bool)
    S = sf.delta(ns, s["o"], s["R"]) / (sf.DELTA_C * sf.U32)
    did = hit["didHit"] == 1
    sph = did & (hit["isSphere"] == 1)
    tri = did & ~sph
    if sph.any():
        slot = {int(i): r for r, i in enumerate(ns.sph_index)}
        surface[sph] = [int(i) in slot for i in hit["objectHitIndex"][sph]]
        sph &= surface
        r = np.array([slot[int(i)] for i in hit["objectHitIndex"][sph]], np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            bound[sph] = bf.sphere_dst_bound(o[sph], d[sph], ns.sph_c[r], ns.sph_r[r], hit["frontFace"][sph] == 1)
    if tri.any():
        key = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(ns.obj, ns.tri))}
        W = ns.W[np.array([key[(int(a), int(b))] for a, b in zip(hit["objectHitIndex"][tri], hit["triHitIndex"][tri])], np.int64)]
        nrm = np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])
        cos_dl = np.abs(np.einsum("nk,nk->n", nrm, d[tri])) / np.linalg.norm(nrm, axis=1)       # |d| cos(incidence)
        with np.errstate(divide="ignore"):
            bound[tri] = 64 * sf.U32 * S[tri] / cos_dl
    return bound, surface
