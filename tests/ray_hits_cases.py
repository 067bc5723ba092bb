"""The cases of the all-hit ray query tests (tests/test_ray_hits_host.py on the CPU, tests/test_ray_hits.py on the GPU): the
scenes and ray sets of closest_hit_cases with the oracle's records, small hand-made scenes for ties and spheres, and the helpers
that turn an (n * k) RtHit array into rows."""
import numpy as np

from oracle import pyoracle
from ray_tracer_amd import engine

import closest_hit_cases as chf

K_MAX = 8                            # RT_HITS_MAX_K
MISS_DST = np.float32(99999999.0)    # RT_MISS_DST
COMPARED = 13                        # words of an RtHit in front of boxTests and triTests

_cases = {}


def case(name, renderer=None):
    """dict(scene, o, d, oracle: the oracle's closest-hit records (hits_to_numpy), oracle_raw: their words (n, 15), bs, ref), once
    per session; the rays are closest_hit_cases' own."""
    key = (name, renderer is not None and name == "blob70k")
    if key not in _cases:
        s, bs, o, d, _, ref, _ = chf._case(name, renderer if name == "blob70k" else None)
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        hits = pyoracle.trace_rays(s, o, d)
        _cases[key] = dict(scene=s, o=o, d=d, oracle=engine.hits_to_numpy(hits), oracle_raw=words(hits, len(o), 1)[:, 0], bs=bs, ref=ref)
    return _cases[key]


def words(hits, n, k):
    """An RtHit array of n * k records -> its uint32 words, shaped (n, k, 15)."""
    if n * k == 0:
        return np.zeros((n, k, 15), np.uint32)
    return np.frombuffer(hits, np.uint8).view(np.uint32).reshape(n, k, 15).copy()


def rows(hits, n, k):
    """hits_to_numpy with every field shaped (n, k, ...)."""
    if n * k == 0:
        return {f: np.zeros((n, k) + ((3,) if f in ("hitPoint", "normal") else ())) for f in ("dst", "didHit", "isSphere", "objectHitIndex", "triHitIndex", "hitPoint", "normal")}
    return {f: v.reshape((n, k) + v.shape[1:]) for f, v in engine.hits_to_numpy(hits).items()}


def is_miss_record(w):
    """Rows of (.., 15) words that are the miss record: dst == RT_MISS_DST and everything else 0."""
    return (w[..., 0] == MISS_DST.view(np.uint32)) & ~w[..., 1:].any(axis=-1)


def check_shape_of_lists(w, counts, k, what):
    """What holds for every answer whatever the scene: min(k, count) hit records in ascending dst with boxTests = triTests = 0, then
    miss records."""
    n = len(counts)
    held = np.minimum(counts, k)
    slot = np.arange(k)[None, :]
    filled = slot < held[:, None]
    assert np.array_equal(is_miss_record(w), ~filled), f"{what}: miss records and counts disagree"
    assert (w[..., 1][filled] == 1).all() and not w[..., 13:][filled].any(), what
    dst = w[..., 0].view(np.float32)
    if k > 1:
        later = filled[:, 1:]
        assert (dst[:, :-1][later] <= dst[:, 1:][later]).all(), f"{what}: a list is not in ascending order"
    assert n == w.shape[0]


def quad_stack():
    """Truncation and ties: one unit quad (two triangles) as 12 objects in front of a ray along +z: objects 0 and 1 place the mesh at
    one place, the other ten are offset copies, by 2^-20 (near-coincident), then by 0.125 each. Returns (scene, origins, dirs): rays
    through the interior of one triangle, so each object gives exactly one crossing."""
    s = engine.Scene()
    s.add_material(engine.default_material())
    pos = np.array([[[-1, -1, 0], [1, 1, 0], [1, -1, 0]], [[-1, -1, 0], [-1, 1, 0], [1, 1, 0]]], np.float32)
    nrm = np.zeros_like(pos)
    nrm[..., 2] = -1
    z = [2.0, 2.0, 2.0 + 2.0 ** -20, 2.0 + 2.0 ** -19] + [2.0 + 0.125 * i for i in range(1, 9)]
    for zi in z:
        s.add_mesh("quad", pos, nrm, engine.placement(position=(0.0, 0.0, zi)), 0)
    rng = np.random.default_rng(3)
    o = np.zeros((96, 3), np.float32)
    o[:, 0] = rng.uniform(0.1, 0.9, 96)
    o[:, 1] = o[:, 0] - rng.uniform(0.05, 0.9, 96)      # x > y: the first triangle
    o[:, 2] = -1.0
    d = np.zeros_like(o)
    d[:, 2] = 1.0
    return s, o, d


def sphere_scene():
    """Spheres (and one quad far above them that no ray reaches): 0 an ordinary one, 1 of radius 0, 2 overlapping 0. Rays: from outside through the spheres, from inside
    sphere 0, tangent to sphere 0 (exactly: origin (1, y, -4) against centre 0, radius 1, direction +z), through the centre of
    the radius-0 sphere, and past everything."""
    s = engine.Scene()
    s.add_material(engine.default_material())
    s.set_sphere(0, (0.0, 0.0, 0.0), 1.0, 0)
    s.set_sphere(1, (3.0, 0.0, 0.0), 0.0, 0)
    s.set_sphere(2, (0.0, 0.5, 1.0), 0.75, 0)
    pos = np.array([[[-1, 50, -1], [1, 50, 1], [1, 50, -1]], [[-1, 50, -1], [-1, 50, 1], [1, 50, 1]]], np.float32)
    nrm = np.zeros_like(pos)
    nrm[..., 1] = -1
    s.add_mesh("far", pos, nrm, engine.placement(), 0)
    rng = np.random.default_rng(4)
    n = 64
    out_o = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), np.full(n, -4.0)], 1)
    out_d = np.tile((0.0, 0.0, 1.0), (n, 1)) * rng.uniform(0.5, 2.0, (n, 1))
    in_o = rng.uniform(-0.4, 0.4, (n, 3))
    in_d = rng.normal(size=(n, 3))
    tan_o = np.array([(1.0, 0.0, -4.0), (0.0, -1.0, -4.0), (-1.0, 0.0, -4.0)])
    tan_d = np.tile((0.0, 0.0, 1.0), (3, 1))
    zero_o = np.array([(3.0, 0.0, -2.0), (3.0, -2.0, 0.0), (3.0, 1e-3, -2.0)])
    zero_d = np.array([(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
    past_o, past_d = np.array([(5.0, 5.0, -4.0)]), np.array([(0.0, 0.0, 1.0)])
    o = np.concatenate([out_o, in_o, tan_o, zero_o, past_o]).astype(np.float32)
    d = np.concatenate([out_d, in_d, tan_d, zero_d, past_d]).astype(np.float32)
    kinds = np.array(["outside"] * n + ["inside"] * n + ["tangent"] * 3 + ["zero"] * 3 + ["past"])
    return s, o, d, kinds


def plane_rays(edited, n=1500, seed=31):
    """Rays at the textured plane of a texture_cases scene (its last object) from random origins in and around the box: two thirds
    aimed at points of the plane, the rest anywhere."""
    import brute_force as bf
    from util import seeded_rays
    bs = bf.BruteScene.from_numpy(edited.scene.numpy())
    o, d = chf._aimed_rays(bs, [len(bs.objects) - 1], n, np.random.default_rng(seed))
    o2, d2 = seeded_rays(n // 2, seed + 1)
    return np.concatenate([o, o2]).astype(np.float32), np.concatenate([d, d2]).astype(np.float32)
