"""Meshes that drive the BVH builders (scene.cpp on the host, bvh_build.hip.h on the GPU, oracle/scene_ref.py as their restatement)
to the places where they can part: partitions that leave one side empty, nodes on which no SAH cost beats the starting 1e30, exact
ties between candidates and axes, and the sizes at which rt_bvh_build changes its launch. Every case comes with the condition that
proves it reaches its edge, asserted from the tree (and, for meshes small enough to restate in Python, from scene_ref's trace), so a
case cannot quietly stop showing what it is there for.

Generators return (positions[n, 3, 3], normals[n, 3, 3]) in float32 and are seeded. Shared by tests/test_bvh_edges_host.py and
tests/test_bvh_device.py."""
import numpy as np

from ray_tracer_amd import scenes

import instantiation_scenes

F = np.float32
RESTATE_MAX = 2000          # triangles up to which oracle/scene_ref.py is run (pure Python, ~0.1 s per 200 triangles)
WIDE_MIN = 8192             # rt_bvh_build: meshes of at least this many triangles take the wide path while a level has <= 32 nodes


def _up(pos):
    nrm = np.zeros_like(pos)
    nrm[..., 1] = 1
    return pos, nrm


def one_ulp(n, seed=1, x=1.0):
    """n triangles flat in x, at x or the next float above it by a seeded bit pattern (both occur), all with the same y and z."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, n)
    b[0], b[1] = 0, 1
    xs = np.where(b == 1, np.nextafter(F(x), F(np.inf)), F(x)).astype(F)
    pos = np.zeros((n, 3, 3), F)
    pos[:, :, 0] = xs[:, None]
    pos[:, 1, 1] = 1
    pos[:, 2, 2] = 1
    return _up(pos)


def two_slabs(a, b, seed=1):
    """one_ulp slabs of a triangles at x = 1 and b triangles at x = 3."""
    return _up(np.concatenate([one_ulp(a, seed, 1.0)[0], one_ulp(b, seed + 1, 3.0)[0]]))


def _huge(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    c = rng.uniform(lo, hi, (n, 1, 3))
    return _up((c + rng.uniform(-1e14, 1e14, (n, 3, 3))).astype(F))


def huge_straddling(n, seed=2):
    """Centroids uniform in +-1e16, corners +-1e14 around them: count * area is above 1e30 for every candidate."""
    return _huge(n, seed, -1e16, 1e16)


def huge_positive(n, seed=3):
    return _huge(n, seed, 1e15, 1e16)


def huge_thin(n, seed=5):
    """Huge in y and z only (every area is above 1e30 through y * z), centroids uniform in +-2 in x with corners +-0.1 around them:
    the starting splitPos of 0 cuts through the mesh, so another starting value gives another tree."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3)) * np.array([2, 1e16, 1e16])
    return _up((c + rng.uniform(-1.0, 1.0, (n, 3, 3)) * np.array([0.1, 1e14, 1e14])).astype(F))


def lattice(k):
    """k^3 copies of one triangle on the integer grid: every bin boundary is hit exactly and the three axes look the same."""
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 1, 3).astype(F)
    return _up((g + np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0.5]], F)).astype(F))


def outlier(n, seed=4):
    """scenes.blob(n) (radius 1) plus three triangles 50 radii away: the first split cuts three triangles off n."""
    pos, nrm = scenes.blob(n, seed=seed)
    far = one_ulp(3, seed)[0] * F(0.1) + np.array([50, 0, 0], F)
    return np.concatenate([pos, far]).astype(F), np.concatenate([nrm, _up(far)[1]]).astype(F)


def skewed():
    return instantiation_scenes.skewed(9000, 8, 6)


def blob(n):
    return scenes.blob(n, seed=n)


# ---------------------------------------------------------------------------------------------------------------- trees
class Tree:
    """One mesh's BVH with indices relative to the mesh: index[v] is the first child (interior, count[v] == 0) or the first
    triangle (leaf); order[p] is the input triangle at position p; trace is scene_ref.build_bvh's, or None."""

    def __init__(self, index, count, order, trace=None):
        self.index, self.count, self.order, self.trace = [int(x) for x in index], [int(x) for x in count], [int(x) for x in order], trace

    @classmethod
    def of_scene(cls, arrays, root=0, tri_first=0, tri_count=None, node_count=None):
        nodes = arrays["bvhNodes"].view(np.uint32).reshape(-1, 8)
        tris = arrays["triangles"].view(np.uint32).reshape(len(arrays["triangles"]), -1)
        tri_count = len(tris) - tri_first if tri_count is None else tri_count
        node_count = len(nodes) - root if node_count is None else node_count
        nd = nodes[root:root + node_count]
        v0 = tris[tri_first:tri_first + tri_count, 0].astype(np.int64)   # add_mesh: unshared points in input order, three per triangle
        index = np.where(nd[:, 7] == 0, nd[:, 6].astype(np.int64) - root, nd[:, 6].astype(np.int64) - tri_first)
        return cls(index, nd[:, 7], (v0 - v0.min()) // 3)

    @classmethod
    def of_ref(cls, nodes, order, trace):
        return cls([nd[6] for nd in nodes], [nd[7] for nd in nodes], order, trace)

    def size(self, v):
        return self.count[v] or self.size(self.index[v]) + self.size(self.index[v] + 1)

    def levels(self):
        out, cur = [], [0]
        while cur:
            out.append(cur)
            cur = [c for v in cur if self.count[v] == 0 for c in (self.index[v], self.index[v] + 1)]
        return out

    def rec(self, node):
        return next(r for r in self.trace if r["node"] == node)


def _rotated(n):
    return list(range(1, n)) + [0]


# ---------------------------------------------------------------------------------------------------------------- conditions
def cond_one_ulp(t, pos):
    n = len(pos)
    assert t.count == [n] and t.order != list(range(n)) and t.order == _rotated(n)       # one leaf, permuted by the give-up
    if t.trace is not None:
        r, = t.trace
        assert r["node"] == 0 and r["nL"] == 0 and not r["split"] and not r["bestDefault"] and r["ties"] == 19 and r["axis"] == 0
        assert r["splitPos"] == F(1.0)                                                    # mn + scale * 1 rounded back to mn


def cond_two_slabs(a, b):
    def cond(t, pos):
        assert t.count == [0, a, b] and t.index[0] == 1                                    # 3 nodes: leaves of a and b > 2 triangles
        if t.trace is not None:
            assert [r["node"] for r in t.trace] == [0, 1, 2]
            assert t.trace[0]["split"] and all(r["nL"] == 0 and not r["split"] and not r["bestDefault"] for r in t.trace[1:])
    return cond


def cond_huge_straddling(t, pos):
    n = len(pos)
    neg = int((((pos[:, 0, 0] + pos[:, 1, 0]) + pos[:, 2, 0]) / F(3) < 0).sum())             # float32 throughout, as the builders' centroids
    assert 0 < neg < n and t.count[:3] == [0, neg, n - neg], (neg, t.count[:3])
    # either side again finds no cost below 1e30 and is partitioned at x = 0 once more: all left / all right, both give up
    assert len(t.count) == 3
    if t.trace is not None:
        r = t.rec(0)
        assert r["bestDefault"] and r["ties"] == 0 and r["axis"] == 0 and r["splitPos"] == 0 and r["nL"] == neg and r["split"]
        assert t.rec(1)["bestDefault"] and t.rec(1)["nL"] == neg and t.rec(2)["bestDefault"] and t.rec(2)["nL"] == 0


def cond_huge_thin(t, pos):
    cond_huge_straddling(t, pos)
    cx = ((pos[:, 0, 0] + pos[:, 1, 0]) + pos[:, 2, 0]) / F(3)
    assert ((cx >= 0) & (cx < 1)).sum() > 0 and ((cx >= -1) & (cx < 0)).sum() > 0            # a start of +-1 would cut elsewhere


def cond_huge_positive(t, pos):
    n = len(pos)
    assert t.count == [n] and t.order == _rotated(n)
    if t.trace is not None:
        r, = t.trace
        assert r["bestDefault"] and r["axis"] == 0 and r["splitPos"] == 0 and r["nL"] == 0 and not r["split"]


def cond_lattice(k):
    def cond(t, pos):
        assert len(pos) == k ** 3 and t.count[0] == 0
        if t.trace is not None:
            tied = [r for r in t.trace if r["ties"] >= 2]
            assert len(tied) >= k and any(len(r["tieAxes"]) >= 2 for r in tied), (len(tied), [r["tieAxes"] for r in tied][:8])
        elif len(pos) > RESTATE_MAX:
            assert len(pos) >= WIDE_MIN                                                  # the same construction through the wide path
    return cond


def cond_outlier(t, pos):
    n = len(pos) - 3
    assert t.count[0] == 0 and sorted((t.size(1), t.size(2))) == [3, n]


def cond_skewed(t, pos):
    n = len(pos)
    hit = [lv for lv in t.levels() if len(lv) > 32 and n // len(lv) < 128 and max(t.size(v) for v in lv) >= 1024]
    assert hit, [(len(lv), max(t.size(v) for v in lv)) for lv in t.levels()]


def cond_none(t, pos):
    pass


SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4223, 4224, 8191, 8192, 8193)

# id -> (mesh, condition)
CASES = {}
for _n in (4, 7, 300, 1024, 1025, 1500):
    CASES[f"one_ulp({_n})"] = (lambda n=_n: one_ulp(n), cond_one_ulp)
for _a, _b in ((6, 7), (700, 900), (4200, 4200)):
    CASES[f"two_slabs({_a},{_b})"] = (lambda a=_a, b=_b: two_slabs(a, b), cond_two_slabs(_a, _b))
for _n in (40, 9000):
    CASES[f"huge_straddling({_n})"] = (lambda n=_n: huge_straddling(n), cond_huge_straddling)
    CASES[f"huge_positive({_n})"] = (lambda n=_n: huge_positive(n), cond_huge_positive)
    CASES[f"huge_thin({_n})"] = (lambda n=_n: huge_thin(n), cond_huge_thin)
for _k in (6, 21):
    CASES[f"lattice({_k})"] = (lambda k=_k: lattice(k), cond_lattice(_k))
for _n in (300, 9000):
    CASES[f"outlier({_n})"] = (lambda n=_n: outlier(n), cond_outlier)
CASES["skewed"] = (skewed, cond_skewed)
for _n in SIZES:
    CASES[f"blob({_n})"] = (lambda n=_n: blob(n), cond_none)
