"""The sign of the signed point queries restated in numpy float64. Nothing here is shared with include/rt_point_side.h, the topology
unit (ray_tracer_amd/csrc/mesh_topology.cpp) or the kernels: it reads the scene arrays with tests/nearest_float64.py's reader, welds
and connects with a union-find of its own, and decides inside and outside by another route than a pseudo-normal.

The truth for the sign is the WINDING NUMBER of the point about the component of the reported triangle: the sum of the triangles'
signed solid angles (Van Oosterom and Strackee) in world space over 4 pi, the component oriented consistently by a walk of this
module's own. Inside iff it rounds to an odd integer. The truth for "must be signed" is this module's classification of the component:
closed (every edge has two triangles), orientable (the walk meets no contradiction), a volume that is not zero.

A point is excluded from the sign comparison only where the float64 answer itself is indecisive:
  - dst_ref < 64 x bound, bound being nearest_float64.nearest()'s (the point is within float32's reach of the surface);
  - |w - round(w)| > 1e-6;
  - |cos| < 0.05 between q - p and the float64 angle-weighted pseudo-normal of the feature the float64 closest point lies on (the
    point sits on the boundary of the feature's normal cone: which side it is on is a coin toss for any fp32 rule).
At most CAP = 2 % of a set's points may be excluded."""
import numpy as np

import nearest_float64 as nf

CAP = 0.02
W_TOL = 1e-6
COS_MIN = 0.05
NEAR = 64.0


class _Component:
    def __init__(self, rows, closed, orientable, volume, sign):
        self.rows = rows                  # rows of NearestScene.W
        self.closed, self.orientable, self.volume = closed, orientable, volume
        self.sign = sign                  # per row: +1, or -1 where the stored winding is turned over by the walk / the volume
        self.signable = bool(closed and orientable and volume != 0.0 and np.isfinite(volume))


class SideScene:
    """The components of every object of a scene (a NearestScene `ns` and the arrays it was read from)."""

    def __init__(self, arrays, ns):
        self.ns = ns
        tp = arrays["triPoints"].view(np.float32).reshape(-1, 8)[:, 0:3]
        tr = arrays["triangles"].view(np.uint32).reshape(-1, 12)[:, 0:3].astype(np.int64)
        self.component_of = np.full(len(ns.W), -1, np.int64)      # per row of ns.W; -1: a degenerate triangle
        self.components = []
        self.weld = np.zeros((len(ns.W), 3), np.int64)            # welded corner ids, unique per object
        self.neighbours = {}                                      # (row, edge k) -> [(row, edge)] of the other users of the edge
        self.row_of = {(int(o), int(t)): r for r, (o, t) in enumerate(zip(ns.obj, ns.tri))}
        base = 0
        for obj in np.unique(ns.obj):
            rows = np.flatnonzero(ns.obj == obj)
            local = tp[tr[ns.tri[rows]]] + np.float32(0.0)        # [T, 3, 3] object space, -0 -> +0
            uniq, inv = np.unique(local.reshape(-1, 3), axis=0, return_inverse=True)
            ids = inv.reshape(-1, 3) + base
            base += len(uniq)
            self.weld[rows] = ids
            self._connect(rows, ids, local.astype(np.float64))

    def _connect(self, rows, ids, local):
        W = self.ns.W[rows]
        n_obj = np.cross(local[:, 1] - local[:, 0], local[:, 2] - local[:, 0])
        degenerate = (ids[:, 0] == ids[:, 1]) | (ids[:, 1] == ids[:, 2]) | (ids[:, 2] == ids[:, 0]) | ~((n_obj ** 2).sum(axis=1) > 0)
        users = {}
        for t in np.flatnonzero(~degenerate):
            for k in range(3):
                a, b = int(ids[t, k]), int(ids[t, (k + 1) % 3])
                users.setdefault((min(a, b), max(a, b)), []).append((int(t), k))
        parent = list(range(len(rows)))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        open_tris = set()
        for use in users.values():
            for t, k in use:
                self.neighbours[(int(rows[t]), k)] = [(int(rows[t2]), k2) for t2, k2 in use if t2 != t]
            if len(use) != 2:
                open_tris.update(t for t, _ in use)
            for t, _ in use[1:]:
                a, b = find(use[0][0]), find(t)
                if a != b:
                    parent[max(a, b)] = min(a, b)
        members = {}
        for t in np.flatnonzero(~degenerate):
            members.setdefault(find(int(t)), []).append(int(t))
        nb = {(t, k): [u for u in use if u[0] != t][0] for use in users.values() if len(use) == 2 for t, k in use}
        for root, mem in members.items():
            closed = not any(t in open_tris for t in mem)
            sign = {root: 1}
            orientable = closed
            if closed:                                             # the walk: neighbours run along a shared edge in opposite directions
                queue = [root]
                while queue and orientable:
                    t = queue.pop()
                    for k in range(3):
                        t2, k2 = nb[(t, k)]
                        want = -sign[t] if ids[t, k] == ids[t2, k2] else sign[t]
                        if t2 not in sign:
                            sign[t2] = want
                            queue.append(t2)
                        elif sign[t2] != want:
                            orientable = False
                            break
            mem = np.array(mem, np.int64)
            s = np.array([sign.get(int(t), 1) for t in mem], np.float64) if orientable else np.ones(len(mem))
            volume = float((s * np.einsum("tk,tk->t", W[mem, 0], np.cross(W[mem, 1], W[mem, 2]))).sum() / 6.0) if orientable else 0.0
            if volume < 0:
                s = -s
            c = _Component(rows[mem], closed, orientable, abs(volume), s)
            self.component_of[rows[mem]] = len(self.components)
            self.components.append(c)

    # ---------------------------------------------------------------- normals
    def unit_normals(self):
        """Per row of ns.W: the world unit normal, turned outward where the component is signable (else the stored winding's)."""
        W = self.ns.W
        n = np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
        for c in self.components:
            if c.signable:
                n[c.rows] *= c.sign[:, None]
        return n

    def vertex_normals(self):
        """welded id -> the angle-weighted sum of the unit normals of the triangles at the vertex (world angles)."""
        W, n = self.ns.W, self.unit_normals()
        out = np.zeros((int(self.weld.max()) + 1 if len(W) else 0, 3))
        live = self.component_of >= 0
        for k in range(3):
            e1, e2 = W[:, (k + 1) % 3] - W[:, k], W[:, (k + 2) % 3] - W[:, k]
            ang = np.arctan2(np.linalg.norm(np.cross(e1, e2), axis=1), np.einsum("tk,tk->t", e1, e2))
            np.add.at(out, self.weld[live, k], (ang[:, None] * n)[live])
        return out

    def pseudo_normal_at(self, rows, p):
        """The float64 pseudo-normal at points p [P, 3] lying on triangles `rows` [P]: the face's, the edge's or the vertex's, by
        the barycentrics of p (within 1e-9 of a corner or an edge counts as on it)."""
        W, n = self.ns.W[rows], self.unit_normals()
        vn = self.vertex_normals()
        a, b, c = W[:, 0], W[:, 1], W[:, 2]
        nn = np.cross(b - a, c - a)
        den = np.maximum(np.einsum("pk,pk->p", nn, nn), 1e-300)
        wb = np.einsum("pk,pk->p", np.cross(p - a, c - a), nn) / den
        wc = np.einsum("pk,pk->p", np.cross(b - a, p - a), nn) / den
        bary = np.stack([1 - wb - wc, wb, wc], axis=1)
        out = n[rows].copy()
        eps = 1e-9
        for i in range(len(rows)):
            zero = bary[i] <= eps
            if zero.sum() >= 2:
                out[i] = vn[self.weld[rows[i], int(np.argmax(bary[i]))]]
            elif zero.sum() == 1:
                k = (int(np.argmax(zero)) + 1) % 3            # the edge opposite the vanishing corner joins corners k and k + 1
                others = self.neighbours.get((int(rows[i]), k), [])
                out[i] = n[rows[i]] + sum((n[r] for r, _ in others[:1]), np.zeros(3))
        return out

    # ---------------------------------------------------------------- the truth
    def winding(self, comp, q):
        """The winding number of points q [P, 3] about component `comp` (oriented by this module's walk)."""
        c = self.components[comp]
        W = self.ns.W[c.rows]
        out = np.zeros(len(q))
        for k in range(0, len(q), 256):
            A, B, C = (W[None, :, j] - q[k:k + 256, None, :] for j in range(3))
            la, lb, lc = (np.linalg.norm(v, axis=-1) for v in (A, B, C))
            num = np.einsum("ptk,ptk->pt", A, np.cross(B, C))
            den = la * lb * lc + np.einsum("ptk,ptk->pt", A, B) * lc + np.einsum("ptk,ptk->pt", A, C) * lb + np.einsum("ptk,ptk->pt", B, C) * la
            out[k:k + 256] = (2.0 * np.arctan2(num, den) * c.sign[None, :]).sum(axis=1) / (4.0 * np.pi)
        return out

    def truth(self, points, rec, ref):
        """For records `rec` (nearest_to_numpy) of `points` and ref = nearest_float64.nearest() of the same points:
        expected [P] int (+1, -1, 0), kept [P] bool (the sign comparison applies), signable [P] bool, w [P]. Points that found a
        sphere or nothing are not kept here (the spheres' rule is exact: sphere_sides)."""
        q = np.asarray(points, np.float32).astype(np.float64)
        P = len(q)
        expected, kept, signable, w = np.zeros(P, np.int64), np.zeros(P, bool), np.zeros(P, bool), np.zeros(P)
        tri = (rec["found"] != 0) & (rec["isSphere"] == 0)
        rows = np.array([self.row_of[(int(o), int(t))] if m else -1 for m, o, t in zip(tri, rec["objectIndex"], rec["triIndex"])], np.int64)
        comp = np.where(tri, self.component_of[np.maximum(rows, 0)], -1) if len(self.component_of) else np.full(P, -1, np.int64)
        for c in np.unique(comp[comp >= 0]):
            sel = np.flatnonzero(comp == c)
            if not self.components[c].signable:
                kept[sel] = True                                   # expected 0, whatever the point
                continue
            signable[sel] = True
            w[sel] = self.winding(c, q[sel])
            odd = np.abs(np.rint(w[sel])).astype(np.int64) % 2 == 1
            expected[sel] = np.where(odd, -1, 1)
            kept[sel] = np.abs(w[sel] - np.rint(w[sel])) <= W_TOL
        # the float64 answer's own indecision: too near the surface, or on the edge of the normal cone
        near = ref["dst"] < NEAR * ref["bound"]
        on_tri = ~ref["sphere"]
        cosine = np.ones(P)
        if on_tri.any():
            i = np.flatnonzero(on_tri)
            N = self.pseudo_normal_at(ref["index"][i], ref["point"][i])
            d = q[i] - ref["point"][i]
            cosine[i] = np.abs(np.einsum("pk,pk->p", d, N)) / np.maximum(np.linalg.norm(d, axis=1) * np.linalg.norm(N, axis=1), 1e-300)
        kept &= ~(signable & (near | (cosine < COS_MIN)))
        return dict(expected=expected, kept=kept, signable=signable, w=w, near=near, cosine=cosine, component=comp)


def sphere_sides(arrays, points, rec):
    """The spheres' rule restated in numpy float32, operation for operation (a difference, a dot summed left to right, a correctly
    rounded root, two comparisons): exact, so no point is excluded. Returns (side [P] int8, is_sphere [P] bool)."""
    sp = arrays["spheres"].view(np.float32).reshape(len(arrays["spheres"]), 8)
    q = np.asarray(points, np.float32)
    sph = (rec["found"] != 0) & (rec["isSphere"] != 0)
    side = np.zeros(len(q), np.int8)
    if sph.any():
        s = sp[rec["objectIndex"][sph]]
        d = q[sph] - s[:, 0:3]
        l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        side[sph] = np.where(l > s[:, 3], 1, np.where(l < s[:, 3], -1, 0))
    return side, sph
