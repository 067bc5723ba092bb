"""TEST INFRASTRUCTURE — the closest-hit query in float64, by brute force; with the texture maps on request (TEXTURE MAPS below).

Every triangle of every object and every sphere is tested against every ray in float64 and the nearest accepted hit is kept:
no BVH, no stack, no box test, no float32, no code shared with oracle/ or the kernels (numpy only; `bvhNodes` is read for
`index` / `triCount` alone, to find which triangles belong to an object, never for its bounds). The semantics are those of
raytrace.comp:195-261,276-353 as DESIGN.md states them:

  spheres    near root, the far root if the near one is negative; frontFace follows that choice; the normal points at the origin's
             side. A sphere of radius 0 is hit only by a ray through its centre.
  triangles  the ray goes to object space through the float64 inverse of the object's (float32) matrix, the direction is not
             renormalised (t stays the world parameter); hit if t >= 0, u >= 0, v >= 0, w >= 0; frontFace = (-d.n >= 1e-8) with
             the unnormalised n = e1 x e2; a back-face hit on a frontOnly triangle is rejected.
  normal     normalize(M (w n0 + u n1 + v n2) * +-1) with the FORWARD matrix (raytrace.comp:318: the reference's quirk, matched).
  hit point  o + t d.
  nearest    spheres before objects, objects in index order, a later primitive must be strictly nearer.

Besides the hit, every ray gets a conditioning verdict (`ill`): a float32 implementation cannot be held to the float64 answer
where the answer hangs on a rounding. With the margin eps a ray is ill-conditioned if
  (a) some triangle with min(u, v, w) > -eps and t > -eps has |min(u, v, w)| < eps or |t| < eps, or is frontOnly and has
      |-d.n - 1e-8| / (|d||n|) < eps; the same facing test on the winning triangle, frontOnly or not (its frontFace and the
      sign of its normal hang on it);
  (b) some sphere has |disc| / (a r^2) < eps (r = 0: / (a |oc|^2)), or a root with |t| < eps;
  (c) the second-nearest accepted t is within eps (relative) of the nearest;
  (d) the hit has no finite error bound (below): the first-order count breaks down there, nothing can be asked of the ray.
For the rays of a path, which start 1e-5 off the surface they leave, closest_hit(offset_rays=True) reads "|t| < eps" in (a) and (b)
as "|t| is within a few of the candidate's own dst bounds of 0" (its docstring); the verdicts without it are unchanged.

ERROR BOUNDS (closest_hit returns them per ray; u = 2^-24 is the unit roundoff of float32, round to nearest)

dst, triangles.  |dt| <= c u [ (|o'-v0| / |d'| + t) / (cos(theta) sin(gamma)) + T ] g, with theta the angle between the ray and the
geometric normal, gamma the triangle's angle at v0 (|e1 x e2| = |e1||e2| sin(gamma): the cancellation of the cross product) and
T the object-space transform's share. The count, first order, every float32 operation one relative error <= u, A = |e1||e2|:
  e1, e2, r = o'-v0     1 rounding per component
  n = e1 x e2           per component fl(fl(ab) - fl(cd)): inputs 2u, product u, difference u = 4u (|ab| + |cd|); the vector of
                        those sums has norm <= sqrt(2) A  (sum_x (1-a_x^2)(1-b_x^2) <= 2 for unit a, b):       |dn| <= 5.66 u A
  num = r.n             r: u |r||n|; n: 5.66 u |r| A; three products and two sums: 3 u |r||n|:                 <= 9.66 u |r| A
  d0 = -d'.n            n: 5.66 u |d'| A; the dot: 3 u |d'||n|:                                                <= 8.66 u |d'| A
  t = num * (1 / d0)    2u t
  with |d0| = |d'| A sin(gamma) cos(theta):  |dt| <= u (9.66 |r|/|d'| + 8.66 t) / (sin cos) + 2 u t <= 11 u (|r|/|d'| + t) / (sin cos).
So c = 11 (DST_C). g = 1 / (1 - c u (1/(sin cos) + |dd'|/(|d'| cos))) carries the second order of d0's own relative error
(infinite where that reaches 1: no bound exists there, and the ray is ill-conditioned by rule (d)).
T: o' = fl(Minv32 [o; 1]) and d' = fl(Minv32 [d; 0]), where Minv32 = rt_mat4_inverse(M) in float32 against the exact inverse.
rt_mat4_inverse is cofactors over 2x2 sub-determinants: a sub-determinant has 2u of its absolute expansion, a cofactor (three
products, two sums) 5u of its absolute expansion (the permanent of the minor's absolute values), the determinant 10u of its own
(the permanent of |M|), 1/det and the final product u each. With E1 = perm(|minor|)/|det| + |Minv| (perm(|M|)/|det| + 1) that is
|dMinv| <= 10 u E1 entry by entry; the transform itself (three products, three sums) adds 4u |Minv| |[o; 1]|. Both fit under
c = 11 with unit weights: do' = (E1 + |Minv|) |[o; 1]|, dd' = (E1 + |Minv|)_3x3 |d|, and a displacement of the ray by do' + t dd'
moves t by at most T = (|do'| + t |dd'|) / (|d'| cos(theta))  (2-norms of the componentwise bounds).

dst, spheres.  The same count through b^2 - a c (sphere_dst_bound below, every line annotated).

hitPoint.  dst bound * |d|, plus for triangles c u [ |M3| (|do'| + t |dd'|) + |M3| (|o'| + t |d'|) + | |M| [|p'|; 1] | ] (the displaced
ray, o' + t d' in float32, the forward transform), for spheres 2u (|o| + t |d|).

normal.  Barycentric error, same count: |du|, |dv| <= B = g [ c u ((|r| + t |d'|) / e_min + 1) + (|do'| + |r||dd'|/|d'|) / e_min + |dd'|/|d'| ]
/ (sin cos) with e_min the shorter of e1, e2; |d ni| <= B (|n1-n0| + |n2-n0|) + 8u (|n0|+|n1|+|n2|) (w = 1-u-v and the three
scaled sums); through the forward matrix and the normalisation: (|M3| |d ni| + 3u | |M3| |ni| |) / |M3 ni| + 5u. It scales with
the triangle: thin smooth-shaded triangles get a wide bound, flat ones a few ulp.

TEXTURE MAPS (closest_hit(..., maps=True); set_textures, set_material, Mesh's uvs, the objects' samplerIndex). The semantics are the
project's own declaration (include/rt_amd.h: the reference's shader samples nothing), restated here from that prose:

  uv         hit.uv = w uv0 + u uv1 + v uv2 with u towards corner 1 and v towards corner 2; (0.5, 0.5) when any two corners share
             their uv exactly.
  texel      column floor(u W), row floor((1 - v) H) (v runs upwards, rows downwards); sampler 0 wraps both by a floor modulus,
             sampler 1 clamps them to the edge; the next texel along an axis wraps to 0 or stays on the last one, by sampler.
             A slot below 0 or beyond the texture table binds nothing. Spheres are not textured.
  decode     the sRGB transfer function of a byte, in float64.
  alpha      inside the search: a triangle candidate (accepted by the triangle test) whose alpha texel's red byte is < 188 is no
             hit, and the nearest candidate that is left wins: a later triangle, a later object, a sphere, or nothing.
  albedo     the material's albedo times the decoded rgb of the albedo texel (triangle hits of a material that binds one).
  mirror     the metalness texel's red byte != 0 (the decode is 0 at byte 0 alone); without a map, reflectance != 0.
  bump       heights are decoded red bytes; hx, hy = the steps from the hit's texel to the next texel of its row and of its column;
             n' = normalize(n_interp) - (hx T^ - hy B^) in object space and BEFORE the front-face sign, T = dP/du and B = dP/dv of
             the triangle (e1 = du1 T + dv1 B, e2 = du2 T + dv2 B), T^, B^ their unit vectors; then the sign, the forward matrix
             and normalize as for `normal`. Unchanged where hx = hy = 0 or the uv determinant du1 dv2 - du2 dv1 is 0.

Conditioning, on top of (a)-(d): a ray is ill-conditioned if
  (e) a triangle candidate that takes part in the decision (the winner; with an alpha map every candidate up to the winner, on a
      miss every one) has u W or (1 - v) H of a map in play within max(eps, B * (|uv1 - uv0| + |uv2 - uv0|) * size) of an integer,
      B the barycentric bound below: float32 may land on the texel next door. The fallback's (0.5, 0.5) is the same number on
      both sides and never in doubt.
  (f) the winner binds a bump map and its uv determinant is nonzero but below eps (|du1 dv2| + |du2 dv1|): its sign, and with it
      the tangent frame's, hangs on a rounding. A determinant of exactly 0 is exactly 0 in float32 too (equal corner uvs give
      equal products): well-conditioned.
  (d) covers the bumped normal's bound too.

Bumped normal, the bound (first order, every float32 operation one relative error <= u, absolute errors in object space):
  normalize(n_interp)      |d ni| / |ni| (the bound on the interpolated normal above) + 5u for the normalisation
  hx, hy                   two decodes at 8 ulp = 16u each (tests/test_glsl_builtins.py, + 1e-9) and the difference:
                           |dhx| <= 16u (h0 + h1) + 2e-9 + u |hx|
  T^                       normalisation leaves of T = (e1 dv2 - e2 dv1) / det only the direction of the bracket and det's sign:
                           e1, dv2 and their product 3u, the difference u: 4u (|e1||dv2| + |e2||dv1|) / |e1 dv2 - e2 dv1| = 4u kT;
                           the scaling by 1 / det u, the normalisation 5u: |dT^| <= (4 kT + 6) u; likewise B^ with kB
  hx T^, hy B^             |dhx| + |hx| (4 kT + 6) u + u |hx| each; their difference u (|hx| + |hy|); the final difference u |n'|
  |dn'| <= |d ni| / |ni| + 5u + |dhx| + |dhy| + u |hx| (4 kT + 7) + u |hy| (4 kB + 7) + u (|hx| + |hy|) + u |n'|
and through the forward matrix and the last normalisation, as for `normal` but with the denominator's own error kept:
(|M3| |dn'| + 3u | |M3| |n'| |) / (|M3 n'| - |M3| |dn'|) + 5u, infinite where the denominator is not positive (n' near 0: the
height step cancels the normal; rule (d)).

OBSERVED with maps, on the CPU oracle (tests/test_texture_maps_float64.py prints these; the GPU cases print their own). "map hits" are
well-conditioned rays that end on a triangle with a bound map; the last column is the largest |dn| / bound over the bumped normals.

    ray set              rays   map hits   excluded   largest |dt| / bound(c = 1)   bumped |dn| / bound
    albedo_bump/aimed    3000   2818       0.70 %     1.16                          0.040
    albedo_bump/camera   6144   1708       0.16 %     1.23                          0.011
    alpha/aimed          3000   2257       1.60 %     1.24                          -
    alpha/camera         6144   1294       0.24 %     0.97                          -
    all/aimed            3000   2251       1.80 %     1.24                          0.027
    all/camera           6144   1294       0.24 %     0.97                          0.011

The bumped normal's ratio is far below 1 because the count charges both decodes their full 16u while the heights' errors largely
cancel in the step, and B is a worst case over the triangle; a wrong sign, frame or texel moves the normal by the size of the
step itself, 10^4 bounds and more. The furnace render of the same test file (its tolerance is derived in its docstring, 26u + 1e-9): the
oracle's worst pixel is 6.7u off. Only the oracle's figures are recorded here; the GPU cases print theirs when they run.

OBSERVED on the CPU oracle.  Largest |dt| / bound(c = 1) on well-conditioned triangle hits, per ray set of
tests/test_closest_hit_float64.py (which prints these figures, for the GPU cases too, and asserts c >= twice the oracle's ratio).
"excluded" is the ill-conditioned share at eps = 1e-4, the rays dropped for starting on the surface they hit included.

    ray set      rays   well-conditioned   excluded   largest |dt| / bound(c = 1)
                        mesh hits
    cornell      5596   1287               0.59 %     0.23
    meshes       4400   3352               0.50 %     0.35
    surface      2979    840               0.84 %     0.38
    blob70k      1400   1141               0.43 %     1.42
    instances    2600   1880               0.69 %     1.37
    front_only   2836   1488               0.35 %     1.51
    camera       4800   1434               0.35 %     0.24

The ratio is near 1.5 where the object's matrix is the identity (T = 0) and lower where T, the transform's share, adds to the
bound; c = 11 is 7 times the worst of them.
"""
import itertools

import numpy as np

U32 = 2.0 ** -24      # unit roundoff of float32
DST_C = 11.0          # the rounding count derived above
EPS = 1e-4            # conditioning margin
ALPHA_CUT_BYTE = 188  # srgb8_to_linear(187) = 0.4969, (188) = 0.5029: "decodes below 0.5", as a test on the byte
DECODE_ULP = 8        # tests/test_glsl_builtins.py holds the float32 decode to 8 ulp (+ 1e-9) of srgb8_to_linear


# ---------------------------------------------------------------- camera rays (moved here from tests/test_aovs.py)
def camera_dirs(pc, W, H):
    """raytrace.comp:547-556 in float64: a plane of nearPlane * tan(fov / 2) * 2 by aspectRatio times that, at depth 0.1 (not
    nearPlane), uv = pixel / image size, dir = normalize(point), (cameraRotation * vec4(dir, 1)).xyz.
    The depth is the double 0.1, the shader's literal as written: temporal_float64.primary_dirs takes float32(0.1) instead."""
    cam = pc.camInfo
    ph = np.float64(np.float32(cam.nearPlane)) * np.tan(np.radians(np.float64(np.float32(cam.fov)) * 0.5)) * 2.0
    pw = ph * np.float64(np.float32(cam.aspectRatio))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = x / W, y / H
    p = np.stack([-pw / 2 + pw * u, -ph / 2 + ph * v, np.full_like(u, 0.1)], -1)
    d = p / np.linalg.norm(p, axis=-1, keepdims=True)
    M = np.array(list(cam.cameraRotation), np.float64).reshape(4, 4).T   # column-major
    return d @ M[:3, :3].T + M[:3, 3]


# ---------------------------------------------------------------- placement matrix
def placement_matrix(position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1)):
    """T * Rx * Ry * Rz * S in float64, rotations in degrees (src/vk_engine.cpp:1597-1601)."""
    if np.isscalar(scale):
        scale = (scale,) * 3
    rx, ry, rz = np.radians(np.asarray(rotation, np.float64))
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rx @ Ry @ Rz @ np.diag(np.asarray(scale, np.float64))
    M[:3, 3] = np.asarray(position, np.float64)
    return M


def _perm(a):
    n = a.shape[0]
    return sum(np.prod([a[i, p[i]] for i in range(n)]) for p in itertools.permutations(range(n)))


def inverse_error_unit(M):
    """E1 of the module docstring: |rt_mat4_inverse(M) - inverse(M)| <= 10 u E1, entry by entry."""
    A, det, Minv = np.abs(M), abs(np.linalg.det(M)), np.linalg.inv(M)
    E = np.zeros((4, 4))
    pdet = _perm(A)
    for i in range(4):
        for j in range(4):
            minor = np.delete(np.delete(A, j, 0), i, 1)      # inverse[i, j] = cofactor(j, i) / det
            E[i, j] = _perm(minor) / det + abs(Minv[i, j]) * (pdet / det + 1.0)
    return E


def _transform_error_unit(M, Minv):
    """E1 + |Minv| of the module docstring. An identity matrix costs nothing: its float32 inverse is the identity exactly, and
    products with 0 and 1 and sums with 0 are exact."""
    if np.array_equal(M, np.eye(4)):
        return np.zeros((4, 4))
    return inverse_error_unit(M) + np.abs(Minv)


def srgb8_to_linear(byte):
    """The sRGB transfer function (IEC 61966-2-1) of a byte, in float64."""
    c = np.asarray(byte, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def texel_index(coord, size, clamp):
    """Nearest filter along one axis: floor(coord * size), clamped to the edge (sampler 1) or wrapped by a floor modulus
    (sampler 0). Also returns coord * size, for the conditioning verdict."""
    f = np.asarray(coord, np.float64) * size
    i = np.floor(f).astype(np.int64)
    return (np.clip(i, 0, size - 1) if clamp else np.mod(i, size)), f


def texel_next(i, size, clamp):
    """The next texel along an axis: stays on the last one under the clamp sampler, wraps to 0 under the other."""
    return np.where(i + 1 < size, i + 1, i if clamp else 0)


MAP_SLOTS = ("albedo", "alpha", "metalness", "bump")


def material_records(arrays):
    """Every material's full record from Scene.numpy(), the float32 values widened to float64: albedo [M, 3], emissionColor [M, 3],
    emissionStrength, reflectance and ior [M] (src/vk_engine.h:69-79). What tests/paths_float64.py shades with."""
    mt = arrays.get("materials", ())
    f = (mt.view(np.float32).reshape(len(mt), -1) if len(mt) else np.zeros((0, 16), np.float32)).astype(np.float64)
    return dict(albedo=f[:, 0:3], emissionColor=f[:, 4:7], emissionStrength=f[:, 7], reflectance=f[:, 8], ior=f[:, 9])


class Mesh:
    def __init__(self, positions, normals, front_only, uvs=None):
        self.P = np.asarray(positions, np.float64).reshape(-1, 3, 3)
        self.N = np.asarray(normals, np.float64).reshape(-1, 3, 3)
        # per-corner uv as float32 holds them; none given: all (0, 0), which is the fallback everywhere
        self.UV = (np.zeros((len(self.P), 3, 2)) if uvs is None
                   else np.asarray(uvs, np.float32).astype(np.float64).reshape(-1, 3, 2))
        a, b, c = self.UV[:, 0], self.UV[:, 1], self.UV[:, 2]
        self.fallback = (a == b).all(axis=1) | (b == c).all(axis=1) | (c == a).all(axis=1)
        fo = np.asarray(front_only, bool)
        self.front_only = np.broadcast_to(fo, (len(self.P),)).copy()
        v0 = self.P[:, 0]
        self.e1, self.e2 = self.P[:, 1] - v0, self.P[:, 2] - v0
        self.n = np.cross(self.e1, self.e2)
        self.c0 = np.einsum("ij,ij->i", v0, self.n)
        self.e1xv0, self.e2xv0 = np.cross(self.e1, v0), np.cross(self.e2, v0)
        self.nlen = np.linalg.norm(self.n, axis=1)
        self.e1l, self.e2l = np.linalg.norm(self.e1, axis=1), np.linalg.norm(self.e2, axis=1)

    def uv_at(self, k, u, v):
        """hit.uv = w uv0 + u uv1 + v uv2 of the triangles k, (0.5, 0.5) where two corners share their uv; and per axis the
        corners' uv spread |uv1 - uv0| + |uv2 - uv0| (what a barycentric error is multiplied by)."""
        UV = self.UV[k]
        uv = (1.0 - u - v)[:, None] * UV[:, 0] + u[:, None] * UV[:, 1] + v[:, None] * UV[:, 2]
        uv[self.fallback[k]] = 0.5
        return uv, np.abs(UV[:, 1] - UV[:, 0]) + np.abs(UV[:, 2] - UV[:, 0])


def _bary_bound(e1l, e2l, nlen, rl, t, dlen, d0, do, ddv):
    """B of the module docstring (the bound on |du|, |dv|), with g, sin(gamma) and cos(theta)."""
    cos = np.abs(d0) / (dlen * nlen)
    sin = nlen / (e1l * e2l)
    den = 1.0 - DST_C * U32 * (1.0 / (sin * cos) + ddv / (dlen * cos))
    g = np.where(den > 0, 1.0 / den, np.inf)
    emin = np.minimum(e1l, e2l)
    B = g * (DST_C * U32 * ((rl + t * dlen) / emin + 1.0) + DST_C * U32 * ((do + rl * ddv / dlen) / emin + ddv / dlen)) / (sin * cos)
    return B, g, sin, cos


def _lookup(tex, uv, spread, B, fallback, clamp, eps):
    """Texel column and row of a map at uv, and whether float32 may land on another texel: u W or (1 - v) H within
    max(eps, B * spread * size) of an integer. The fallback's (0.5, 0.5) is exact on both sides: never in doubt."""
    h, w = tex.shape[:2]
    x, fx = texel_index(uv[:, 0], w, clamp)
    y, fy = texel_index(1.0 - uv[:, 1], h, clamp)
    mx, my = np.maximum(eps, B * spread[:, 0] * w), np.maximum(eps, B * spread[:, 1] * h)
    near = ~fallback & ~((np.abs(fx - np.rint(fx)) >= mx) & (np.abs(fy - np.rint(fy)) >= my))
    return x, y, near


class BruteScene:
    """Spheres, meshes and objects (mesh, 4x4 float64 matrix, material) in the order the renderer numbers them."""

    def __init__(self):
        self.sph_c = np.zeros((0, 3)); self.sph_r = np.zeros(0); self.sph_mat = np.zeros(0, np.int64)
        self.meshes, self.objects = [], []          # objects: [mesh index, M, material, samplerIndex]
        self.materials = {}                         # material index -> dict(albedo, reflectance, <slot>Index ...); absent: no maps
        self.textures = []                          # uint8 [h, w, 4], in slot order
        self.material_table = None                  # material_records() of the scene from_numpy read

    def set_textures(self, images):
        self.textures = [np.asarray(im, np.uint8) for im in images]

    def set_material(self, index, albedo=(1.0, 1.0, 1.0), reflectance=0.0, albedoIndex=-1, alphaIndex=-1, metalnessIndex=-1, bumpIndex=-1):
        self.materials[int(index)] = dict(albedo=np.asarray(albedo, np.float32).astype(np.float64), reflectance=float(reflectance),
                                          albedoIndex=int(albedoIndex), alphaIndex=int(alphaIndex),
                                          metalnessIndex=int(metalnessIndex), bumpIndex=int(bumpIndex))

    def bound_map(self, material, slot):
        """The texture a material's slot binds; a slot below 0 or beyond the table binds nothing."""
        m = self.materials.get(int(material))
        i = -1 if m is None else m[slot + "Index"]
        return self.textures[i] if 0 <= i < len(self.textures) else None

    def set_spheres(self, centres, radii, materials):
        self.sph_c = np.asarray(centres, np.float64).reshape(-1, 3)
        self.sph_r = np.asarray(radii, np.float64).reshape(-1)
        self.sph_mat = np.asarray(materials, np.int64).reshape(-1)

    def add_object(self, positions, normals, matrix, front_only=False, material=0, uvs=None, sampler=0):
        self.meshes.append(Mesh(positions, normals, front_only, uvs))
        self.objects.append([len(self.meshes) - 1, np.asarray(matrix, np.float64).reshape(4, 4), int(material), int(sampler)])
        return len(self.objects) - 1

    def replace_mesh(self, obj, positions, normals, front_only, uvs=None):
        """The test's own arrays instead of what from_numpy read for this object (and for every object sharing its mesh)."""
        self.meshes[self.objects[obj][0]] = Mesh(positions, normals, front_only, uvs)

    @classmethod
    def from_numpy(cls, arrays):
        """From Scene.numpy(): triPoints, triangles, objects, spheres, and the leaf ranges (index / triCount) under bvhIndex."""
        s = cls()
        sp = arrays["spheres"]
        if len(sp):
            f, u = sp.view(np.float32).reshape(len(sp), -1), sp.view(np.uint32).reshape(len(sp), -1)
            s.set_spheres(f[:, 0:3], f[:, 3], u[:, 4])
        tp = arrays["triPoints"].view(np.float32).reshape(-1, 8)
        ob = arrays["objects"]
        if not len(ob):                                                       # spheres alone
            s.material_table = material_records(arrays)
            return s
        tr = arrays["triangles"].view(np.uint32).reshape(len(arrays["triangles"]), -1)
        nodes = arrays["bvhNodes"].view(np.uint32).reshape(len(arrays["bvhNodes"]), -1)[:, 6:8]
        of, ou = ob.view(np.float32).reshape(len(ob), -1), ob.view(np.uint32).reshape(len(ob), -1)
        by_root = {}
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
                t = tr[np.array(sorted(tris), np.int64)]
                corners = tp[t[:, 0:3].astype(np.int64)]                  # [T, 3, 8]
                s.meshes.append(Mesh(corners[:, :, 0:3], corners[:, :, 4:7], t[:, 3] != 0, corners[:, :, [3, 7]]))   # uv = (position.w, normal.w)
                by_root[root] = len(s.meshes) - 1
            M = of[i, 0:16].astype(np.float64).reshape(4, 4).T            # column-major m[c * 4 + r]
            s.objects.append([by_root[root], M, int(ou[i, 18]), int(ou[i, 19])])
        mt = arrays.get("materials", ())
        if len(mt):
            mf, mi = mt.view(np.float32).reshape(len(mt), -1), mt.view(np.int32).reshape(len(mt), -1)
            for i in range(len(mt)):
                s.set_material(i, mf[i, 0:3], mf[i, 8], albedoIndex=mi[i, 10], metalnessIndex=mi[i, 11], alphaIndex=mi[i, 12], bumpIndex=mi[i, 13])
        s.material_table = material_records(arrays)
        return s

    # ------------------------------------------------------------------------------------------------------------
    def closest_hit(self, origins, dirs, eps=EPS, max_pairs=3_000_000, maps=False, offset_rays=False):
        """The nearest accepted hit of every ray, its conditioning verdict and its error bounds: a dict of arrays. With `maps`
        the texture maps take part (module docstring, TEXTURE MAPS): the alpha cut inside the search, and uv, texels, albedo,
        mirror and the bumped normal of the hit.

        `offset_rays` (tests/paths_float64.py): the rays are a path's, which leave a surface from 1e-5 (or 0.01) off it along the
        normal, so the surface they left is a candidate with |t| = 1e-5 / cos(theta) and rules (a) and (b) would call every such
        ray ill. The only decision that hangs on a small t is its sign, and float32 gets t wrong by no more than the dst bound of
        that very candidate, which shrinks with 1 / cos(theta) as t does. With offset_rays, "|t| < eps" in (a) and (b) reads
        "|t| < max(1e-6, 4 x the candidate's own dst bound)": the first-order bound of the module docstring without the
        transform's share, times 4 to cover that share and the second order; for a sphere, whose bound is complete to first order
        (sphere_dst_bound), times 2. A ray that leaves a sphere of radius r from 1e-5 off it has |t| = 12 / r bounds: beyond
        r = 6 float32 cannot tell which side of the sphere such a ray starts on. Everything else is as without it."""
        o = np.asarray(origins, np.float32).astype(np.float64).reshape(-1, 3)
        d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
        n = len(o)
        INF = np.inf
        best = np.full(n, INF); second = np.full(n, INF)
        kind = np.full(n, -1)                       # -1 miss, 0 sphere, 1 triangle
        bobj = np.zeros(n, np.int64); btri = np.zeros(n, np.int64)
        ill = np.zeros(n, bool)
        sfront = np.zeros(n, bool)
        near_t = np.full(n, INF)                    # nearest candidate whose alpha texel hangs on a rounding
        cut_t = np.full(n, INF)                     # nearest candidate the alpha map cut out

        def merge(rows, t1, t2, k, obj, tri):
            """t1 <= t2: the two nearest accepted t of one primitive set, for the rays `rows`."""
            b, s2 = best[rows], second[rows]
            win = t1 < b
            second[rows] = np.where(win, np.minimum(b, t2), np.minimum(s2, t1))
            w = rows[win]
            best[w] = t1[win]; kind[w] = k; bobj[w] = obj if np.isscalar(obj) else obj[win]; btri[w] = tri[win]
            return win

        rows_all = np.arange(n)
        with np.errstate(all="ignore"):
            # ---- spheres
            a = np.einsum("ij,ij->i", d, d)
            for i in range(len(self.sph_r)):
                oc = self.sph_c[i] - o
                r = self.sph_r[i]
                b = np.einsum("ij,ij->i", oc, d)
                oc2 = np.einsum("ij,ij->i", oc, oc)
                disc = b * b - a * (oc2 - r * r)
                ill |= np.abs(disc) / (a * (r * r if r > 0 else oc2)) < eps
                sq = np.sqrt(np.maximum(disc, 0.0))
                tn, tf = (b - sq) / a, (b + sq) / a
                ok = disc >= 0
                if offset_rays:
                    cc = np.repeat(self.sph_c[i][None], n, 0)
                    bn, bfar = sphere_dst_bound(o, d, cc, r, np.ones(n, bool)), sphere_dst_bound(o, d, cc, r, np.zeros(n, bool))
                    ill |= ok & ~((np.abs(tn) >= np.maximum(1e-6, 2 * bn)) & (np.abs(tf) >= np.maximum(1e-6, 2 * bfar)))
                else:
                    ill |= ok & ((np.abs(tn) < eps) | (np.abs(tf) < eps))
                front = tn >= 0
                t = np.where(front, tn, tf)
                t = np.where(ok & (t >= 0), t, INF)
                win = merge(rows_all, t, np.full(n, INF), 0, i, np.zeros(n, np.int64))
                sfront[rows_all[win]] = front[win]
            # ---- triangles
            xf = []
            for j, (mi, M, mat, sampler) in enumerate(self.objects):
                mesh = self.meshes[mi]
                alpha = self.bound_map(mat, "alpha") if maps else None
                Minv = np.linalg.inv(M)
                op = o @ Minv[:3, :3].T + Minv[:3, 3]
                dp = d @ Minv[:3, :3].T
                xf.append((Minv, op, dp))
                T = len(mesh.P)
                if T == 0:
                    continue
                dlen = np.linalg.norm(dp, axis=1)
                if alpha is not None:
                    Wj = _transform_error_unit(M, Minv)
                    do_all = np.linalg.norm(np.concatenate([np.abs(o), np.ones((n, 1))], axis=1) @ Wj[:3, :].T, axis=1)
                    ddv_all = np.linalg.norm(np.abs(d) @ Wj[:3, :3].T, axis=1)
                step = max(1, max_pairs // T)
                for r0 in range(0, n, step):
                    rows = rows_all[r0:r0 + step]
                    oo, dd = op[rows], dp[rows]
                    od = np.cross(oo, dd)
                    d0 = -(dd @ mesh.n.T)
                    t = (oo @ mesh.n.T - mesh.c0) / d0
                    uu = (od @ mesh.e2.T - dd @ mesh.e2xv0.T) / d0
                    vv = -(od @ mesh.e1.T - dd @ mesh.e1xv0.T) / d0
                    m = np.minimum(np.minimum(uu, vv), 1.0 - uu - vv)
                    back = ~(d0 >= 1e-8)
                    fo = mesh.front_only[None, :]
                    acc = (t >= 0) & (m >= 0) & ~(fo & back)
                    if alpha is not None:
                        # the alpha cut: a candidate whose alpha texel's red byte is below 188 is no hit; the search goes on
                        ri, ti = np.nonzero(acc)
                        rr = rows[ri]
                        tc, uc, vc = t[ri, ti], uu[ri, ti], vv[ri, ti]
                        rl = np.linalg.norm(oo[ri] - mesh.P[ti, 0], axis=1)
                        Bc = _bary_bound(mesh.e1l[ti], mesh.e2l[ti], mesh.nlen[ti], rl, tc, dlen[rr], d0[ri, ti], do_all[rr], ddv_all[rr])[0]
                        uvc, spread = mesh.uv_at(ti, uc, vc)
                        x, y, near = _lookup(alpha, uvc, spread, Bc, mesh.fallback[ti], sampler == 1, eps)
                        cut = alpha[y, x, 0] < ALPHA_CUT_BYTE
                        np.minimum.at(near_t, rr[near], tc[near])
                        np.minimum.at(cut_t, rr[cut], tc[cut])
                        acc[ri[cut], ti[cut]] = False
                    cand = (m > -eps) & (t > -eps)
                    t_small = np.abs(t) < eps
                    if offset_rays:
                        v0 = mesh.P[:, 0]
                        rl = np.sqrt(np.maximum((oo * oo).sum(axis=1)[:, None] - 2.0 * (oo @ v0.T) + (v0 * v0).sum(axis=1)[None, :], 0.0))
                        sincos = np.abs(d0) / (dlen[rows, None] * (mesh.e1l * mesh.e2l)[None, :])
                        t_small = ~(np.abs(t) >= np.maximum(1e-6, 4 * DST_C * U32 * (rl / dlen[rows, None] + np.abs(t)) / sincos))
                    bad = cand & ((np.abs(m) < eps) | t_small |
                                  (fo & (np.abs(d0 - 1e-8) < eps * dlen[rows, None] * mesh.nlen[None, :])))
                    ill[rows] |= bad.any(axis=1)
                    tt = np.where(acc, t, INF)
                    i1 = np.argmin(tt, axis=1)
                    k = np.arange(len(rows))
                    t1 = tt[k, i1]
                    tt[k, i1] = INF
                    merge(rows, t1, tt.min(axis=1), 1, j, i1)

            hit = kind >= 0
            ill |= hit & ((second - best) < eps * best)
            # a candidate that takes part in the decision (the winner, or one cut out in front of it; on a miss every one) and
            # whose alpha texel a float32 uv may place next door
            ill |= np.isfinite(near_t) & (near_t <= best)
            res = dict(didHit=hit, isSphere=kind == 0, objectHitIndex=np.where(hit, bobj, 0), triIndex=btri, dst=best,
                       frontFace=np.zeros(n, bool), materialIndex=np.zeros(n, np.int64), hitPoint=np.zeros((n, 3)),
                       normal=np.zeros((n, 3)), corners=np.zeros((n, 3, 3)), ill=ill,
                       dst_bound=np.zeros(n), dst_bound_c1=np.zeros(n), point_bound=np.zeros(n), normal_bound=np.zeros(n))
            res["hitPoint"][hit] = o[hit] + best[hit, None] * d[hit]
            if maps:
                res.update(uv=np.zeros((n, 2)), fallback=np.zeros(n, bool), cutNearer=np.isfinite(cut_t) & (cut_t < best), samplerIndex=np.zeros(n, np.int64),
                           albedo=np.ones((n, 3)), mirror=np.zeros(n, bool), hx=np.zeros(n), hy=np.zeros(n), bumped=np.zeros(n, bool),
                           texel={k: np.full((n, 2), -1, np.int64) for k in MAP_SLOTS})
            self._finish_spheres(res, o, d, a, sfront)
            self._finish_triangles(res, o, d, xf, eps, maps)
            if maps:
                for mi_ in np.unique(res["materialIndex"][hit]):
                    mt = self.materials.get(int(mi_))
                    if mt is not None:
                        rows = np.flatnonzero(hit & (res["materialIndex"] == mi_))
                        res["albedo"][rows] *= mt["albedo"]
                        unmapped = res["isSphere"][rows] | (self.bound_map(mi_, "metalness") is None)
                        res["mirror"][rows] = np.where(unmapped, mt["reflectance"] != 0.0, res["mirror"][rows])
            # where the first-order count gives no bound (g, or the sphere's root of disc) the ray cannot be held to anything:
            # ill-conditioned, and counted as such, instead of passing under an infinite bound
            for k in ("dst_bound", "point_bound", "normal_bound"):
                res["ill"] |= hit & ~np.isfinite(res[k])
        return res

    def _finish_spheres(self, res, o, d, a, sfront):
        rows = np.flatnonzero(res["isSphere"])
        if not len(rows):
            return
        i = res["objectHitIndex"][rows]
        c, r, t = self.sph_c[i], self.sph_r[i], res["dst"][rows]
        p = res["hitPoint"][rows]
        front = sfront[rows]
        nrm = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True) * np.where(front, 1.0, -1.0)[:, None]
        res["normal"][rows] = nrm
        res["frontFace"][rows] = front
        res["materialIndex"][rows] = self.sph_mat[i]
        dt = sphere_dst_bound(o[rows], d[rows], c, r, front)
        dl, ol = np.linalg.norm(d[rows], axis=1), np.linalg.norm(o[rows], axis=1)
        pb = dt * dl + 2 * U32 * (ol + t * dl)
        res["dst_bound"][rows] = dt
        res["dst_bound_c1"][rows] = dt
        res["point_bound"][rows] = pb
        # normalize(p - c): the point's error and the difference's rounding over the radius, the normalisation's 5u
        res["normal_bound"][rows] = (pb + U32 * np.linalg.norm(p - c, axis=1)) / np.linalg.norm(p - c, axis=1) + 5 * U32

    def _finish_triangles(self, res, o, d, xf, eps, maps=False):
        tri_rows = np.flatnonzero(res["didHit"] & ~res["isSphere"])
        for j in np.unique(res["objectHitIndex"][tri_rows]):
            rows = tri_rows[res["objectHitIndex"][tri_rows] == j]
            mi, M, mat, sampler = self.objects[j]
            mesh = self.meshes[mi]
            Minv, op, dp = xf[j]
            k = res["triIndex"][rows]
            oo, dd, t = op[rows], dp[rows], res["dst"][rows]
            v0, e1, e2, nn = mesh.P[k, 0], mesh.e1[k], mesh.e2[k], mesh.n[k]
            r = oo - v0
            d0 = -np.einsum("ij,ij->i", dd, nn)
            q = np.cross(r, dd)
            uu = np.einsum("ij,ij->i", e2, q) / d0
            vv = -np.einsum("ij,ij->i", e1, q) / d0
            ww = 1.0 - uu - vv
            front = d0 >= 1e-8
            dlen, nlen = np.linalg.norm(dd, axis=1), mesh.nlen[k]
            res["ill"][rows] |= np.abs(d0 - 1e-8) < eps * dlen * nlen       # the winner's own facing
            N0, N1, N2 = mesh.N[k, 0], mesh.N[k, 1], mesh.N[k, 2]
            ni = ww[:, None] * N0 + uu[:, None] * N1 + vv[:, None] * N2
            M3 = M[:3, :3]
            wn = (ni * np.where(front, 1.0, -1.0)[:, None]) @ M3.T
            wnl = np.linalg.norm(wn, axis=1)
            res["normal"][rows] = wn / wnl[:, None]
            res["frontFace"][rows] = front
            res["materialIndex"][rows] = mat
            res["corners"][rows] = mesh.P[k]
            # ---- bounds (module docstring)
            W = _transform_error_unit(M, Minv)
            o1 = np.concatenate([np.abs(o[rows]), np.ones((len(rows), 1))], axis=1)
            do = np.linalg.norm(o1 @ W[:3, :].T, axis=1)
            ddv = np.linalg.norm(np.abs(d[rows]) @ W[:3, :3].T, axis=1)
            rl = np.linalg.norm(r, axis=1)
            e1l, e2l = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
            B, g, sin, cos = _bary_bound(e1l, e2l, nlen, rl, t, dlen, d0, do, ddv)
            G = (rl / dlen + t) / (cos * sin)
            T = (do + t * ddv) / (dlen * cos)
            c1 = U32 * (G + T) * g
            res["dst_bound_c1"][rows] = c1
            res["dst_bound"][rows] = DST_C * c1
            wl = np.linalg.norm(d[rows], axis=1)
            m2 = np.linalg.norm(M3, 2)
            pobj = np.abs(oo + t[:, None] * dd)
            p1 = np.concatenate([pobj, np.ones((len(rows), 1))], axis=1)
            res["point_bound"][rows] = DST_C * c1 * wl + DST_C * U32 * (
                m2 * (do + t * ddv) + m2 * (np.linalg.norm(oo, axis=1) + t * dlen) + np.linalg.norm(p1 @ np.abs(M[:3, :]).T, axis=1))
            dni = B * (np.linalg.norm(N1 - N0, axis=1) + np.linalg.norm(N2 - N0, axis=1)) + 8 * U32 * (
                np.linalg.norm(N0, axis=1) + np.linalg.norm(N1, axis=1) + np.linalg.norm(N2, axis=1))
            res["normal_bound"][rows] = (m2 * dni + 3 * U32 * np.linalg.norm(np.abs(ni) @ np.abs(M3).T, axis=1)) / wnl + 5 * U32
            if not maps:
                continue
            # ---- texture maps (module docstring, TEXTURE MAPS)
            clamp = sampler == 1
            fb = mesh.fallback[k]
            uv, spread = mesh.uv_at(k, uu, vv)
            res["uv"][rows], res["fallback"][rows], res["samplerIndex"][rows] = uv, fb, sampler
            near = np.zeros(len(rows), bool)
            for slot in MAP_SLOTS:
                tex = self.bound_map(mat, slot)
                if tex is None:
                    continue
                x, y, nr = _lookup(tex, uv, spread, B, fb, clamp, eps)
                near |= nr
                res["texel"][slot][rows] = np.stack([x, y], axis=1)
                if slot == "albedo":
                    res["albedo"][rows] = srgb8_to_linear(tex[y, x, :3])           # times the material's, in closest_hit
                elif slot == "metalness":
                    res["mirror"][rows] = tex[y, x, 0] != 0                       # the decode is 0 at byte 0 alone
                elif slot == "bump":
                    h, w = tex.shape[:2]
                    h0 = srgb8_to_linear(tex[y, x, 0])
                    hx1, hy1 = srgb8_to_linear(tex[y, texel_next(x, w, clamp), 0]), srgb8_to_linear(tex[texel_next(y, h, clamp), x, 0])
                    hx, hy = hx1 - h0, hy1 - h0
                    UV = mesh.UV[k]
                    du1, dv1 = (UV[:, 1] - UV[:, 0]).T
                    du2, dv2 = (UV[:, 2] - UV[:, 0]).T
                    det = du1 * dv2 - du2 * dv1
                    near |= (det != 0) & (np.abs(det) < eps * (np.abs(du1 * dv2) + np.abs(du2 * dv1)))
                    on = (det != 0) & ((hx != 0) | (hy != 0))
                    res["hx"][rows], res["hy"][rows], res["bumped"][rows] = hx, hy, on
                    a = np.flatnonzero(on)
                    if not len(a):
                        continue
                    Tv = e1[a] * dv2[a, None] - e2[a] * dv1[a, None]              # dP/du and dP/dv, times det: the sign is all
                    Bv = e2[a] * du1[a, None] - e1[a] * du2[a, None]              # that the normalisation leaves of it
                    sg = np.sign(det[a])[:, None]
                    Tl, Bl = np.linalg.norm(Tv, axis=1), np.linalg.norm(Bv, axis=1)
                    nil = np.linalg.norm(ni[a], axis=1)
                    nb = ni[a] / nil[:, None] - (hx[a, None] * sg * Tv / Tl[:, None] - hy[a, None] * sg * Bv / Bl[:, None])
                    wb = (nb * np.where(front[a], 1.0, -1.0)[:, None]) @ M3.T
                    wbl = np.linalg.norm(wb, axis=1)
                    res["normal"][rows[a]] = wb / wbl[:, None]
                    # the bound (module docstring, "bumped normal")
                    kT = (e1l[a] * np.abs(dv2[a]) + e2l[a] * np.abs(dv1[a])) / Tl
                    kB = (e2l[a] * np.abs(du1[a]) + e1l[a] * np.abs(du2[a])) / Bl
                    dec = 2 * DECODE_ULP * U32
                    dhx = dec * (h0[a] + hx1[a]) + 2e-9 + U32 * np.abs(hx[a])
                    dhy = dec * (h0[a] + hy1[a]) + 2e-9 + U32 * np.abs(hy[a])
                    dnb = (dni[a] / nil + 5 * U32 + dhx + dhy + U32 * np.abs(hx[a]) * (4 * kT + 7) + U32 * np.abs(hy[a]) * (4 * kB + 7)
                           + U32 * (np.abs(hx[a]) + np.abs(hy[a])) + U32 * np.linalg.norm(nb, axis=1))
                    den = wbl - m2 * dnb
                    res["normal_bound"][rows[a]] = np.where(
                        den > 0, (m2 * dnb + 3 * U32 * np.linalg.norm(np.abs(nb) @ np.abs(M3).T, axis=1)) / den + 5 * U32, np.inf)
            res["ill"][rows] |= near


def sphere_dst_bound(o, d, c, r, front):
    """First-order bound on the float32 sphere root against the float64 one, operation by operation (raytrace.comp:195-224)."""
    u = U32
    oc = c - o                                             # 1 rounding per component
    ocl, dl = np.linalg.norm(oc, axis=1), np.linalg.norm(d, axis=1)
    a = dl * dl
    b = np.einsum("ij,ij->i", oc, d)
    cc = ocl * ocl - r * r
    disc = b * b - a * cc
    da = 3 * u * a                                         # three products, two sums, all terms positive
    db = 4 * u * ocl * dl                                  # oc's rounding + three products, two sums
    dcc = 6 * u * ocl * ocl + 2 * u * r * r                # oc twice (2u) + dot (3u) + the difference (u of each side); r * r: u
    ddisc = 2 * np.abs(b) * db + 2 * u * b * b + np.abs(cc) * da + a * dcc + 2 * u * a * np.abs(cc)   # b * b, a * c: u each; the difference: u of each side
    s = np.sqrt(np.maximum(disc, 0.0))
    ds = np.where(ddisc < disc, ddisc / (2 * s) + u * s, np.inf)
    num = np.where(front, b - s, b + s)
    return (db + ds + u * np.abs(num)) / a + np.abs(num / a) * (da / a + u)   # the sum: u; the division: u; a's own error


def hits_agree(ref, got, corners_of):
    """Compares a float64 reference result with a hit record (hits_to_numpy's dict; `corners_of(object, triHitIndex)` gives the
    three object-space corner positions of the triangles the record names). Returns a dict of per-ray boolean failure masks
    (over all rays; the caller masks by ~ref['ill']) and the per-ray |dt|."""
    hit = ref["didHit"]
    g_hit = got["didHit"].astype(bool)
    both = hit & g_hit
    fail = {"didHit": hit != g_hit}
    for k in ("isSphere", "objectHitIndex", "frontFace", "materialIndex"):
        fail[k] = both & (got[k].astype(np.int64) != ref[k].astype(np.int64))
    tri = both & ~ref["isSphere"] & (got["isSphere"] == 0)
    corners = np.zeros_like(ref["corners"])
    corners[tri] = corners_of(got["objectHitIndex"][tri], got["triHitIndex"][tri])
    fail["triangle"] = tri & (np.abs(corners - ref["corners"]).reshape(len(hit), -1).max(axis=1) != 0)
    dt = np.where(both, np.abs(got["dst"].astype(np.float64) - np.where(both, ref["dst"], 0.0)), 0.0)
    fail["dst"] = both & ~(dt <= ref["dst_bound"])
    dp = np.linalg.norm(got["hitPoint"].astype(np.float64) - ref["hitPoint"], axis=1)
    fail["hitPoint"] = both & ~(dp <= ref["point_bound"])
    dn = np.linalg.norm(got["normal"].astype(np.float64) - ref["normal"], axis=1)
    fail["normal"] = both & ~(dn <= ref["normal_bound"])
    return fail, dt
