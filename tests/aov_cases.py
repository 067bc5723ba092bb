"""What the tests of the first-hit planes (rt_render_aovs) and of the guide planes (rt_render_guides) share: the plane names, a scene's upload with its textures, and the checks of records against hits."""
import numpy as np

from util import EditedScene


MISS_DST = np.float32(99999999.0)   # RT_MISS_DST
PLANES = ("depth", "normal", "position", "albedo", "ray_dir", "object", "triangle", "material", "hit", "sphere", "front_face")


# ---------------------------------------------------------------- GPU helpers
def _upload(renderer, s):
    if isinstance(s, EditedScene):
        renderer.upload_scene(s.scene)
        for what in ("objects", "materials", "spheres"):
            s.push(renderer, what)
    else:
        renderer.upload_scene(s)


def _as_hits(a):
    """The planes as the RtHit fields of rt_trace_rays (a miss: zeros beside dst)."""
    h = a["hit"].reshape(-1)
    z = lambda x: np.where(h, x.reshape(-1), 0).astype(np.uint32)   # noqa: E731
    return dict(dst=a["depth"].reshape(-1), didHit=h.astype(np.uint32), isSphere=a["sphere"].reshape(-1).astype(np.uint32),
                objectHitIndex=z(a["object"]), triHitIndex=z(a["triangle"]), materialIndex=z(a["material"]),
                frontFace=a["front_face"].reshape(-1).astype(np.uint32), hitPoint=a["position"].reshape(-1, 3),
                normal=a["normal"].reshape(-1, 3))


def _check_misses(a):
    m = ~a["hit"]
    assert np.all(a["depth"][m] == MISS_DST)
    for k in ("normal", "position", "albedo"):
        assert not a[k][m].any()
    for k in ("object", "triangle", "material"):
        assert np.all(a[k][m] == 0xFFFFFFFF)
    assert not (a["sphere"][m].any() or a["front_face"][m].any())


# ---------------------------------------------------------------- 3. albedo
def _albedos(s):
    arr = s.arrays()
    return np.array([list(arr.materials[i].albedo) for i in range(arr.materialCount)], np.float32)
