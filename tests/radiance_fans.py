"""TEST INFRASTRUCTURE — the batch the radiance-query tests share: three 32 x 24 fans of camera rays from three eye points with
different rotations inside the Cornell box + bunny scene, one behind the other, the last 5 rays dropped: n = 2299, no multiple of
64 or 256. The origins differ per ray, so a sample that restarts from one origin for all shows in two fans of three."""
import numpy as np

from ray_tracer_amd import engine
from util import model_scene

FW, FH = 32, 24
DROP = 5
N = 3 * FW * FH - DROP          # 2299
# eye point, camera angles in degrees
EYES = (((-0.3, -0.2, -0.9), (-5.0, 20.0, 2.0)),
        ((0.5, -0.3, -0.6), (0.0, -35.0, -3.0)),
        ((0.0, -1.1, -0.5), (-40.0, 0.0, 0.0)))


def scene():
    """The Cornell box, the bunny on its floor, a glass sphere (model_scene's) and a mirror sphere beside it."""
    s = model_scene("bunny.obj", spheres=True)
    s.set_sphere(1, (-0.55, 0.15, -0.2), 0.3, 4)
    return s


def fan_constants(k, samples, bounces, frame=0, **more):
    """The push constants whose rt_render is fan k."""
    pos, angles = EYES[k]
    return engine.push_constants(FW, FH, singleRender=1, sampleLimit=samples, bounceLimit=bounces, frameCount=frame, pos=pos, cameraAngles=angles, **more)


def batch(dirs_of_fan):
    """(origins (N, 3), dirs (N, 3), ids (N,): each fan's own pixel indices) from dirs_of_fan(k) -> the (FH * FW, 3) float32
    directions of fan k in row-major order."""
    o, d, ids = [], [], []
    for k, (pos, _) in enumerate(EYES):
        dk = np.asarray(dirs_of_fan(k), np.float32).reshape(FW * FH, 3)
        d.append(dk)
        o.append(np.repeat(np.asarray(pos, np.float32)[None], FW * FH, 0))
        ids.append(np.arange(FW * FH, dtype=np.uint32))
    cut = lambda a: np.ascontiguousarray(np.concatenate(a)[:N])   # noqa: E731
    return cut(o), cut(d), cut(ids)


def fan_rows(k):
    """The rows of the batch that are fan k's pixels [0, count)."""
    first = k * FW * FH
    return first, min(FW * FH, N - first)
