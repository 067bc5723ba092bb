"""The device scene tables (ray_tracer_amd/csrc/scene_layout.h). On the CPU: tests/scene_layout_check.cpp derives them for
Cornell, for Cornell with 74 more objects and for hand-built meshes, and checks the numbering, the node and object tables, the
object hierarchy, spheres, emitters, maps and every refusal against the scene. On the GPU: a refused scene leaves the context
as it was."""
import ctypes as C
import os

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_tables_on_the_cpu(tmp_path, built):
    """scene.cpp + scene_layout.cpp + the checker with plain g++ (no hipcc, no device), under UBSan where it is installed."""
    exe = hostcheck.build(tmp_path, "scene_layout_check", ["scene.cpp", "scene_layout.cpp"], "scene_layout_check.cpp", sanitize="undefined")
    hostcheck.run(exe, [os.path.join(ROOT, "assets")], ok="scene layout ok")


class _WithNodes:
    """A scene's arrays with its BVH nodes replaced by an edited copy."""

    def __init__(self, scene, edit):
        self._scene = scene
        self._a = scene.arrays()
        n = self._a.bvhNodeCount
        self._nodes = (_capi.BVHNode * n)()
        C.memmove(self._nodes, self._a.bvhNodes, C.sizeof(self._nodes))
        edit(self._nodes, n)
        self._a.bvhNodes = C.cast(self._nodes, C.POINTER(_capi.BVHNode))

    def arrays(self):
        return self._a

    def counts(self):
        return self._scene.counts()


def _child_past_the_end(nodes, n):
    k = next(i for i in range(n) if nodes[i].triCount == 0)
    nodes[k].index = n


def _cycle(nodes, n):
    # an interior node whose first or second child is interior too: that child gets its parent's children, itself among them
    for p in range(n):
        if nodes[p].triCount:
            continue
        for c in (nodes[p].index, nodes[p].index + 1):
            if nodes[c].triCount == 0:
                nodes[c].index = nodes[p].index
                return
    raise AssertionError("no interior node below an interior node")


@pytest.mark.gpu
def test_a_refused_scene_leaves_the_context_as_it_was(renderer):
    s = engine.Scene()
    s.prepare_storage_buffers()
    s.set_sphere(0, (0.0, 0.1, -0.3), 0.4, 5)
    W = H = 64
    pc = engine.push_constants(W, H, singleRender=1, sampleLimit=4)

    def render():
        renderer.reset_counters()
        img = renderer.render(pc, W, H)
        c = renderer.counters()
        return img, (c["boxTests"], c["triTests"])

    renderer.upload_scene(s)
    img0, tests0 = render()
    assert tests0[0] > 0 and tests0[1] > 0
    with pytest.raises(engine.RtError, match="BVH child index out of range"):
        renderer.upload_scene(_WithNodes(s, _child_past_the_end))
    with pytest.raises(engine.RtError, match="BVH has a cycle"):
        renderer.upload_scene(_WithNodes(s, _cycle))
    renderer.update_objects(s)
    img1, tests1 = render()
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
    assert tests1 == tests0
