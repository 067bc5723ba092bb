"""The host-only unit of the signed point queries on the CPU (ray_tracer_amd/csrc/mesh_topology.h; the rule include/rt_point_side.h;
DESIGN.md, "Signed point queries").

tests/mesh_topology_check.cpp, built with plain g++ under the sanitizers, holds hand-made meshes with their exact rows and statistics
(a tetrahedron with its adjacency spelled out, reversed faces, shared vertices, open, non-orientable, degenerate, flat and long-fan
meshes), every refusal message, the orientation table, rt_point_triangle_feature against the (u, v) of rt_point_triangle over random
and degenerate triangles, and rt_angle against double atan2 within 1e-6 rad. rt_scene_topology is then held to the edge-sharing counts
of the project's assets, counted here with numpy."""
import os

import numpy as np
import pytest

from ray_tracer_amd import engine

import hostcheck
from point_query_cases import _bare_scene


@pytest.fixture(scope="module")
def checked(tmp_path_factory, built):
    d = tmp_path_factory.mktemp("mesh_topology")
    exe = hostcheck.build(d, "mesh_topology_check", ["mesh_topology.cpp", "point_queries.cpp"], "mesh_topology_check.cpp", opt="-O1")
    return hostcheck.run(exe, ok="mesh topology ok")


def test_hand_made_meshes_refusals_orientation_and_the_units_of_the_rule(checked):
    worst = [float(line.split()[-1]) for line in checked.splitlines() if line.startswith("rt_angle worst")]
    assert len(worst) == 1 and worst[0] <= 1e-6


def _edge_counts(path):
    """Edges of an OBJ file after welding by position, by how many triangles share them: {uses: edges}, and the triangle count."""
    v, faces = [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == "f":
                idx = [int(x.split("/")[0]) - 1 for x in p[1:]]
                faces += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    v = np.array(v, np.float32) + np.float32(0.0)
    _, weld = np.unique(v, axis=0, return_inverse=True)
    f = weld[np.array(faces)]
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    uses, n = np.unique(counts, return_counts=True)
    return dict(zip(uses.tolist(), n.tolist())), len(faces)


@pytest.mark.parametrize("asset, shared_by_two, others, signable", [
    ("cube.obj", 18, {}, True),
    ("bunny.obj", 1261, {1: 55, 3: 41, 4: 6}, False),
    ("klein_bottle.obj", 53760, {}, False)])
def test_scene_topology_on_the_assets(asset, shared_by_two, others, signable):
    path = os.path.join(engine.ASSET_DIR, asset)
    counts, triangles = _edge_counts(path)
    assert counts.pop(2) == shared_by_two and counts == others
    s = _bare_scene()
    s.read_obj(path, engine.placement(rotation=(10, 20, 30), scale=(1.0, -0.5, 2.0)), 0)
    (t,) = s.topology()
    assert t["triangles"] == triangles and t["degenerateTriangles"] == 0
    assert t["boundaryEdges"] == others.get(1, 0) and t["nonManifoldEdges"] == sum(n for k, n in others.items() if k > 2)
    assert t["orientation"] == -1
    if signable:
        assert (t["components"], t["signableComponents"], t["signableTriangles"]) == (1, 1, triangles)
    else:
        assert t["signableComponents"] == 0 and t["signableTriangles"] == 0 and t["flippedTriangles"] == 0
    if not others and not signable:      # closed, and still not signable: not orientable (its volume would not be zero)
        assert t["boundaryEdges"] == 0 and t["nonManifoldEdges"] == 0


def test_two_objects_that_place_one_mesh_share_its_rows_and_differ_in_orientation():
    s = _bare_scene()
    cube = os.path.join(engine.ASSET_DIR, "cube.obj")
    s.read_obj(cube, engine.placement(position=(-2, 0, 0)), 0)
    s.read_obj(cube, engine.placement(position=(2, 0, 0), scale=(1, 1, -1)), 0)
    a, b = s.topology()
    assert a["orientation"] == 1 and b["orientation"] == -1
    assert {k: v for k, v in a.items() if k != "orientation"} == {k: v for k, v in b.items() if k != "orientation"}
