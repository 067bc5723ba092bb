"""Deforming meshes in place, on the CPU (ray_tracer_amd/csrc/mesh_refit.h). tests/mesh_refit_check.cpp, built with plain g++ from
scene.cpp, scene_layout.cpp and mesh_refit.cpp, checks the rule against the builder's boxes, the refit plan against the device
numbering, rt_scene_update_points against the vertices it was given and every refusal; it runs once more under ASan + UBSan.
For every deformed case it leaves the arrays before and after in a directory, and this file restates the rule in numpy
(`numpy_refit`: nothing shared with the C++) and compares the refit nodes bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("cornell", "cornell_cube", "cornell_bunny", "two_bunnies")

NODE = np.dtype([("box", np.float32, (3, 2)), ("index", np.uint32), ("triCount", np.uint32)])   # BVHNode: (min, max) per axis


def numpy_refit(nodes, tri, pos, root):
    """The rule: a leaf starts from (+1e30, -1e30) and grows by its triangles in order, corners v0, v1, v2, with lo = p < lo ? p : lo
    and hi = hi < p ? p : hi; an interior node is its left child's box grown by its right child's with the same comparisons."""
    n = nodes[root]
    if n["triCount"]:
        lo, hi = np.full(3, 1e30, np.float32), np.full(3, -1e30, np.float32)
        for p in pos[tri[n["index"]:n["index"] + n["triCount"]].reshape(-1)]:
            lo, hi = np.where(p < lo, p, lo), np.where(hi < p, p, hi)
    else:
        for c in (n["index"], n["index"] + 1):
            numpy_refit(nodes, tri, pos, c)
        (lo, hi), (rlo, rhi) = nodes[n["index"]]["box"].T.copy(), nodes[n["index"] + 1]["box"].T
        lo, hi = np.where(rlo < lo, rlo, lo), np.where(hi < rhi, rhi, hi)
    nodes[root]["box"][:, 0], nodes[root]["box"][:, 1] = lo, hi


def _build(directory, name, **how):
    return hostcheck.build(directory, name, ["scene.cpp", "scene_layout.cpp", "mesh_refit.cpp"], "mesh_refit_check.cpp", opt="-O1", **how)


@pytest.fixture(scope="module")
def checked(tmp_path_factory, built):
    """The check program, built without sanitizers and run once: its output directory."""
    d = tmp_path_factory.mktemp("mesh_refit")
    hostcheck.run(_build(d, "mesh_refit_check", sanitize=None), [os.path.join(ROOT, "assets"), d], ok="mesh refit ok")
    return d


def test_rule_plan_update_and_refusals_on_the_cpu(checked):
    assert os.path.exists(checked / "two_bunnies_2_nodes_after.bin")


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _sanitizers_installed(tmp_path):
    """Asked before the check program is built: an empty main compiled, linked and run with the same sanitizer flags."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp_path / "probe")
    b = subprocess.run(["g++", str(src), "-o", exe] + SANITIZE, capture_output=True, text=True, timeout=120)
    return b.returncode == 0 and subprocess.run([exe], capture_output=True, timeout=60).returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_check_program_under_asan_and_ubsan(tmp_path, built):
    if not _sanitizers_installed(tmp_path):
        pytest.skip("the sanitizer runtimes are not installed")
    exe = _build(tmp_path, "mesh_refit_check_san", fallback=False, extra=["-g"])
    hostcheck.run(exe, [os.path.join(ROOT, "assets"), tmp_path], ok="mesh refit ok", timeout=300)


@pytest.mark.parametrize("kind", (0, 1, 2), ids=("all_points", "sub_range", "straddles_two_meshes"))
@pytest.mark.parametrize("scene", SCENES)
def test_host_refit_equals_the_numpy_restatement_bit_for_bit(checked, scene, kind):
    load = lambda name, dtype: np.fromfile(checked / f"{scene}_{kind}_{name}.bin", dtype=dtype)
    tri = load("triangles", np.uint32).reshape(-1, 12)[:, :3]
    pos = load("points", np.float32).reshape(-1, 8)[:, :3]
    before, after, roots = load("nodes_before", NODE), load("nodes_after", NODE), load("roots", np.uint32)
    assert len(roots) >= (2 if kind == 2 else 1)
    expect = before.copy()
    for r in roots:
        numpy_refit(expect, tri, pos, int(r))
    assert expect.tobytes() == after.tobytes(), f"{int((expect.view(np.uint8).reshape(-1, 32) != after.view(np.uint8).reshape(-1, 32)).any(axis=1).sum())} nodes differ"
    assert (kind != 0) or not np.array_equal(before["box"], after["box"])
