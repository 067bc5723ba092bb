"""What the ray queries (rt_query_closest, rt_query_occluded and their _host forms) and rt_render_ao refuse before anything is
allocated, and the slot and byte arithmetic of a batch (ray_tracer_amd/csrc/ray_queries.h), on the CPU: tests/ray_queries_check.cpp
provokes every refusal with made-up addresses, in the stated order, with its message, covers n == 0 and the arithmetic at
n = 1, 63, 64, 65 and 2^30 - 1, and runs rt_ao_rays_host, which lives in the same host-only unit, on two records."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ray_query_checks_on_the_cpu(tmp_path, built):
    """ray_queries.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they are
    installed."""
    exe = str(tmp_path / "ray_queries_check")
    cc = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
          os.path.join(CSRC, "ray_queries.cpp"), os.path.join(ROOT, "tests", "ray_queries_check.cpp"), "-o", exe]
    b = subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "ray queries ok" in p.stdout
