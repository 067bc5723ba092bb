"""The launch policy (ray_tracer_amd/csrc/launch_plan.h) on the CPU: tests/launch_plan_check.cpp restates the documented policy as
worked cases — the pipeline, the probe, the parts with their slices and grid share, the frames per dispatch, the kernel key with
its depth buckets and top-level tables, the launch shapes, the measured statistics and every tuning key — and checks the
decisions against them. What the GPU then runs by them is asserted by test_instantiations, test_lanes and the parity tests."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_plan_on_the_cpu(tmp_path, built):
    """launch_plan.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under UBSan where it is installed."""
    exe = str(tmp_path / "launch_plan_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(built.HIPCC))), "include")
    cc = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "launch_plan.cpp"),
          os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe]
    b = subprocess.run(cc + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "ubsan" in b.stderr.lower():
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "launch plan ok" in p.stdout
