"""The launch plan's side of the wide work-groups (k_trace_pw_wide) on the CPU: tests/wide_plan_check.cpp restates when
trace_kernel_key returns the wide key (a 20-entry stack, the table of hot_pairs 2, no culling, no counters, a dispatch of at least
wide_min_kslots x 1024 paths) and that every other key is what it was, the knob with its range errors, the grid trace_shape gives a
launch of wide groups, and the LDS sum of the shipped shape. tests/test_launch_plan.py pins the rest of the plan; what the GPU runs
by these decisions is tests/test_wide_groups.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_wide_plan_on_the_cpu(tmp_path, built):
    """launch_plan.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under UBSan where it is installed."""
    exe = str(tmp_path / "wide_plan_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(built.HIPCC))), "include")
    cc = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "launch_plan.cpp"),
          os.path.join(ROOT, "tests", "wide_plan_check.cpp"), "-o", exe]
    b = subprocess.run(cc + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "ubsan" in b.stderr.lower():
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "wide plan ok" in p.stdout
