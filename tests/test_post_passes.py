"""The host logic of the AOV, denoising and temporal passes (ray_tracer_amd/csrc/post_passes.h) on the CPU:
tests/post_passes_check.cpp provokes every refusal that test_denoise and test_temporal assert on the GPU, finds the input planes of
a pass among made-up addresses, checks outputs against them, replays the call / reset / toggle / upload / resize / refusal scripts of
test_temporal and test_temporal_motion through the temporal history, and restates the image plane of a camera. What the GPU then
does by these answers is asserted by those tests."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_post_passes_on_the_cpu(tmp_path, built):
    """post_passes.cpp + temporal_motion.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan
    where they are installed."""
    exe = str(tmp_path / "post_passes_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(built.HIPCC))), "include")
    cc = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "post_passes.cpp"), os.path.join(CSRC, "temporal_motion.cpp"),
          os.path.join(ROOT, "tests", "post_passes_check.cpp"), "-o", exe]
    b = subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "post passes ok" in p.stdout
