"""What rt_render_guides refuses before anything is allocated (ray_tracer_amd/csrc/post_passes.h: check_guides and the tile checks it
shares with rt_render and rt_render_aovs) on the CPU: tests/guides_check.cpp provokes every refusal that test_guides asserts through
the C ABI on the GPU, in their order, and finds the overlapping plane pairs among made-up addresses."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_guide_checks_on_the_cpu(tmp_path, built):
    """post_passes.cpp + temporal_motion.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan
    where they are installed."""
    exe = str(tmp_path / "guides_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(built.HIPCC))), "include")
    cc = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "post_passes.cpp"), os.path.join(CSRC, "temporal_motion.cpp"),
          os.path.join(ROOT, "tests", "guides_check.cpp"), "-o", exe]
    b = subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "guides ok" in p.stdout
