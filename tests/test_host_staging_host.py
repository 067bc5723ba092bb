"""Where the arrays of a _host call lie in the ctx staging buffer (ray_tracer_amd/csrc/host_staging.h: stage_layout), on the CPU:
tests/host_staging_check.cpp lays out the part lists of every _host entry point (the ray, point and radiance queries with and
without their optional array, for n = 0, 1, 63, 64, 65, 255, 256, 257, 1024, 2299 and 2^30 - 1; the planes of the denoiser, the temporal
accumulation, the sample map, the strips and the math probe) and checks the one rule on each: the first part at 0, every offset
and the total a multiple of 256, no part reaching into the next, an absent part at the next one's offset, less than 256 bytes of
padding behind any part, size_t arithmetic past 32 bits, the pinned offsets of a batch of 65, nothing for an all-absent list, and a
refusal of more parts than the rule holds."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stage_layout_on_the_cpu(tmp_path):
    """host_staging.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they are
    installed, as a program of its own."""
    exe = str(tmp_path / "host_staging_check")
    cc = ["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
          os.path.join(CSRC, "host_staging.cpp"), os.path.join(ROOT, "tests", "host_staging_check.cpp"), "-o", exe]
    b = subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "host staging ok" in p.stdout
