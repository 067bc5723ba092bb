"""What the radiance queries (rt_query_radiance and its _host form) refuse before anything is allocated, the pieces a batch runs in,
the bytes of its arrays and the frame's seed (ray_tracer_amd/csrc/radiance_queries.h), on the CPU:
tests/radiance_queries_check.cpp provokes every refusal with made-up addresses, in the stated order, with its message, covers
[0, n) with the pieces for n = 0, 1, 1023, 1024, 1025 and 3 x 1024 + 5 at "radiance_max_kslots" 1, checks the byte counts with and without ids
(that the staged arrays are aligned and do not overlap: tests/test_host_staging_host.py), and prints startingSeed for frameCount 0, 3 and 2^32 - 1, which is compared here
with the oracle's random() pushed through uint(random(frameCount) * 23892183.f)."""
import re

import numpy as np

from oracle import pyoracle

import hostcheck


def test_radiance_query_checks_on_the_cpu(tmp_path, built):
    """radiance_queries.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they
    are installed."""
    exe = hostcheck.build(tmp_path, "radiance_queries_check", ["radiance_queries.cpp"], "radiance_queries_check.cpp", rocm=False)
    out = hostcheck.run(exe, ok="radiance queries ok")
    seeds = {int(f): int(s) for f, s in re.findall(r"^seed (\d+) (\d+)$", out, re.M)}
    assert sorted(seeds) == [0, 3, 2**32 - 1], out
    for frame, seed in seeds.items():
        _, r = pyoracle.random(frame)
        assert seed == int(np.uint32(np.float32(r) * np.float32(23892183.0))), (frame, seed, r)
    assert seeds[0] == 721543 and seeds[3] == 11858218   # (tests/test_paths_float64.py: test_frame_count_seeds has them by hand)
