"""Where the arrays of a _host call lie in the ctx staging buffer (ray_tracer_amd/csrc/host_staging.h: stage_layout), on the CPU:
tests/host_staging_check.cpp lays out the part lists of every _host entry point (the ray, point and radiance queries with and
without their optional array, for n = 0, 1, 63, 64, 65, 255, 256, 257, 1024, 2299 and 2^30 - 1; the planes of the denoiser, the temporal
accumulation, the sample map, the strips and the math probe) and checks the one rule on each: the first part at 0, every offset
and the total a multiple of 256, no part reaching into the next, an absent part at the next one's offset, less than 256 bytes of
padding behind any part, size_t arithmetic past 32 bits, the pinned offsets of a batch of 65, nothing for an all-absent list, and a
refusal of more parts than the rule holds."""
import hostcheck


def test_stage_layout_on_the_cpu(tmp_path):
    """host_staging.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they are
    installed, as a program of its own."""
    exe = hostcheck.build(tmp_path, "host_staging_check", ["host_staging.cpp"], "host_staging_check.cpp", rocm=False, fp_contract_off=False)
    hostcheck.run(exe, ok="host staging ok")
