"""The host logic of the AOV, denoising and temporal passes (ray_tracer_amd/csrc/post_passes.h) on the CPU:
tests/post_passes_check.cpp provokes every refusal that test_denoise and test_temporal assert on the GPU, finds the input planes of
a pass among made-up addresses, checks outputs against them, replays the call / reset / toggle / upload / resize / refusal scripts of
test_temporal and test_temporal_motion through the temporal history, and restates the image plane of a camera. What the GPU then
does by these answers is asserted by those tests."""
import hostcheck


def test_post_passes_on_the_cpu(tmp_path, built):
    """post_passes.cpp + temporal_motion.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan
    where they are installed."""
    exe = hostcheck.build(tmp_path, "post_passes_check", ["post_passes.cpp", "temporal_motion.cpp"], "post_passes_check.cpp")
    hostcheck.run(exe, ok="post passes ok")
