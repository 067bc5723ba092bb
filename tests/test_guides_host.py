"""What rt_render_guides refuses before anything is allocated (ray_tracer_amd/csrc/post_passes.h: check_guides and the tile checks it
shares with rt_render and rt_render_aovs) on the CPU: tests/guides_check.cpp provokes every refusal that test_guides asserts through
the C ABI on the GPU, in their order, and finds the overlapping plane pairs among made-up addresses."""
import hostcheck


def test_guide_checks_on_the_cpu(tmp_path, built):
    """post_passes.cpp + temporal_motion.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan
    where they are installed."""
    exe = hostcheck.build(tmp_path, "guides_check", ["post_passes.cpp", "temporal_motion.cpp"], "guides_check.cpp")
    hostcheck.run(exe, ok="guides ok")
