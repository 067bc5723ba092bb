"""The launch policy (ray_tracer_amd/csrc/launch_plan.h) on the CPU: tests/launch_plan_check.cpp restates the documented policy as
worked cases — the pipeline, the probe, the parts with their slices and grid share, the frames per dispatch, the kernel key with
its depth buckets and top-level tables, the launch shapes, the measured statistics and every tuning key — and checks the
decisions against them. What the GPU then runs by them is asserted by test_instantiations, test_lanes and the parity tests."""
import hostcheck


def test_launch_plan_on_the_cpu(tmp_path, built):
    """launch_plan.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under UBSan where it is installed."""
    exe = hostcheck.build(tmp_path, "launch_plan_check", ["launch_plan.cpp"], "launch_plan_check.cpp", sanitize="undefined")
    hostcheck.run(exe, ok="launch plan ok")
