"""The launch plan's side of the wide work-groups (k_trace_pw_wide) on the CPU: tests/wide_plan_check.cpp restates when
trace_kernel_key returns the wide key (a 20-entry stack, the table of hot_pairs 2, no culling, no counters, a dispatch of at least
wide_min_kslots x 1024 paths) and that every other key is what it was, the knob with its range errors, the grid trace_shape gives a
launch of wide groups, and the LDS sum of the shipped shape. tests/test_launch_plan.py pins the rest of the plan; what the GPU runs
by these decisions is tests/test_wide_groups.py."""
import hostcheck


def test_wide_plan_on_the_cpu(tmp_path, built):
    """launch_plan.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under UBSan where it is installed."""
    exe = hostcheck.build(tmp_path, "wide_plan_check", ["launch_plan.cpp"], "wide_plan_check.cpp", sanitize="undefined")
    hostcheck.run(exe, ok="wide plan ok")
