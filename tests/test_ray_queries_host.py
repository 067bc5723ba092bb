"""What the ray queries (rt_query_closest, rt_query_occluded and their _host forms) and rt_render_ao refuse before anything is
allocated, and the slot and byte arithmetic of a batch (ray_tracer_amd/csrc/ray_queries.h), on the CPU: tests/ray_queries_check.cpp
provokes every refusal with made-up addresses, in the stated order, with its message, covers n == 0 and the arithmetic at
n = 1, 63, 64, 65 and 2^30 - 1, and runs rt_ao_rays_host, which lives in the same host-only unit, on two records."""
import hostcheck


def test_ray_query_checks_on_the_cpu(tmp_path, built):
    """ray_queries.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan where they are
    installed."""
    exe = hostcheck.build(tmp_path, "ray_queries_check", ["ray_queries.cpp"], "ray_queries_check.cpp", rocm=False)
    hostcheck.run(exe, ok="ray queries ok")
