"""The host logic of the per-pixel sample counts on the CPU: tests/sample_map_check.cpp provokes every parameter refusal of
rt_build_sample_map, the rule for the ctx-owned moments plane (none yet, another size) and rt_render_sampled's refusal of a map with
the debug heat maps (ray_tracer_amd/csrc/post_passes.h); and the tiling helper that cuts a whole-frame map into a rank's rows."""

import numpy as np
import pytest

import hostcheck


def test_sample_map_checks_on_the_cpu(tmp_path, built):
    """post_passes.cpp + temporal_motion.cpp + the checker with plain g++ (no hipcc, no HIP runtime, no device), under ASan and UBSan
    where they are installed."""
    exe = hostcheck.build(tmp_path, "sample_map_check", ["post_passes.cpp", "temporal_motion.cpp"], "sample_map_check.cpp")
    hostcheck.run(exe, ok="sample map ok")


@pytest.mark.parametrize("H,world", [(33, 1), (33, 2), (33, 4), (33, 8), (8, 8), (5, 8), (1, 3), (1080, 7)])
def test_a_ranks_rows_of_a_whole_frame_map(H, world):
    """sample_map_rows(map, r, N) is the map of rows r, r + N, ... in order: what rank r hands to rt_render_sampled with row0 = r,
    rowStride = N and nRows = len(rows_of_rank) — also where N does not divide the height, and for ranks that get no row at all."""
    from ray_tracer_amd import tiling
    W = 7
    whole = (np.arange(H * W, dtype=np.uint32).reshape(H, W) * 3 + 1)
    seen = np.zeros(H, bool)
    for rank in range(world):
        rows = list(tiling.rows_of_rank(H, rank, world))
        part = tiling.sample_map_rows(whole, rank, world)
        assert part.shape == (len(rows), W) and part.dtype == np.uint32 and part.flags["C_CONTIGUOUS"]
        assert len(rows) == (H - rank + world - 1) // world if rank < H else len(rows) == 0   # rt_render's nRows for this tile
        assert len(rows) <= tiling.max_rows(H, world)
        for k, y in enumerate(rows):
            assert y == rank + k * world and np.array_equal(part[k], whole[y])
            seen[y] = True
        part[...] = 0   # a copy: the whole-frame map is not written through it
    assert seen.all() and (whole > 0).all()


def test_a_ranks_rows_of_a_tensor_map():
    import torch
    from ray_tracer_amd import tiling
    whole = torch.arange(33 * 5, dtype=torch.int32).reshape(33, 5)
    part = tiling.sample_map_rows(whole, 2, 4)
    assert part.is_contiguous() and torch.equal(part, whole[2::4])


def test_cli_flags():
    from ray_tracer_amd import render
    p = render.build_parser()
    assert p.parse_args([]).adaptive is None
    assert p.parse_args(["--temporal-frames", "4", "--adaptive", "0.05"]).adaptive == 0.05
    with pytest.raises(SystemExit):
        render.main(["--adaptive", "0.05"])   # needs --temporal-frames
