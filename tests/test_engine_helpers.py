"""The small rules engine.py states once (no GPU)."""
import pytest

from ray_tracer_amd import engine


@pytest.mark.parametrize("height,row0,rowStride,rows", [(5, 1, 2, 2), (5, 4, 2, 1), (1, 0, 3, 1)])
def test_tile_rows_by_hand(height, row0, rowStride, rows):
    assert engine._tile_rows(height, row0, rowStride) == rows


def test_tile_rows_are_the_rows_of_the_range():
    for height in range(1, 10):
        for row0 in range(height):
            for rowStride in range(1, 5):
                assert engine._tile_rows(height, row0, rowStride) == len(range(row0, height, rowStride)), (height, row0, rowStride)
