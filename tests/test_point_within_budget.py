"""The resources of the radius point query kernels (ray_tracer_amd/csrc/rt_point_within.hip.h), read from the gfx950 code object
inside the built library as tests/test_ray_hits_budget.py reads the others: no instantiation of k_points_within and no
k_points_within_resolve spills a register or has a private segment (the lists live in LDS or in a ctx buffer, never in scratch),
the shallow search fits its 24 KB stack and 24 KB of lists in 48 KB of LDS (three work-groups of it on a CU's 160 KB), the deep
one the 64 KB a work-group may have, and the resolve uses none."""
import re

import pytest

from util import code_object


@pytest.fixture(scope="module")
def kernels(built):
    return {n: k for n, k in code_object().kernels(built.LIB).items() if re.match(r"void k_points_within(_resolve)?<", n)}


def test_every_instantiation_is_there(kernels):
    assert sorted(kernels) == ["void k_points_within<24, false>", "void k_points_within<64, true>", "void k_points_within_resolve<256>"]


def test_no_spills_and_no_private_segment(kernels):
    assert len(kernels) == 3
    for name, k in kernels.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs, {k['.sgpr_spill_count']} SGPRs spilled"
        assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"
        assert not k.get(".uses_dynamic_stack", False), name


def test_lds_of_the_two_searches(kernels):
    assert kernels["void k_points_within<24, false>"][".group_segment_fixed_size"] <= 48 * 1024
    assert kernels["void k_points_within<64, true>"][".group_segment_fixed_size"] <= 64 * 1024
    assert kernels["void k_points_within_resolve<256>"][".group_segment_fixed_size"] == 0
