"""The resources of the sphere sweep kernel (ray_tracer_amd/csrc/rt_sweep.hip.h), read from the gfx950 code object inside the
built library as tests/test_point_within_budget.py reads the others: exactly the two instantiations of k_sweep_spheres, neither
spills a register or has a private segment (the rule's six feature times stay in registers, the stack lives in LDS), the shallow
one fits its 24 entries of two words in 48 KB of LDS (three work-groups of it on a CU's 160 KB), the deep one its 64 entries of
one word in the 64 KB a work-group may have."""
import re

import pytest

from util import code_object


@pytest.fixture(scope="module")
def kernels(built):
    return {n: k for n, k in code_object().kernels(built.LIB).items() if re.match(r"void k_sweep_spheres<", n)}


def test_exactly_the_two_instantiations(kernels):
    assert sorted(kernels) == ["void k_sweep_spheres<24, true>", "void k_sweep_spheres<64, false>"]


def test_no_spills_and_no_private_segment(kernels):
    assert len(kernels) == 2
    for name, k in kernels.items():
        print(name, "VGPRs", k.get(".vgpr_count"), "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs, {k['.sgpr_spill_count']} SGPRs spilled"
        assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"
        assert not k.get(".uses_dynamic_stack", False), name


def test_lds_of_the_two_instantiations(kernels):
    assert kernels["void k_sweep_spheres<24, true>"][".group_segment_fixed_size"] <= 48 * 1024
    assert kernels["void k_sweep_spheres<64, false>"][".group_segment_fixed_size"] <= 64 * 1024
