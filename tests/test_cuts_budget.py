"""The resources of the cut query kernel (ray_tracer_amd/csrc/rt_tri_cut.hip.h), read from the gfx950 code object inside the built
library as tests/test_triangles_budget.py reads its kernel's, for its reasons: exactly the two declared instantiations of
k_tris_cut (the search computes the kept cuts itself; there is no resolve kernel); neither spills a register, has a private
segment or a dynamic stack; the shallow search fits its 24 KB stack and 16 KB of key lists in 48 KB of LDS (three work-groups of
it on a CU's 160 KB) and the deep one the 64 KB a work-group may have; and the register count is not what limits residency below
what LDS allows: 168 VGPRs for three waves a SIMD, 256 for the deep kernel's one."""
import re

import pytest

from util import code_object

SHALLOW, DEEP = "void k_tris_cut<24, false>", "void k_tris_cut<64, true>"


@pytest.fixture(scope="module")
def kernels(built):
    return {n: k for n, k in code_object().kernels(built.LIB).items() if re.match(r"void k_(tris_cut|cuts_)", n)}


def test_exactly_the_declared_instantiations(kernels):
    assert sorted(kernels) == [SHALLOW, DEEP]


def test_no_spills_no_private_segment_no_dynamic_stack(kernels):
    assert len(kernels) == 2
    for name, k in kernels.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs, {k['.sgpr_spill_count']} SGPRs spilled"
        assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"
        assert not k.get(".uses_dynamic_stack", False), name


def test_lds_of_the_two_searches(kernels):
    assert kernels[SHALLOW][".group_segment_fixed_size"] <= 48 * 1024
    assert kernels[DEEP][".group_segment_fixed_size"] <= 64 * 1024


def test_registers_do_not_limit_residency_below_what_lds_allows(kernels):
    for name, k in kernels.items():
        print(f"{name}: {k['.vgpr_count']} VGPRs ({k.get('.agpr_count', 0)} AGPRs), {k['.sgpr_count']} SGPRs, {k['.group_segment_fixed_size']} bytes of LDS")
    assert kernels[SHALLOW][".vgpr_count"] <= 168
    assert kernels[DEEP][".vgpr_count"] <= 256
