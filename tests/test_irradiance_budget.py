"""The resources of the two baked-light kernels (ray_tracer_amd/csrc/rt_irradiance.hip.h), read from the gfx950 code object inside
the built library as tests/test_sweep_budget.py reads the others: exactly the instantiations k_irradiance_rays<false | true> and
k_irradiance_gather<false | true>, none spills a register or has a private segment (the probe form's 27 partial sums and nine SH
weights stay in registers), and the fold across the lanes takes no LDS of the work-group's."""
import re

import pytest

from util import code_object


@pytest.fixture(scope="module")
def kernels(built):
    return {re.sub(r"\(IrradianceArgs\)$", "", n): k for n, k in code_object().kernels(built.LIB).items() if re.match(r"void k_irradiance_", n)}


def test_exactly_the_four_instantiations(kernels):
    assert sorted(kernels) == ["void k_irradiance_gather<false>", "void k_irradiance_gather<true>", "void k_irradiance_rays<false>",
                               "void k_irradiance_rays<true>"]


def test_no_spills_no_private_segment_no_lds(kernels):
    assert len(kernels) == 4
    for name, k in kernels.items():
        print(name, "VGPRs", k.get(".vgpr_count"), "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs, {k['.sgpr_spill_count']} SGPRs spilled"
        assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"
        assert not k.get(".uses_dynamic_stack", False), name
        assert k[".group_segment_fixed_size"] == 0, f"{name}: {k['.group_segment_fixed_size']} bytes of LDS"
        assert k[".max_flat_workgroup_size"] == 256, name
