"""The resources of the lightmap texel kernels (ray_tracer_amd/csrc/rt_texels.hip.h), read from the gfx950 code object inside the
built library as tests/test_irradiance_budget.py reads the others: exactly the expected kernels and scan instantiations, none
spills a register or has a private segment (the 64-bit edge functions and the snapped corners stay in registers), and the only
LDS is the scan's: one value per wave of a group, in the scan's own kernels and in the compaction, which scans its flags."""
import re

import pytest

from util import code_object

PLAIN = ["k_texel_bins", "k_texel_cover", "k_texel_resolve", "k_texel_scatter", "k_texel_dilate"]
SCANNING = {"k_texel_compact": 16,
            "void k_scan_local<unsigned long long, ScanLoadU32>": 32, "void k_scan_local<unsigned long long, ScanLoadSame<unsigned long long>>": 32,
            "void k_scan_local<unsigned int, ScanLoadCovered>": 16, "void k_scan_local<unsigned int, ScanLoadSame<unsigned int>>": 16}
ADDING = ["void k_scan_add<unsigned long long>", "void k_scan_add<unsigned int>"]


@pytest.fixture(scope="module")
def kernels(built):
    return {re.sub(r"\(.*\)$", "", n).replace("> >", ">>"): k for n, k in code_object().kernels(built.LIB).items() if re.match(r"(void )?k_(texel|scan)_", n)}


def test_exactly_the_expected_kernels(kernels):
    assert sorted(kernels) == sorted(PLAIN + list(SCANNING) + ADDING)


def test_no_spills_no_private_segment_and_lds_only_in_the_scan(kernels):
    assert len(kernels) == len(PLAIN) + len(SCANNING) + len(ADDING)
    for name, k in kernels.items():
        print(name, "VGPRs", k.get(".vgpr_count"), "SGPRs", k.get(".sgpr_count"), "LDS", k[".group_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs, {k['.sgpr_spill_count']} SGPRs spilled"
        assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"
        assert not k.get(".uses_dynamic_stack", False), name
        assert k[".group_segment_fixed_size"] == SCANNING.get(name, 0), f"{name}: {k['.group_segment_fixed_size']} bytes of LDS"
        assert k[".max_flat_workgroup_size"] == (64 if name == "k_texel_resolve" else 256), name
