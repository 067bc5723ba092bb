"""The register arithmetic that lets a shading wave sit beside six traversal waves on every SIMD, read from the gfx950 code object
inside the built library (tools/code_object.py), as tests/test_wide_budget.py reads the wide kernel's other budgets.

A SIMD has 512 VGPRs per lane, handed out in eights. Six waves of k_trace_pw_wide<20, 192, 768> (two 768-thread groups per CU)
at 72 registers leave 512 - 6 x 72 = 80: one wave of k_shade, if k_shade needs no more than 80. At 73 the traversal takes 80 each
and leaves 32, and k_shade runs only in the half-CU slots a finished group gives back. Neither kernel may pay for the squeeze with
a spill, and seven waves share a SIMD's 800 SGPRs, handed out in sixteens, only at 112 or fewer each (7 x 112 = 784)."""
import re

import pytest

from util import code_object

WIDE = "void k_trace_pw_wide<20, 192, 768>"


@pytest.fixture(scope="module")
def kernels(built):
    return code_object().kernels(built.LIB)


def _allocated(vgprs):
    return (vgprs + 7) // 8 * 8


def test_one_shading_wave_fits_beside_six_wide_traversal_waves(kernels):
    assert [n for n in kernels if re.match(r"void k_trace_pw_wide<", n)] == [WIDE]
    wide, shade = kernels[WIDE][".vgpr_count"], kernels["k_shade"][".vgpr_count"]
    total = 6 * _allocated(wide) + _allocated(shade)
    assert total <= 512, f"6 x {_allocated(wide)} (k_trace_pw_wide: {wide}) + {_allocated(shade)} (k_shade: {shade}) = {total} VGPRs"


@pytest.mark.parametrize("name", [WIDE, "k_shade"])
def test_no_spill_and_no_scratch(kernels, name):
    k = kernels[name]
    assert k[".vgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs spilled"
    assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"


def test_shade_kernel_sgprs(kernels):
    assert kernels["k_shade"][".sgpr_count"] <= 112, f"k_shade: {kernels['k_shade']['.sgpr_count']} SGPRs"
