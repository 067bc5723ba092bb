"""The budgets of the wide traversal kernel, k_trace_pw_wide<20, 192, 768>, read from the gfx950 code object inside the built
library (tools/code_object.py), as tests/test_register_budget.py reads the other kernels'.

Two work-groups of 768 threads per CU are 24 waves, six per SIMD. That holds only while a wave needs at most 512 / 6 = 85 -> 80
VGPRs (allocated in eights) without scratch, at most 112 SGPRs (a SIMD's 800 hold floor(800 / (ceil(sgpr / 16) * 16 + 16)) waves)
and a work-group at most half of a CU's 160 KiB of LDS. A compiler or a source change that takes one of them away costs the sixth
wave, or the second work-group, silently: it shows here, on the CPU."""
import os
import re

import pytest

from util import code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wide(built):
    found = {n: k for n, k in code_object().kernels(built.LIB).items() if re.match(r"void k_trace_pw_wide<", n)}
    assert list(found) == ["void k_trace_pw_wide<20, 192, 768>"], f"the wide kernels in the library: {sorted(found)}"
    return found["void k_trace_pw_wide<20, 192, 768>"]


def test_wide_kernel_fits_six_waves_per_simd(wide):
    assert wide[".vgpr_count"] <= 80, f"{wide['.vgpr_count']} VGPRs"
    assert wide[".vgpr_spill_count"] == 0, f"{wide['.vgpr_spill_count']} VGPRs spilled"
    assert wide[".private_segment_fixed_size"] == 0, f"{wide['.private_segment_fixed_size']} bytes of scratch"
    sgprs = wide[".sgpr_count"]
    assert sgprs <= 112, f"{sgprs} SGPRs"
    assert 800 // ((sgprs + 15) // 16 * 16 + 16) == 6, f"{sgprs} SGPRs admit {800 // ((sgprs + 15) // 16 * 16 + 16)} waves per SIMD"


def test_two_wide_groups_fit_a_cu(wide):
    assert wide[".max_flat_workgroup_size"] == 768
    assert wide[".group_segment_fixed_size"] <= 81920, f"{wide['.group_segment_fixed_size']} bytes of LDS per work-group"
    assert wide[".group_segment_fixed_size"] == 768 * 21 * 4 + 1024 + 192 * 64   # stacks, object metadata, table (launch_plan.h: wide_group_lds)


def test_wide_kernel_keeps_its_packed_slab_test(built):
    """box_intersect_pair is packed by hand: six v_pk_add_f32 and six v_pk_mul_f32 per copy of the interior step."""
    ops = code_object().disassembly(built.LIB)["_Z15k_trace_pw_wideILi20ELi192ELi768EEv8DevScene9PathState11TracePwArgs"]
    packed = sum(op in ("v_pk_add_f32", "v_pk_mul_f32") for op in ops)
    assert packed > 0 and packed % 12 == 0, f"{packed} packed fp32 instructions in the wide kernel"
