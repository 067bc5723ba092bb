"""The register budget the device build rests on since the SLP vectorizer is off for it (__graft_entry__.HIPFLAGS), read from the
gfx950 code object inside the built library (tools/code_object.py; tools/kernel_info.py reads the same figures from a listing).

With the vectorizer packing the fp32 algebra into v_pk_* instructions the traversal kernels stood at 78-84 VGPRs with up to 8 of
them spilled, k_shade at 106, and the fused kernels spilled 38-58. Without it: every k_trace_pw instantiation that carries no
phase statistics fits the 72 registers that leave room for a k_shade wave beside five traversal waves per SIMD, k_shade fits 96
(five waves per SIMD), and the fused kernels spill a third of what they did. profiles/r05_registers.txt has both columns for all
kernels; the fused kernels' limits below are its parent column. A compiler or a source change that takes the registers back
shows here, on the CPU, before it shows as a slower frame."""
import os
import re

import pytest

from util import code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_KERNEL = "_Z10k_trace_pwILi20ELb0ELb0ELb0ELb0ELi144ELi5EEv8DevScene9PathState11TracePwArgs"   # k_trace_pw<20, 0, 0, 0, 0, 144, 5>


@pytest.fixture(scope="module")
def kernels(built):
    return code_object().kernels(built.LIB)


def _parent_column():
    """{kernel: (VGPRs, SGPRs, scratch bytes, SGPR spills, VGPR spills)} of the parent build, from profiles/r05_registers.txt."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "r05_registers.txt")):
        m = re.match(r"^(.*?)\((\d+), (\d+), (\d+), (\d+), (\d+)\) -> \(", line)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    return rows


def test_traversal_kernels_fit_72_registers_without_spills(kernels):
    seen = 0
    for name, k in kernels.items():
        m = re.match(r"void k_trace_pw<(\d+), (\w+), (\w+), (\w+), (\w+), (\d+), (\d+)>$", name)   # <STACK, OVF, PIX, STATS, CULL, HOT, BLOCKS>
        if not m or m.group(4) == "true":
            continue
        seen += 1
        assert k[".vgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs spilled"
        assert k[".vgpr_count"] <= 72, f"{name}: {k['.vgpr_count']} VGPRs"
    assert seen >= 30, f"only {seen} k_trace_pw instantiations without phase statistics found"


def test_shade_kernels_fit_96_registers_without_spills(kernels):
    for name in ("k_shade", "k_shade_maps"):
        k = kernels[name]
        assert k[".vgpr_spill_count"] == 0, f"{name}: {k['.vgpr_spill_count']} VGPRs spilled"
        assert k[".vgpr_count"] <= 96, f"{name}: {k['.vgpr_count']} VGPRs"


def test_fused_kernels_spill_no_more_than_the_parent_build(kernels):
    parent = _parent_column()
    fused = [n for n in kernels if re.match(r"void k_render_fused<", n)]
    assert len(fused) == 24, fused
    for name in fused:
        assert name in parent, f"{name} is not in profiles/r05_registers.txt"
        assert kernels[name][".vgpr_spill_count"] <= parent[name][4], \
            f"{name}: {kernels[name]['.vgpr_spill_count']} VGPRs spilled, the parent build spilled {parent[name][4]}"


def test_bench_kernel_keeps_its_packed_slab_test(built):
    """box_intersect_pair is packed by hand (ext_vector_type): six v_pk_add_f32 and six v_pk_mul_f32 per copy of the interior step.
    The vectorizer switch must not take them away."""
    ops = code_object().disassembly(built.LIB)[BENCH_KERNEL]
    packed = sum(op in ("v_pk_add_f32", "v_pk_mul_f32") for op in ops)
    assert packed > 0 and packed % 12 == 0, f"{packed} packed fp32 instructions in the bench kernel"
