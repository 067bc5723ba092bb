"""The kernels of the radiance queries (rt_query_radiance) in the built library's gfx950 code object (tools/code_object.py, as
tests/test_register_budget.py reads it): the shading kernels that restart a sample from the caller's origins keep k_shade's budget
(96 VGPRs: five waves per SIMD; nothing spilled), and the two kernels that make the rays and write the results use no scratch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels(built):
    spec = importlib.util.spec_from_file_location("code_object", os.path.join(ROOT, "tools", "code_object.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.kernels(built.LIB)


def _kernel(kernels, name):
    """The row of the kernel `name` (a row's key keeps the argument list of a kernel whose first argument is not the scene)."""
    rows = [k for n, k in kernels.items() if n == name or n.startswith(name + "(")]
    assert len(rows) == 1, f"{name}: {len(rows)} kernels of that name in the code object"
    return rows[0]


@pytest.mark.parametrize("name", ["k_shade_rays", "k_shade_rays_maps"])
def test_shade_rays_kernels_fit_96_registers_without_spills(kernels, name):
    k = _kernel(kernels, name)
    print(name, {f: v for f, v in k.items() if f != ".name"})
    assert k[".vgpr_count"] <= 96, f"{name}: {k['.vgpr_count']} VGPRs"
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, f"{name}: spills {k['.vgpr_spill_count']} VGPRs, {k['.sgpr_spill_count']} SGPRs"


@pytest.mark.parametrize("name", ["k_radiance_rays", "k_radiance_resolve"])
def test_ray_and_resolve_kernels_use_no_scratch(kernels, name):
    k = _kernel(kernels, name)
    print(name, {f: v for f, v in k.items() if f != ".name"})
    assert k[".private_segment_fixed_size"] == 0, f"{name}: {k['.private_segment_fixed_size']} bytes of scratch"
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0
