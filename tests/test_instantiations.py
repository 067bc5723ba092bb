"""Every traversal kernel instantiation in the library, launched and compared with the oracle.

The traversal is one device function (trace_wave) compiled into ~80 kernels: k_trace_pw<STACK, OVF, PIX, STATS, CULL, HOT, BLOCKS>,
k_render_fused<STACK, OVF, PIX, CULL> and the one-ray-per-lane k_trace<STACK>. Which one runs follows from the scene (deepest
leaf, placed objects), the dispatch (heat maps) and knobs — so the other parity tests cover whatever their scenes happen to
select. Rounds 2 and 3 met three wrong binaries of heavily spilling k_render_fused instantiations (all others stayed right) under
ROCm 7.2.0's AMDGPU backend; the pass they have in common is si-opt-vgpr-liverange (tools/pass_attribution.sh) and the library is
built with it off (__graft_entry__.HIPFLAGS; tools/miscompile_repro.sh). This test is the guard for that decision — on the
library built with si-opt-vgpr-liverange left on it fails —: it reads the list of instantiations out of the built library (host stubs in its symbol table), forces
each of them through scenes of the right BVH depth, with and without placed objects, heat maps, phase statistics, the three
top-level-table modes and the LDS stack caps, asks the library which kernel it launched (rt_last_kernel), compares pixels and
counters with the oracle bit for bit, and fails if any instantiation in the binary was not reached."""
import numpy as np
import pytest

from oracle import pyoracle
from ray_tracer_amd import engine
from instantiation_scenes import _same, build_scene, skewed, soup
from util import kernel_instantiations

pytestmark = pytest.mark.gpu

# the builder's depth cap is 64 and a mesh that deep cannot be made small; k_trace<64> is the A/B baseline kernel's last size
UNREACHED_ON_PURPOSE = {"k_trace<64>"}


def library_instantiations():
    return kernel_instantiations("k_(?:trace_pw_alpha|trace_pw|render_fused|trace)")


# (name, mesh, depth bucket the mesh is made for)
MESHES = [("d4", lambda: soup(24, 1, 0.08), (1, 8)), ("d13", lambda: soup(1200, 2, 0.04), (9, 16)), ("d17", lambda: soup(40000, 3), (17, 20)),
          ("d22", lambda: soup(300000, 4, 0.01), (21, 24)), ("d28", lambda: skewed(100000, 4, 5), (25, 32)), ("d37", lambda: skewed(100000, 8, 6), (33, 48))]


def test_every_instantiation_in_the_library_against_the_oracle(renderer):
    in_library = library_instantiations()
    assert len(in_library) > 60, "could not read the kernel instantiations out of the library's symbol table"
    reached = {}
    W, H = 64, 48
    knobs = ("pipeline", "hot_pairs", "lds_stack", "phase_stats", "trace_variant")
    renderer.set_tuning("blocks_per_cu", 0); renderer.set_tuning("pixel_refill", 0)
    try:
        for name, mesh, (lo, hi) in MESHES:
            for placed in (False, True):
                s, depth = build_scene(mesh, placed)
                assert lo <= depth <= hi, f"mesh {name}: BVH depth {depth} left its bucket {lo}..{hi}"
                pcs = {False: engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=4, environmentOn=True),
                       True: engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=4, environmentOn=True, debug=2, boxCap=400, triangleCap=60)}
                refs = {dbg: pyoracle.render(s, pc, W, H) for dbg, pc in pcs.items()}
                renderer.upload_scene(s)

                def run(tag, dbg=False, **tune):
                    for k, v in tune.items():
                        renderer.set_tuning(k, v)
                    renderer.reset_counters()
                    img = renderer.render(pcs[dbg], W, H)
                    kern = renderer.last_kernel()
                    _same(img, renderer.counters(), *refs[dbg], what=f"{name} placed={placed} {tag} -> {kern}")
                    reached.setdefault(kern, f"{name} placed={placed} {tag}")
                    for k in tune:
                        renderer.set_tuning(k, {"pipeline": -1, "hot_pairs": 2, "lds_stack": 24, "phase_stats": 0, "trace_variant": 1}[k])

                # the fused kernel once more on a tile big enough that a wave works through several blocks and replaces finished pixels
                # while its other lanes are in flight (one work-group per CU, pixels replaced at 8 free lanes): round 3's wrong binary
                # of k_render_fused<24, true, false, false> was right on one block per wave and wrong from the second hand-out on
                if True:
                    Wb, Hb = 512, 384
                    pcb = engine.push_constants(Wb, Hb, singleRender=1, sampleLimit=2, bounceLimit=4, environmentOn=True)
                    refb = pyoracle.render(s, pcb, Wb, Hb, threads=pyoracle.effective_cpus())
                    for k, v in (("pipeline", 1), ("blocks_per_cu", 1), ("pixel_refill", 8)):
                        renderer.set_tuning(k, v)
                    renderer.reset_counters()
                    imgb = renderer.render(pcb, Wb, Hb)
                    _same(imgb, renderer.counters(), *refb, what=f"{name} placed={placed} fused, several blocks per wave -> {renderer.last_kernel()}")
                    for k, v in (("pipeline", -1), ("blocks_per_cu", 0), ("pixel_refill", 0)):
                        renderer.set_tuning(k, v)

                caps = [24] + ([16] if depth > 16 else []) + ([8] if depth > 8 else [])
                for cap in caps:
                    for hot in (0, 1, 2):
                        run(f"multi-kernel hot_pairs={hot} lds_stack={cap}", pipeline=0, hot_pairs=hot, lds_stack=cap)
                    run(f"multi-kernel heat map lds_stack={cap}", dbg=True, pipeline=0, lds_stack=cap)
                    run(f"multi-kernel phase_stats lds_stack={cap}", pipeline=0, phase_stats=1, lds_stack=cap)
                    run(f"fused lds_stack={cap}", pipeline=1, lds_stack=cap)
                    run(f"fused heat map lds_stack={cap}", dbg=True, pipeline=1, lds_stack=cap)
                run("one ray per lane", pipeline=0, trace_variant=0)
                if name == "d13":
                    # k_trace_pw_alpha<PIX>, the traversal of scenes that bind an alpha map (tests/test_textures.py has its real cases):
                    # the meshes here carry no uvs, so every hit looks up the map's one texel at (0.5, 0.5) — opaque: the same frame
                    m = s.material(s.grey); m.alphaIndex = 0; s.set_material(s.grey, m)
                    opaque = [np.full((2, 2, 4), 255, np.uint8)]
                    renderer.upload_scene(s); renderer.upload_textures(opaque); pyoracle.set_textures(opaque)
                    try:
                        for dbg in (False, True):
                            refs[dbg] = pyoracle.render(s, pcs[dbg], W, H)
                            run("alpha map", dbg=dbg)
                    finally:
                        renderer.upload_textures([]); pyoracle.set_textures([])
    finally:
        for k in knobs:
            renderer.set_tuning(k, {"pipeline": -1, "hot_pairs": 2, "lds_stack": 24, "phase_stats": 0, "trace_variant": 1}[k])
    unknown = set(reached) - in_library
    assert not unknown, f"rt_last_kernel named kernels the library's symbol table does not hold: {sorted(unknown)}"
    missed = in_library - set(reached) - UNREACHED_ON_PURPOSE
    assert not missed, f"{len(missed)} instantiations in the library were never launched: {sorted(missed)}"
