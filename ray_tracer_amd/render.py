"""Command-line driver: the place of the reference's `main.cpp` + ImGui panels.

    python -m ray_tracer_amd.render --scene cornell --width 1728 --height 1117 \
        --single-render --sample-limit 100 --out cornell.png

Every tunable of the reference's "Ray Tracer Info", "Camera Info" and
"Environment" panels (src/vk_engine.cpp:1503-1534) is a flag with the
reference's default (src/vk_engine.h:145-171,325). The frame loop follows
draw() (src/vk_engine.cpp:1774-1815): dispatches run while
totalSamples < sampleLimit; a single render is one dispatch of sampleLimit
samples per pixel, otherwise each dispatch adds raysPerPixel samples and, when
progressive, is blended into the fp32 frame with weight 1/(frame+1).

Two deliberate deviations from draw(), both because this is a command that has
to end and the reference is a window that does not: (1) with singleRender off
the reference resets totalSamples to 0 after every frame
(src/vk_engine.cpp:1813-1814), so sampleLimit never stops it; here
totalSamples accumulates and the loop ends at sampleLimit. (2) With neither
--progressive nor --single-render every dispatch would be the identical
frameCount-0 frame (the reference re-renders it until the window closes); here
exactly one such frame is rendered.

Several GPUs of one node: launch one process per GPU,

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
        -m ray_tracer_amd.render --scene sponza --single-render --sample-limit 1024 --out sponza.png

rank r renders rows r, r+N, ... of the frame (the same pixels, bit for bit, as a
single process), and one RCCL gather at the end brings the strips to rank 0,
which writes the file.
"""
import argparse
import os
import sys
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before the first HIP call: the renderer's three streams beside torch's and RCCL's (rt_amd.h, "lane_grid_pct")

from . import _capi, engine, scenes  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m ray_tracer_amd.render", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell", choices=sorted(scenes.CONFIGS) + ["obj"])
    ap.add_argument("--obj", help="with --scene obj: an OBJ file placed in the default Cornell box")
    ap.add_argument("--obj-material", type=int, default=0, help="0 white 1 red 2 green 3 light 4 mirror 5 dielectric")
    ap.add_argument("--obj-scale", type=float, default=0.7)
    ap.add_argument("--obj-position", type=float, nargs=3, default=(0.0, 0.53, 0.0))
    ap.add_argument("--obj-rotation", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--obj-albedo-map", help="with --scene obj: an image bound as the albedo texture of the OBJ's materials "
                                             "(what an MTL's map_Kd line does; dread.mtl has none, the author bound dread_alb.png by hand)")
    ap.add_argument("--textures", action="store_true",
                    help="sample the maps the scene's MTL files name (and --obj-albedo-map). Off by default: the reference snapshot uploads "
                         "textures and never samples them (raytrace.comp declares TextureBuffer / TextureSampler and reads neither), so the "
                         "untextured image is the one that matches its shader; the sampling semantics are this build's declaration "
                         "(DESIGN.md 3a, parity unpinned)")
    ap.add_argument("--width", type=int, default=1728)
    ap.add_argument("--height", type=int, default=1117)
    ap.add_argument("--device", type=int, default=0, help="GPU of a single-process run (one process per GPU uses LOCAL_RANK)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="several processes: nccl (= RCCL, one GPU per rank); gloo lets all ranks share --device (rehearsal on one GPU)")
    ap.add_argument("--out", help="PNG (8-bit sRGB) or .npy (fp32 RGBA) output file")
    ap.add_argument("--aov-out", metavar="FILE.npz",
                    help="also write the first-hit planes of the camera rays (Renderer.render_aovs: depth, normal, position, albedo, "
                         "ray_dir, object, triangle, material, hit, sphere, front_face) to this .npz")
    ap.add_argument("--denoise", action="store_true",
                    help="write the frame through the edge-aware a-trous denoiser (Renderer.denoise, defaults; DESIGN.md, "
                         "\"Denoising\") to --out; it runs the first-hit AOV pass itself unless --aov-out did")
    ap.add_argument("--guide-bounces", type=int, default=0, metavar="N",
                    help="with --denoise: guide the denoiser by the first surface that is no mirror along up to N reflections (0..8) of "
                         "each camera ray, so that reflections keep their edges (Renderer.render_guides; DESIGN.md, \"Mirror-following "
                         "guide planes\"); 0: by the first hit")
    ap.add_argument("--temporal-frames", type=int, default=0, metavar="N",
                    help="render N non-progressive frames of --rays-per-pixel samples with consecutive frameCounts and one fixed camera, "
                         "accumulate them through the temporal pass (Renderer.temporal_accumulate, defaults; DESIGN.md, \"Temporal "
                         "accumulation\") and write the result, through --denoise afterwards if given. One process only: the pass needs "
                         "the whole frame on one GPU")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TAU",
                    help="with --temporal-frames: frame 0 is uniform, every later frame gets a sample count per pixel from the moments "
                         "so far (Renderer.build_sample_map with target relative error TAU, base --rays-per-pixel, 1 .. 4 x base; "
                         "Renderer.render_sampled; DESIGN.md, \"Per-pixel sample counts\"); prints the map's statistics per frame")
    # Ray Tracer Info panel
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--frames-in-flight", type=int, default=1,
                    help="progressive accumulation: frames handed to the GPU at once (rt_render_frames: the same image as one "
                         "dispatch per frame, sooner — more paths per dispatch; 1 = the reference's frame loop)")
    ap.add_argument("--single-render", action="store_true")
    ap.add_argument("--debug", type=int, default=-1, choices=[-1, 0, 1, 2])
    ap.add_argument("--rays-per-pixel", type=int, default=1)
    ap.add_argument("--bounce-limit", type=int, default=8)
    ap.add_argument("--triangle-cap", type=int, default=50)
    ap.add_argument("--box-cap", type=int, default=200)
    ap.add_argument("--sample-limit", type=int, default=10)
    # Camera Info panel
    ap.add_argument("--fov", type=float, default=None)
    ap.add_argument("--camera-angles", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--camera-position", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    # Environment panel
    ap.add_argument("--environment", action="store_true", help="environment lighting on (lightDir.w = 1)")
    ap.add_argument("--sun-direction", type=float, nargs=3, default=None)
    ap.add_argument("--sun-focus", type=float, default=None)
    ap.add_argument("--sun-intensity", type=float, default=None)
    ap.add_argument("--bake-object", type=int, default=None, metavar="I",
                    help="instead of rendering: the lightmap of object I over its uv layout (rt_bake_lightmap: --rays-per-pixel samples per texel, "
                         "--bounce-limit bounces, the environment options' sky), written to --bake-out")
    ap.add_argument("--bake-size", type=int, nargs=2, default=(256, 256), metavar=("W", "H"))
    ap.add_argument("--bake-dilate", type=int, default=2, metavar="N", help="gutter passes around the charts")
    ap.add_argument("--bake-out", metavar="FILE.npy", help="with --bake-object: the (H, W, 4) fp32 map; FILE.fill.npy gets the (H, W) uint8 fill plane")
    return ap


def make_scene(args):
    if args.scene == "obj":
        if not args.obj:
            raise SystemExit("--scene obj needs --obj FILE")
        s = engine.Scene()
        s.prepare_storage_buffers()
        n0 = s.counts()["materials"]
        s.read_obj(args.obj, engine.placement(position=args.obj_position, scale=args.obj_scale, rotation=args.obj_rotation, samplerIndex=1), args.obj_material)
        if args.obj_albedo_map:
            slot = s.add_texture(args.obj_albedo_map)
            for mi in range(n0, s.counts()["materials"]) or [args.obj_material]:
                m = s.material(mi)
                m.albedoIndex = slot
                s.set_material(mi, m)
        return s, args.obj
    return scenes.CONFIGS[args.scene]()


def make_constants(args):
    W, H = args.width, args.height
    kw = dict(progressive=int(args.progressive), singleRender=int(args.single_render), debug=args.debug,
              raysPerPixel=args.rays_per_pixel, bounceLimit=args.bounce_limit, triangleCap=args.triangle_cap,
              boxCap=args.box_cap, sampleLimit=args.sample_limit)
    cam = scenes.sponza_camera if args.scene.startswith("sponza") else engine.push_constants
    if args.fov is not None:
        kw["fov"] = args.fov
    if args.camera_angles is not None:
        kw["cameraAngles"] = args.camera_angles
    if args.camera_position is not None:
        kw["pos"] = args.camera_position
    if args.environment:
        kw["environmentOn"] = True
    pc = cam(W, H, **kw)
    if args.sun_direction is not None:
        d = np.asarray(args.sun_direction, np.float32)
        pc.environment.lightDir[0:3] = [float(x) for x in d]
    if args.sun_focus is not None:
        pc.environment.horizonColor[3] = args.sun_focus
    if args.sun_intensity is not None:
        pc.environment.zenithColor[3] = args.sun_intensity
    return pc


def srgb8(img):
    """Display encoding of the fp32 frame, the one rt_read_rgba8_srgb applies."""
    v = np.clip(np.nan_to_num(img, nan=0.0), 0.0, 1.0)
    rgb = np.where(v[..., :3] <= 0.0031308, 12.92 * v[..., :3], 1.055 * np.power(v[..., :3], 1.0 / 2.4) - 0.055)
    return (np.concatenate([rgb, v[..., 3:]], axis=-1) * 255.0 + 0.5).astype(np.uint8)


def gather_planes(planes, height, world, rank, on):
    """Each rank's rows of the AOV planes -> the whole image's on rank 0 (None elsewhere), through tiling.gather_frame. The
    planes travel as int32 (uint32 ids) and uint8 (flags) tensors, which every backend gathers."""
    import torch
    from . import tiling
    out = {}
    for k, a in planes.items():
        wire = a.view(np.int32) if a.dtype == np.uint32 else a.view(np.uint8) if a.dtype == np.bool_ else a
        strip = torch.from_numpy(np.ascontiguousarray(wire)).to(on)
        frame = torch.zeros((height,) + tuple(strip.shape[1:]), dtype=strip.dtype, device=on) if rank == 0 else None
        tiling.gather_frame(strip, frame, height, world, rank)
        if rank == 0:
            out[k] = frame.cpu().numpy().view(a.dtype)
    return out if rank == 0 else None


def main(argv=None):
    args = build_parser().parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = args.device
    if args.temporal_frames < 0:
        raise SystemExit("--temporal-frames must be >= 0")
    if not 0 <= args.guide_bounces <= 8:
        raise SystemExit("--guide-bounces must be 0..8")
    if args.guide_bounces and not args.denoise:
        raise SystemExit("--guide-bounces guides the denoiser: it needs --denoise")
    if args.adaptive is not None and not args.temporal_frames:
        raise SystemExit("--adaptive takes its sample counts from the temporal pass: it needs --temporal-frames")
    if args.adaptive is not None and not args.adaptive > 0:
        raise SystemExit("--adaptive must be > 0")
    if args.bake_object is not None and (world > 1 or not args.bake_out or not args.bake_out.endswith(".npy")):
        raise SystemExit("--bake-object is a single-process job and needs --bake-out FILE.npy")
    if args.temporal_frames and world > 1:   # before any rank waits for another
        raise SystemExit(f"--temporal-frames needs the whole frame on one GPU: launched on {world} ranks, run it as a single process")
    if world > 1:
        import torch
        import torch.distributed as dist
        from . import tiling
        if args.backend == "nccl":
            tiling.prepare_rccl_env()
            device = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(device)
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")
    scene, label = make_scene(args)
    pc = make_constants(args)
    r = engine.Renderer(device)
    r.upload_scene(scene)
    paths = scene.texture_paths()
    textured = False
    if args.textures and paths and all(os.path.exists(p) for p in paths):   # the MTL files' maps (src/vk_engine.cpp:1155); absent files: untextured
        r.upload_textures(engine.load_textures(scene))
        textured = True
    elif paths and rank == 0:
        print(f"{len(paths)} texture map(s) named by the scene are not sampled (the reference's shader samples none; --textures applies this build's declared semantics)")
    if args.bake_object is not None:
        p = _capi.RtIrradianceParams(max(args.rays_per_pixel, 1), args.bounce_limit, 0, 0, 1e-5)
        bw, bh = args.bake_size
        t0 = time.perf_counter()
        rgba, fill, st = r.bake_lightmap(args.bake_object, bw, bh, params=p, env=pc.environment, dilate=args.bake_dilate)
        print(f"{label}: lightmap of object {args.bake_object}, {bw}x{bh}, {p.samples} samples per texel, {time.perf_counter() - t0:.3f} s, {st}")
        np.save(args.bake_out, rgba)
        np.save(args.bake_out[:-4] + ".fill.npy", fill)
        print("wrote", args.bake_out)
        return 0
    W, H = args.width, args.height
    tile = dict(row0=rank, rowStride=world) if world > 1 else {}
    t0 = time.perf_counter()
    frames = 0
    img = None
    temporal = args.temporal_frames > 0
    if temporal:   # N independent frames of one camera, blended by the temporal pass instead of the progressive framebuffer
        pc.rayTraceParams.progressive, pc.rayTraceParams.singleRender = 0, 0
        aovs = r.render_aovs(pc, W, H)
        base, d_map, spent = args.rays_per_pixel, None, 0
        for k in range(args.temporal_frames):
            pc.frameCount = k
            if d_map is None:
                r.render(pc, W, H, sync=False)
                spent += base * W * H
            else:   # the frame's own count is the cap of the map's
                pc.rayTraceParams.raysPerPixel = 4 * base
                r.render_sampled(pc, W, H, d_map, sync=False)
                pc.rayTraceParams.raysPerPixel = base
            img = r.temporal_accumulate(pc)
            frames += 1
            if args.adaptive is not None and k + 1 < args.temporal_frames:
                d_map = r.build_sample_map(to_host=False, base_samples=base, min_samples=min(1, base), max_samples=4 * base,
                                           target_rel_error=args.adaptive)
                st = r.sample_map_stats()
                spent += st["samples"]
                print(f"frame {k + 1}: sample map {st['samples']} samples over {st['pixels']} pixels ({st['samples'] / max(st['pixels'], 1):.2f} "
                      f"per pixel), {st['unknown']} without a variance yet, {st['aboveMin']} above the minimum, {st['atMax']} at the maximum")
        r.totalSamples = -(-spent // max(W * H, 1)) if args.adaptive is not None else args.temporal_frames * args.rays_per_pixel
        if args.denoise:
            img = r.denoise(img, r.render_guides(pc, W, H, args.guide_bounces) if args.guide_bounces else aovs)
    while not temporal:
        out = r.run_compute(pc, W, H, frames=args.frames_in_flight, **tile)
        if out is None:
            break
        img = out
        frames += 1
        if not args.progressive and not args.single_render:
            break  # every further dispatch would be this very frame again (frameCount does not advance)
    denoise = args.denoise and img is not None and not temporal
    if not temporal:
        aovs = r.render_aovs(pc, W, H, **tile) if args.aov_out or denoise else None
    on = f"cuda:{device}" if args.backend == "nccl" else "cpu"
    guides = r.render_guides(pc, W, H, args.guide_bounces, **tile) if denoise and args.guide_bounces else None
    if world > 1 and aovs is not None:
        aovs = gather_planes(aovs, H, world, rank, on)
    if world > 1 and guides is not None:
        guides = gather_planes(guides, H, world, rank, on)
    if world > 1 and img is not None:   # strips -> frame on rank 0
        strip = torch.from_numpy(img).to(on)
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device=on) if rank == 0 else None
        tiling.gather_frame(strip, frame, H, world, rank)
        img = frame.cpu().numpy() if rank == 0 else None
    if denoise and world == 1 and guides is None:
        img = r.denoise()   # the context's own frame and planes
    elif denoise and rank == 0:
        img = r.denoise(img, aovs if guides is None else guides)   # the gathered frame and planes, or the guide planes
    dt = time.perf_counter() - t0
    c = r.counters()
    if world > 1:
        tot = torch.tensor([float(c["raysReference"]), float(c["raysTraced"])], dtype=torch.float64,
                           device=f"cuda:{device}" if args.backend == "nccl" else "cpu")
        dist.all_reduce(tot)
        c = {"raysReference": float(tot[0]), "raysTraced": float(tot[1])}
    if rank == 0:
        print(f"{label}{' [textures sampled: declared semantics, parity unpinned]' if textured else ''}: {W}x{H}, {r.totalSamples} spp in {frames} dispatch(es)" + (f" on {world} GPUs" if world > 1 else "") +
              f", {dt:.3f} s, {c['raysReference'] / dt / 1e6:.0f} Mrays/s (reference semantics), {c['raysTraced'] / dt / 1e6:.0f} M executed rays/s")
        if args.out and img is not None:
            if args.out.endswith(".npy"):
                np.save(args.out, img)
            else:
                from PIL import Image
                Image.fromarray((srgb8(img) if world > 1 or denoise or temporal else r.read_rgba8_srgb())[..., :3]).save(args.out)
            print("wrote", args.out)
        if args.aov_out:
            np.savez(args.aov_out, **aovs)
            print("wrote", args.aov_out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
