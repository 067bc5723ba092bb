// launch_plan.cpp — the launch policy (launch_plan.h). Host only: no HIP runtime call, no context, no kernel.
#include "launch_plan.h"

#include <algorithm>

#include "scene_layout.h"   // RT_MAP_*

// ---------------------------------------------------------------- tuning
TuningChange set_tuning(Tuning& t, const std::string& k, int value) {
    auto refuse = [](const std::string& m) { return TuningChange{m, false}; };
    if (k == "pipeline") { if (value < -1 || value > 1) return refuse("pipeline: -1 (auto), 0 or 1"); t.pipeline = value; }
    else if (k == "probe") { t.probe = value ? 1 : 0; }
    else if (k == "frames_max_mslots") { if (value < 1 || value > 1000) return refuse("frames_max_mslots: 1..1000 (millions of paths per multi-frame dispatch)"); t.framesMaxSlots = (uint64_t)value << 20; }
    else if (k == "radiance_max_kslots") { if (value < 0 || value > (1 << 20)) return refuse("radiance_max_kslots: 1..1048576 (x 1024 rays per piece of a radiance query), 0 = as frames_max_mslots"); t.radianceMaxSlots = (uint64_t)value << 10; }
    else if (k == "frames_per_launch") { if (value < 0) return refuse("frames_per_launch >= 0"); t.framesPerLaunch = value; }
    else if (k == "camera_reuse") { t.cameraReuse = value ? 1 : 0; }
    else if (k == "light_queries") { t.lightQueries = value ? 1 : 0; return TuningChange{"", true}; }
    else if (k == "fused_below_box_tests") { if (value < 0) return refuse("fused_below_box_tests >= 0"); t.fusedBelowBoxTests = (uint32_t)value; }
    else if (k == "fused_below_pixels") { if (value < 0) return refuse("fused_below_pixels >= 0"); t.fusedBelowPixels = (uint32_t)value; }
    else if (k == "trace_variant") { if (value < 0 || value > 1) return refuse("trace_variant: 0 or 1"); t.traceVariant = value; }
    else if (k == "refill") { if (value < 1 || value > 64) return refuse("refill: 1..64"); t.refill = value; t.refillMk = value; t.refillMkSet = true; }
    else if (k == "hot_pairs") { if (value < 0 || value > 2) return refuse("hot_pairs: 0, 1 (six work-groups per CU) or 2 (five)"); t.hotPairs = value; }
    else if (k == "mk_refill") { if (value < 1 || value > 64) return refuse("mk_refill: 1..64"); t.refillMk = value; t.refillMkSet = true; }
    else if (k == "lds_stack") { if (value != 8 && value != 16 && value != 24) return refuse("lds_stack: 8, 16 or 24"); t.ldsStackCap = value; }
    else if (k == "fast_lanes") { if (value < 0 || value > 65) return refuse("fast_lanes: 1..65 (0: back to the defaults)"); t.fastLanesSet = value != 0; t.fastLanes = value ? value : 32; }
    else if (k == "chunk") { if (value < 1 || value > 4096) return refuse("chunk: 1..4096"); t.chunk = value; }
    else if (k == "w_setup") { if (value < 1 || value > 512) return refuse("w_setup: 1..512"); t.wSetup = value; t.wSetupFused = value; t.wSetupSet = true; }
    else if (k == "w_leaf") { if (value < 1 || value > 512) return refuse("w_leaf: 1..512"); t.wLeaf = value; t.wLeafFused = value; t.wLeafSet = true; }
    else if (k == "mk_w_setup") { if (value < 1 || value > 512) return refuse("mk_w_setup: 1..512"); t.wSetup = value; t.wSetupSet = true; }
    else if (k == "mk_w_leaf") { if (value < 1 || value > 512) return refuse("mk_w_leaf: 1..512"); t.wLeaf = value; }
    else if (k == "tile_slots") { t.tileSlots = value != 0; }
    else if (k == "mask_identity") { t.maskIdentity = value != 0; }
    else if (k == "fast_share") { if (value < 0 || value > 16) return refuse("fast_share: 0..16"); t.fastShare = value; }
    else if (k == "scatter") { if (value != -1 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 16) return refuse("scatter: -1 (auto), 0, 1, 2, 4, 8 or 16"); t.scatter = value; }
    else if (k == "fused_maps") { if (value < 0 || value > 1) return refuse("fused_maps: 0 (map scenes take the multi-kernel pipeline) or 1 (they choose as usual)"); t.fusedMaps = value; }
    else if (k == "tri_plane") { if (value < 0 || value > 1) return refuse("tri_plane: 0 (the triangle queries descend by boxes only) or 1 (and by the query's plane)"); t.triPlane = value; }
    else if (k == "pixel_refill") { if (value < 0 || value > (int)RT_WAVE) return refuse("pixel_refill must be 0 (by ray length) .. 64"); t.pixelRefill = value; }
    else if (k == "batch_pixels") { if (value < 0 || value > (int)RT_WAVE) return refuse("batch_pixels must be 0 (auto) .. 64"); t.batchPixels = value; }
    else if (k == "batch_fixed") { if (value < 0 || value > 4096) return refuse("batch_fixed out of range"); t.batchFixed = value; }
    else if (k == "phase_stats") { if (value < 0) return refuse("phase_stats >= 0"); t.phaseStats = value; }
    else if (k == "object_tree_min") { if (value < 0) return refuse("object_tree_min >= 0"); t.objTreeMin = value; }
    else if (k == "lanes") { if (value < 0 || value > RT_MAX_LANES) return refuse("lanes: 1..4 (parts of a multi-kernel dispatch, each on its own stream), 0 = automatic"); t.lanes = value ? value : 3; t.lanesSet = value != 0; }
    else if (k == "lane_grid_pct") { if (value != 0 && (value < 10 || value > 100)) return refuse("lane_grid_pct: 0 (by size) or 10..100"); t.laneGridPct = value; }
    else if (k == "lanes_min_kslots") { if (value < 0) return refuse("lanes_min_kslots >= 0"); t.lanesMinSlots = (uint32_t)value << 10; }
    else if (k == "wide_min_kslots") { if (value < 0) return refuse("wide_min_kslots >= 0"); t.wideMinSlots = (uint64_t)value << 10; }
    else if (k == "wide_grid_pct") { if (value != 0 && (value < 10 || value > 100)) return refuse("wide_grid_pct: 0 (the parts' share) or 10..100"); t.wideGridPct = value; }
    else if (k == "blocks_per_cu") { if (value < 0 || value > 8) return refuse("blocks_per_cu: 0..8"); t.blocksPerCU = value; }
    else return refuse("unknown tuning key " + k);
    return TuningChange{};
}

// ---------------------------------------------------------------- measured
void fold_snapshot(Measured& m, const RayCounters& snap) {
    const unsigned long long box = snap.boxTests - snap.skippedBoxTests, rays = snap.raysTraced;  // executed tests: what a ray costs the GPU
    if (rays > m.snapRays && box >= m.snapBox && rays - m.snapRays > 100000ull)
        m.boxPerRay = (double)(box - m.snapBox) / (double)(rays - m.snapRays);
    const unsigned long long seg = snap.segments, paths = snap.paths;
    if (paths > m.snapPaths && seg >= m.snapSeg && paths - m.snapPaths > 100000ull) m.segPerPath = (double)(seg - m.snapSeg) / (double)(paths - m.snapPaths);
    m.snapBox = box;
    m.snapRays = rays;
    m.snapSeg = seg;
    m.snapPaths = paths;
}

void fold_probe(Measured& m, const RayCounters& before, const RayCounters& after) {
    if (after.raysTraced > before.raysTraced + 1000ull)
        m.boxPerRay = (double)((after.boxTests - after.skippedBoxTests) - (before.boxTests - before.skippedBoxTests)) / (double)(after.raysTraced - before.raysTraced);
}

// ---------------------------------------------------------------- pipeline
// Both pipelines give the same bits; which one is faster depends on how much a wave has to do per pixel. Small tiles
// and scenes with short rays (few box tests per ray, measured on this context's earlier dispatches) go to the fused one.
// 0 = multi-kernel, 1 = fused.
int choose_pipeline(const Tuning& t, const Measured& m, const SceneFacts& sc, const DispatchFacts& d) {
    const double boxPerRay = m.boxPerRay;
    const uint32_t nSlots = (uint32_t)dispatch_slots(d.nPixels, d.nFrames);
    const bool shortRays = boxPerRay >= 0.0 && boxPerRay < (double)t.fusedBelowBoxTests;
    // the longer the rays, the earlier the global queue of the multi-kernel pipeline pays — and with the dispatch in overlapping
    // parts earlier than it used to (tools/size_sweep.py, one 1080p frame = 2.07 M paths, fused / multi-kernel in parts: Sponza,
    // 153 executed box tests per ray, 113.8 / 103.4 ms; Sponza + 16 dragons 167.2 / 162.5; the klein bottle x 8, 84 tests,
    // 70.2 / 76.6; half a frame, 1.04 M paths: 61.5 / 66.3, 91.9 / 106.8, 41.5 / 57.4): 4 M paths up to 90 tests per ray, falling
    // to 1.5 M at 150
    double sizeLimit = (double)t.fusedBelowPixels;
    if (boxPerRay > 90.0) sizeLimit = std::max(0.375 * sizeLimit, sizeLimit - (boxPerRay - 90.0) * (0.625 / 60.0) * sizeLimit);
    // (the paths of all the frames of the dispatch count: four frames of a quarter of a 4K frame are a 4K frame's worth)
    // Short rays keep the fused pipeline at any size — unless the traversal misses the caches: a scene whose hot data (child pairs
    // and triangle positions) exceeds one XCD's 4 MB of L2 is bound by latency even with few tests per ray, and from 10 M paths the
    // multi-kernel pipeline's extra resident waves and overlapping parts win there too (Cornell + bunny, 33 box tests per ray, ten
    // 1080p frames: 36.1 against 38.0 ms per frame; + dragon 36.3 against 40.1; level between four and six frames:
    // tools/frames_sweep.py), while small scenes (bobadog, the 45-object scene)
    // and scenes of very short rays (fewer than 25 executed tests: 232 k loose triangles on a floor) stay fused (tools/heuristics_table.py)
    const bool bigScene = (uint64_t)sc.nodeCount * 32u + (uint64_t)sc.triCount * 48u > (4ull << 20);
    const bool shortButMissing = shortRays && bigScene && boxPerRay >= 25.0 && nSlots >= (10u << 20);
    const int chosen = d.pipeline >= 0 ? d.pipeline : (((double)nSlots < sizeLimit || (shortRays && !shortButMissing)) ? 1 : 0);
    // a scene that binds a metalness, alpha or bump map: the multi-kernel pipeline's kernels that read them (k_shade_maps,
    // k_trace_pw_alpha), whatever "pipeline" asks for — unless "fused_maps" lets it choose as usual (k_render_fused_maps)
    return (sc.mapFlags && !t.fusedMaps) ? 0 : chosen;
}

// ---------------------------------------------------------------- the ray-cost probe
// The launch parameters of both pipelines follow the scene's measured box tests per ray, which the first dispatch of a
// scene does not have — and a single-render job (the reference's singleRender mode: all samples in one dispatch) is
// nothing but a first dispatch. Before a big one, eight rows of the same tile are rendered once with one sample per
// pixel into a scratch image and the counters put back: a few ms, no trace in anything the caller can read.
bool probe_first(const Tuning& t, const Measured& m, const SceneFacts& sc, const DispatchFacts& d) {
    return m.boxPerRay < 0.0 && t.probe && !d.probe && !sc.mapFlags && (uint64_t)d.nPixels * d.samples >= 8000000ull && d.debug < 0;
}
TileRows probe_rows(const TileRows& tile) {
    const uint32_t rows = std::min(tile.nRows, 8u), skip = tile.nRows / rows;
    return TileRows{tile.row0 + (skip / 2u) * tile.rowStride, tile.rowStride * skip, rows};
}

// ---------------------------------------------------------------- parts of a multi-kernel dispatch
// The parts a multi-kernel dispatch is wanted in (the device may grant fewer: one stream per part)
int choose_parts(const Tuning& t, const Measured& m, const SceneFacts& sc, const DispatchFacts& d) {
    const uint32_t nSlots = (uint32_t)dispatch_slots(d.nPixels, d.nFrames);
    int nLanes = (d.samples > 0 && nSlots >= t.lanesMinSlots) ? std::max(1, std::min(t.lanes, (int)RT_MAX_LANES)) : 1;
    if (d.phaseStats) nLanes = 1;  // the diagnostic kernel's statistics are per launch
    // One scene shape loses by it (tools/lanes_table.py): long rays that walk into many placed objects (C5: sixteen instanced dragons,
    // ~190 executed box tests per ray; 116.1 ms per frame in one part against 121.2 in three at 1080p, 472 against 492 at 4K).
    // Every placed object a ray enters costs a set-up round that reloads the ray from its path state in HBM, so that traversal
    // competes with the other parts' k_shade for HBM instead of complementing it. Such scenes keep one part unless "lanes" was set.
    // (from 8 M paths on: a single 1080p frame of the same scene still gains 7 % from its parts, whose launches are short against their tails)
    if (!t.lanesSet && sc.cull && m.boxPerRay >= 150.0 && nSlots >= (8u << 20)) nLanes = 1;
    return nLanes;
}
// ... and the share of the resident work-groups each part's k_trace_pw launches take
// (small parts — one 1080p frame per dispatch is three parts of 0.69 M paths — run better on 40 % grids: 101.7 -> 99.5 ms per
// frame; the bench's ten frames per dispatch, 6.9 M paths per part, on 50 %: 77.2 against 78.6)
int part_grid_pct(const Tuning& t, int nLanes, uint32_t firstPartSlots) {
    return nLanes > 1 ? (t.laneGridPct > 0 ? t.laneGridPct : (firstPartSlots < 1200000u ? 40 : 50)) : 100;
}
// The slots of a dispatch in nLanes contiguous ranges of whole blocks
PartSlices slice_parts(const Tuning& t, uint32_t nSlots, uint32_t nFrames, int nLanes) {
    PartSlices p{};
    const uint32_t unit = 256u * std::max(1u, nFrames);  // whole blocks of k_shade, whole tile blocks of all their frames
    const uint32_t units = (nSlots + unit - 1) / unit;
    uint32_t at = 0;
    for (int l = 0; l < nLanes; l++) {
        const uint32_t u = units / (uint32_t)nLanes + ((uint32_t)l < units % (uint32_t)nLanes ? 1u : 0u);
        const uint32_t end = std::min(nSlots, at + u * unit);
        p.begin[l] = at; p.n[l] = end - at;
        at = end;
    }
    p.gridPct = part_grid_pct(t, nLanes, p.n[0]);
    return p;
}

// ---------------------------------------------------------------- frames per dispatch (rt_render_frames)
// The frames of one call are one dispatch: their paths share the launch (fused pipeline) or the queues of every round
// (multi-kernel pipeline; the pipeline is picked by the paths of all the frames together, so four frames of a
// quarter of a 4K frame run like a whole 4K frame). Ordinary frames only (no heat maps: those read per-pixel counters at
// resolve time), within the 30-bit slot ids and RT_FRAMES_MAX_SLOTS paths (3.9 GB of path state); more frames than that
// go in several dispatches.
uint32_t frames_per_dispatch(const Tuning& t, uint64_t np, uint32_t nFrames, int debug) {
    uint32_t per = 1;
    if (nFrames > 1u && debug < 0 && np > 0) {
        const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(t.framesMaxSlots, np), (1ull << 30) - 1);
        per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nFrames, cap / frame_slots(np)));
        if (t.framesPerLaunch > 0) per = std::min(per, (uint32_t)t.framesPerLaunch);
    }
    return per;
}

// ---------------------------------------------------------------- the traversal kernel
namespace {
// The traversal kernel's stack for a BVH of depth d and at most `cap` LDS entries per lane; ovf: the deeper entries in the
// overflow buffer. Only the multi-kernel pipeline has a 20-entry kernel.
// (tests/test_instantiations.py makes a scene for each depth bucket of these rows)
struct StackBucket { int stack; bool ovf; };
StackBucket stack_bucket(uint32_t d, uint32_t cap, bool allow20) {
    if (d <= 8) return {8, false};
    if (cap < 16) return {8, true};
    if (d <= 16) return {16, false};
    if (cap < 24) return {16, true};
    if (allow20 && d <= 20) return {20, false};
    if (d <= 24) return {24, false};
    return {24, true};
}
}  // namespace

KernelKey trace_kernel_key(const Tuning& t, const SceneFacts& sc, const DispatchFacts& d) {
    const uint32_t depth = sc.maxLeafDepth;
    const bool pix = d.pixStats || d.perRay;  // per-ray counters are only needed for the pixel heat maps (debug >= 0) and rt_trace_rays
    const bool alpha = sc.mapFlags & RT_MAP_ALPHA;  // a bound alpha map: the one traversal kernel that reads it (any depth, any objects)
    if (alpha) return KernelKey{KernelFamily::trace_pw_alpha, 24, true, pix, false, false, 0, 0};
    if (t.traceVariant == 0)  // one ray per lane, whole stack in LDS
        return KernelKey{KernelFamily::trace, depth <= 8 ? 8 : depth <= 16 ? 16 : depth <= 24 ? 24 : depth <= 32 ? 32 : depth <= 48 ? 48 : 64, false, false, false, false, 0, 0};
    // persistent waves; at most 24 entries in LDS, deeper ones in the overflow buffer
    // BVHs deeper than 24: 16 entries in LDS, the rest in the overflow buffer (the stack only holds far siblings and is rarely
    // that deep), which leaves room for 120 top-level pairs beside six work-groups per CU: C5 at 4K 474 -> 468 ms per step,
    // flattened 471 -> 462, 1080p 117.5 -> 115.6 (Cornell + dragon: level)
    const bool tableWanted = t.hotPairs && sc.hotNodes > 0 && !d.phaseStats && !pix;
    const uint32_t cap = (depth > 24u && t.ldsStackCap >= 24 && tableWanted) ? 16u : (uint32_t)t.ldsStackCap;
    const StackBucket b = stack_bucket(depth, cap, true);
    const int h6 = hot6(b.stack, b.ovf), h5 = hot5(b.stack, b.ovf);
    int hotMode = tableWanted ? t.hotPairs : 0;
    if (hotMode == 1 && h6 == 0) hotMode = 2;   // (a 24-entry stack leaves no room at six work-groups)
    if (hotMode == 2 && h5 == 0) hotMode = h6 ? 1 : 0;   // (overflow-stack instantiations: the table only beside 16-entry stacks)
    // A big dispatch of a scene whose kernel would be <20, .., 144, 5>: work-groups of RT_WIDE_THREADS threads, RT_WIDE_GROUPS per CU. That
    // is the sixth wave per SIMD of hot_pairs 1 and, with two copies of the table per CU instead of five, all RT_WIDE_HOT pairs
    // beside them. Small dispatches keep the 256-thread groups (a grid of few, coarse groups fills the device unevenly).
    if (hotMode == 2 && b.stack == 20 && !b.ovf && !sc.cull && dispatch_slots(d.nPixels, d.nFrames) >= t.wideMinSlots)
        return KernelKey{KernelFamily::trace_pw, 20, false, false, false, false, RT_WIDE_HOT, RT_WIDE_GROUPS, RT_WIDE_THREADS};
    if (hotMode == 1) return KernelKey{KernelFamily::trace_pw, b.stack, b.ovf, false, false, sc.cull, h6, 6};
    if (hotMode == 2) return KernelKey{KernelFamily::trace_pw, b.stack, b.ovf, false, false, sc.cull, h5, 5};
    if (d.phaseStats) return KernelKey{KernelFamily::trace_pw, b.stack, b.ovf, true, true, sc.cull, 0, 6};
    return KernelKey{KernelFamily::trace_pw, b.stack, b.ovf, pix, false, sc.cull, 0, 6};
}

KernelKey fused_kernel_key(const Tuning& t, const SceneFacts& sc, const DispatchFacts& d) {
    if (sc.mapFlags) return KernelKey{KernelFamily::render_fused_maps, 24, true, d.pixStats, false, true, 0, 0};  // one kernel, any depth, any objects: <24, true, *, true>
    const StackBucket b = stack_bucket(sc.maxLeafDepth, (uint32_t)t.ldsStackCap, false);
    return KernelKey{KernelFamily::render_fused, b.stack, b.ovf, d.pixStats, false, sc.cull, 0, 0};
}

// ---------------------------------------------------------------- launch shapes
TraceShape trace_shape(const Tuning& t, const Measured& m, const SceneFacts& sc, const DispatchFacts& d, uint32_t maxRays, uint32_t resident) {
    TraceShape s;
    // a part of a dispatch that runs beside the other parts' launches takes its share of the resident work-groups (DispatchFacts::gridPct)
    // (a work-group per groupThreads rays: 256, or the wide kernel's)
    const uint32_t threads = std::max(d.groupThreads, (uint32_t)RT_WAVE);
    // wide work-groups beside the other parts' launches: their own share (Tuning::wideGridPct), unless lane_grid_pct was set by hand
    const bool wideInParts = threads != RT_BLOCK && d.gridPct < 100 && t.laneGridPct == 0 && t.wideGridPct > 0;
    const uint32_t pct = wideInParts ? (uint32_t)t.wideGridPct : (uint32_t)d.gridPct;
    s.blocks = std::min((uint32_t)(((uint64_t)maxRays + threads - 1) / threads), std::max(1u, (uint32_t)((uint64_t)resident * pct / 100u)));
    const bool times = d.phaseStats == 1 || (d.phaseStats >= 2 && d.counted && d.launches == (uint64_t)(d.phaseStats - 2));  // 1: the last launch's waves; 2 + k: launch k's (after rt_reset_counters)
    s.waveTimes = !(sc.mapFlags & RT_MAP_ALPHA) && times;
    // Long rays (the measure the pipeline choice uses) want new rays sooner and their set-up served later: idle lanes re-armed at 12
    // instead of 16, set-up steps voted in at weight 32 instead of 16 (Sponza 81.0 -> 79.4 ms per step, C5 115.4 -> 114.1;
    // Cornell + bunny / + dragon, short rays: +2.5 / +3.5 % with the same, so they keep 16 / 16). Knobs set by hand win.
    const bool longRays = m.boxPerRay >= (double)t.fusedBelowBoxTests;
    s.refillMk = t.refillMkSet ? (uint32_t)t.refillMk : (longRays ? 12u : 16u);
    s.wSetup = t.wSetupSet ? (uint32_t)t.wSetup : (longRays ? 32u : 16u);
    return s;
}

namespace {
// Pixels per wave-private block of k_render_fused. A wave finishes its block's samples one after the
// other (the reference's RNG runs on from sample to sample of a pixel), so a tile is done when the wave
// with the most blocks is: nPixels/64 blocks rarely divide evenly over the resident waves (a 1/8-height
// 1080p tile is 4050 blocks for 5120 waves), and a slightly smaller block that gives every wave the
// same number of blocks shortens that critical path. Measured block time ~ (80 + pixels) (drain of the
// longest ray and the shading step do not shrink with the block); beyond two blocks per wave the
// dynamic hand-out evens the waves out by itself and whole 8x8 blocks are best.
uint32_t fused_batch_pixels(const Tuning& t, uint32_t nPixels, uint32_t waves, uint32_t evenBelow) {
    if (t.batchPixels > 0) return (uint32_t)std::min(t.batchPixels, (int)RT_WAVE);
    if (((uint64_t)nPixels + RT_WAVE - 1) / RT_WAVE > (uint64_t)evenBelow * waves) return RT_WAVE;
    uint32_t best = RT_WAVE;
    uint64_t bestCost = ~0ull;
    for (uint32_t b = RT_WAVE; b >= 16; b--) {
        const uint64_t nb = (nPixels + b - 1) / b;
        const uint64_t rounds = (nb + waves - 1) / waves;
        const uint64_t cost = rounds * (uint64_t)((uint32_t)t.batchFixed + b);
        if (cost < bestCost) { bestCost = cost; best = b; }
    }
    return best;
}
}  // namespace

FusedShape fused_shape(const Tuning& t, const Measured& m, const DispatchFacts& d, uint32_t resident) {
    FusedShape s;
    const uint32_t nSlots = (uint32_t)dispatch_slots(d.nPixels, d.nFrames);  // rt_render_frames: frames are more slots of the same tile
    // Pixels are replaced as they finish when rays are long (Sponza -7 %, its 1/2 and 1/4 tiles -8 % and -11 %: the wave no
    // longer drains to its slowest pixel once per block) and when a wave gets fewer than five blocks (Cornell + bunny /
    // + dragon, rank 0's rows of 2 GPUs -3 %, of 4 GPUs -13 %); with short rays and many blocks per wave a block at a
    // time is 4-7 % faster (the full 1080p frame of Cornell, + bunny, + dragon)
    // (scenes whose paths end early — open scenes, most samples leave after a bounce or two: fewer than 2.5 segments per sample
    // against ~4 in a closed box — empty a block's lanes unevenly; there replacing pays up to eight blocks per wave:
    // tools/heuristics_table.py, 256 bunnies on a floor under the sky, one 1080p frame: 19.1 against 19.7 ms)
    const uint64_t fewBelow = (m.segPerPath >= 0.0 && m.segPerPath < 2.5) ? 8ull : 5ull;
    const bool fewBlocks = ((uint64_t)nSlots + RT_WAVE - 1) / RT_WAVE < fewBelow * resident * (RT_BLOCK / RT_WAVE);
    s.pixelRefill = t.pixelRefill > 0 ? (uint32_t)t.pixelRefill
                  : ((m.boxPerRay >= (double)t.fusedBelowBoxTests || fewBlocks) ? 8u : (uint32_t)RT_WAVE);
    // a wave that replaces its pixels one by one evens out by itself as soon as there is more than one block per wave
    s.evenBelow = s.pixelRefill < RT_WAVE ? 1u : 2u;
    const uint32_t wavesResident = resident * (RT_BLOCK / RT_WAVE);
    s.batchPixelsEven = s.batchPixels = fused_batch_pixels(t, nSlots, wavesResident, s.evenBelow);
    // With one or two blocks per wave (one, when pixels are replaced as they finish) the tile is done when the most expensive block is: blocks made of 4-slot chunks from
    // all over the tile cost about the same (-6 % on a 1/8-height 1080p tile); with more blocks per wave the dynamic
    // hand-out balances by itself and neighbouring pixels (shared cache lines, coherent rays) are 3-8 % faster.
    s.g = d.nFrames > 1u ? 0u : t.scatter >= 0 ? (uint32_t)t.scatter : ((((uint64_t)nSlots + RT_WAVE - 1) / RT_WAVE <= (uint64_t)s.evenBelow * wavesResident) ? 4u : 0u);
    if (s.g) s.batchPixels = std::min((uint32_t)RT_WAVE, (s.batchPixels + s.g - 1) / s.g * s.g);
    s.nBatches = s.g ? ((nSlots + s.g - 1) / s.g + s.batchPixels / s.g - 1) / (s.batchPixels / s.g) : (nSlots + s.batchPixels - 1) / s.batchPixels;
    s.blocks = std::max(1u, std::min((s.nBatches + (RT_BLOCK / RT_WAVE) - 1) / (RT_BLOCK / RT_WAVE), resident));
    // lanes at interior nodes that make the wave skip the vote: long rays (Sponza: 157 box tests per ray) want the interior step
    // to wait for more lanes (40: -4 %); 24 for short rays and until the scene is measured
    s.fastLanes = t.fastLanesSet ? (uint32_t)t.fastLanes : (m.boxPerRay >= (double)t.fusedBelowBoxTests ? 40u : 24u);
    s.wSetup = (uint32_t)t.wSetupFused;
    s.wLeaf = (uint32_t)t.wLeafFused;
    s.waveTimes = d.phaseStats != 0;
    return s;
}
