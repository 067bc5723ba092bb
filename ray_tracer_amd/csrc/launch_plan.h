// launch_plan.h — how a dispatch is to be run, decided on the host: the knobs (Tuning), what earlier dispatches measured
// (Measured) and the pure functions that turn them, the scene and the dispatch into a pipeline, parts, a kernel and launch
// shapes. Nothing in this pair of files needs a device: rt_device.hip gathers the facts, asks here, and allocates, launches and
// records; tests/launch_plan_check.cpp pins every decision on the CPU.
#pragma once

#include <stdint.h>

#include <string>

#define RT_WAVE 64
#define RT_BLOCK 256
#define RT_MAX_LANES 4
// the wide work-group of the persistent-wave traversal (k_trace_pw_wide, KernelKey::threads): RT_WIDE_GROUPS groups of RT_WIDE_THREADS
// threads per CU are six waves per SIMD, and the two of them share the LDS with two copies of the top-level table instead of five
// or six: all RT_WIDE_HOT = RT_HOT_PAIRS pairs fit beside 21-entry stacks (the static_assert beside hot5 / hot6)
#ifndef RT_WIDE_THREADS
#define RT_WIDE_THREADS 768
#endif
#ifndef RT_WIDE_GROUPS
#define RT_WIDE_GROUPS 2
#endif
#ifndef RT_WIDE_HOT
#define RT_WIDE_HOT 192
#endif
#define RT_FRAMES_MAX_SLOTS (24ull << 20)   // default for the paths of one multi-frame dispatch (ten 1080p frames or three 4K frames: 5.8 GB of path state)

// ---------------------------------------------------------------- tuning: what rt_set_tuning writes, each "given explicitly" flag beside the knob it qualifies
struct Tuning {
    int objTreeMin = 48;    // rt_set_tuning("object_tree_min"): general-transform objects from which the object hierarchy is built (0 = never)
    int framesPerLaunch = 0; // rt_render_frames: most frames of a tile rendered by one launch (0 = as many as fit)
    uint64_t framesMaxSlots = RT_FRAMES_MAX_SLOTS;  // most paths of one multi-frame dispatch (rt_render_frames)
    uint64_t radianceMaxSlots = 0;  // rt_set_tuning("radiance_max_kslots"): most rays of one piece of an rt_query_radiance batch (0 = framesMaxSlots)
    int cameraReuse = 1;    // rt_set_tuning("camera_reuse", 0): trace the camera ray of every sample
    int lightQueries = 1;   // rt_set_tuning("light_queries", 0): trace every NEE ray and cosine probe in full
    int lanes = 3;                        // rt_set_tuning("lanes", 1..RT_MAX_LANES)
    bool lanesSet = false;                // "lanes" given explicitly: no automatic fall-back to one part
    uint32_t lanesMinSlots = 1u << 20;    // dispatches of fewer paths than this stay in one part
    uint64_t wideMinSlots = 1u << 20;     // rt_set_tuning("wide_min_kslots"): dispatches of at least this many paths run the 20-entry, table-carrying traversal in wide
                                          // work-groups (k_trace_pw_wide; trace_kernel_key). 0 = always, more than a dispatch can have = never. The default is
                                          // lanesMinSlots: the dispatches that go into parts
    int wideGridPct = 40;                 // rt_set_tuning("wide_grid_pct"): the share of the resident WIDE work-groups a launch takes while a dispatch runs in several
                                          // parts and lane_grid_pct is automatic (0 = the parts' share as it is). Three parts of 6.9 M paths: 67.3 ms per step at 40,
                                          // 69.5 at 50, 72.5 at 60, 67.7 at 37, 72.4 at 30 (profiles/README.md, Round 6); the 256-thread groups keep their 50
    int laneGridPct = 0;                  // rt_set_tuning("lane_grid_pct"): share of the resident work-groups a k_trace_pw launch takes while a dispatch runs in several parts (0 = by the parts' size: 50, 40 below 1.2 M paths per part)
    int traceVariant = 1;   // 0 = one-ray-per-lane k_trace, 1 = persistent waves k_trace_pw
    int pipeline = -1;      // 0 = multi-kernel wavefront pipeline, 1 = wave-private fused pipeline (k_render_fused), -1 = by tile size
    uint32_t fusedBelowPixels = 4000000;  // auto: dispatches of fewer paths than this use the fused pipeline — scaled down to 1.5 M as the rays get longer
                                          // (choose_pipeline: sizeLimit). Sponza, 8 spp, ms per step with 1 / 2 / 4 / 10 frames of 1080p in one dispatch
                                          // (round 3, multi-kernel in three parts): fused 113.8 / 109.4 / 107.4 / 105, multi-kernel 103.4 / 90.7 / 84.7 / 79.5
    uint32_t fusedBelowBoxTests = 70;     // auto: ... and so do scenes whose rays are short (EXECUTED box tests per ray, measured), with one exception (choose_pipeline)
    int refill = 8;         // k_trace_pw: idle lanes that trigger a refill
    int refillMk = 16;      // the same for k_trace_pw over the global queue when set by hand ("mk_refill"); automatic: 12 for long rays, 16 otherwise (trace_shape)
    bool refillMkSet = false;  // given explicitly (else by the scene's ray length, trace_shape)
    int chunk = 256;        // k_trace_pw: most queue entries reserved per atomic
    int ldsStackCap = 24;   // k_trace_pw: LDS stack entries per lane (8, 16 or 24); deeper BVHs use the overflow buffer
    int fastLanes = 32;     // k_trace_pw: lanes at interior nodes that skip the full vote (4K Sponza: 24 -> 32 is -2 %, 1080p: equal)
    bool fastLanesSet = false;  // fast_lanes given explicitly: it then also applies to the fused pipeline
    int wSetup = 16, wLeaf = 16; // k_trace_pw: vote weights in eighths (interior = 8); the set-up weight when set by hand ("mk_w_setup"), automatic: 32 for long rays, 16 otherwise
    bool wSetupSet = false, wLeafSet = false;  // given explicitly (the set-up weight else by the scene's ray length, trace_shape)
    int wSetupFused = 16, wLeafFused = 24;  // vote weights of the fused pipeline (short private lists: leaves and set-ups sooner)
    int blocksPerCU = 0;    // k_trace_pw: 0 = occupancy query
    int phaseStats = 0;     // diagnostic: k_trace_pw counts rounds / active lanes per phase
    int tileSlots = 1;      // slots follow 8x8 pixel blocks instead of rows
    int fastShare = 10;     // sixteenths of the live lanes that suffice to skip the vote (0 = fixed count only): -1..-2 % everywhere
    int maskIdentity = 0;   // identity-transform objects in the rays' object masks too (rt_update_objects reads it)
    int scatter = -1;       // fused pipeline: blocks made of chunks of this many slots from all over the tile; 0 = neighbouring pixels; -1 = auto
    int hotPairs = 2;       // k_trace_pw: child pairs of the meshes' top levels from LDS. 0 = off, 1 = as many as fit beside the stacks of
                            // six work-groups per CU, 2 = of five (Sponza, 21-entry stacks, ten frames in flight: 90.4 / 90.6 / 88.7 ms per step)
                            // — or, for a 20-entry stack in a big dispatch, all of them beside two wide work-groups (wideMinSlots)
    int pixelRefill = 0;    // fused pipeline: free lanes at which a wave reserves new pixels (64 = a block at a time, 0 = by ray length)
    int batchPixels = 0;    // fused pipeline: pixels per wave-private block (0 = chosen per launch)
    int batchFixed = 80;    // ... and the fixed part of a block's cost in the chooser, in pixel units
    int triPlane = 1;       // rt_query_triangles: 1: the descent also discards a node that lies beside the query's plane (pruning (b)); 0: by boxes only. Same answer.
    int fusedMaps = 0;      // 1: a scene that binds an alpha, metalness or bump map may take the fused pipeline (k_render_fused_maps); 0: multi-kernel only
    int probe = 1;          // measure an unknown scene with a small dispatch before its first big one
};

// rt_set_tuning on a Tuning: `error` is empty when the key and the value were accepted (a refused one leaves t as it was);
// rebuildEmitters: the emitter list follows the knob that changed ("light_queries")
struct TuningChange { std::string error; bool rebuildEmitters = false; };
TuningChange set_tuning(Tuning& t, const std::string& key, int value);

// ---------------------------------------------------------------- measured on earlier dispatches
struct Measured {
    bool snapPending = false;
    unsigned long long snapBox = 0, snapRays = 0, snapSeg = 0, snapPaths = 0;  // counters at the previous snapshot
    double boxPerRay = -1.0;              // < 0: not measured yet
    double segPerPath = -1.0;             // path segments per pixel sample of this scene, from the same snapshots (< 0: not measured yet)
};
// the device counters the measurements are taken from, as copied back
struct RayCounters { unsigned long long boxTests, skippedBoxTests, raysTraced, segments, paths; };
void fold_snapshot(Measured& m, const RayCounters& snap);                             // a counter snapshot that has arrived
void fold_probe(Measured& m, const RayCounters& before, const RayCounters& after);   // the counters around the ray-cost probe

// ---------------------------------------------------------------- the facts a plan is made from
struct SceneFacts {
    uint32_t maxLeafDepth = 0;
    bool cull = false;       // kernels with the object-skipping code (CULL) for this scene
    uint32_t mapFlags = 0;   // RT_MAP_*
    uint32_t hotNodes = 0, nodeCount = 0, triCount = 0;
};
struct DispatchFacts {
    uint32_t nPixels = 0, nFrames = 1, samples = 0;
    int debug = -1;
    bool pixStats = false;   // per-pixel box/triangle counts are wanted (debug heat maps)
    bool perRay = false;     // per-ray counters are wanted (rt_trace_rays)
    int phaseStats = 0;      // "phase_stats" as it holds for this dispatch
    int pipeline = -1;       // "pipeline" as it holds for this dispatch
    bool probe = false;      // the ray-cost probe itself
    int gridPct = 100;       // share of the resident work-groups a k_trace_pw launch of this part takes
    uint32_t groupThreads = RT_BLOCK;  // threads of a work-group of the launch's kernel (KernelKey::threads; trace_shape)
    bool counted = false;    // its traversal launches are counted ...
    uint64_t launches = 0;   // ... and this many have been so far (phase_stats >= 2)
};

// Paths of a dispatch. Several frames in one dispatch: the paths are {64 tile slots} x {frames} (FrameParams::nFrames; rt_kernels.hip.h:
// frame_slot), in either pipeline
inline uint64_t frame_slots(uint64_t nPixels) { return (nPixels + 63) / 64 * 64; }
inline uint64_t dispatch_slots(uint64_t nPixels, uint32_t nFrames) { return nFrames > 1u ? frame_slots(nPixels) * nFrames : nPixels; }

// ---------------------------------------------------------------- the decisions
int choose_pipeline(const Tuning& t, const Measured& m, const SceneFacts& s, const DispatchFacts& d);   // 0 = multi-kernel, 1 = fused

// the rows y = row0 + k*rowStride, k in [0,nRows) of a tile
struct TileRows { uint32_t row0, rowStride, nRows; };
bool probe_first(const Tuning& t, const Measured& m, const SceneFacts& s, const DispatchFacts& d);
TileRows probe_rows(const TileRows& tile);

int choose_parts(const Tuning& t, const Measured& m, const SceneFacts& s, const DispatchFacts& d);
int part_grid_pct(const Tuning& t, int nParts, uint32_t firstPartSlots);
struct PartSlices { uint32_t begin[RT_MAX_LANES], n[RT_MAX_LANES]; int gridPct; };
PartSlices slice_parts(const Tuning& t, uint32_t nSlots, uint32_t nFrames, int nParts);

uint32_t frames_per_dispatch(const Tuning& t, uint64_t framePixels, uint32_t nFrames, int debug);

// The traversal kernel of a launch, by its template arguments. stack and ovf always say what the kernel's stack is (the overflow
// buffer is sized by them); the other arguments stay 0 / false where a family does not have them. rt_device.hip turns a key into
// the instantiation's address and name; a key it has no instantiation for is an error there.
// blocks: the work-groups per CU the kernel is built for; threads: those of one work-group. RT_BLOCK everywhere but in the wide
// traversal kernel (family trace_pw with threads == RT_WIDE_THREADS: k_trace_pw_wide<stack, hot, threads>, blocks == RT_WIDE_GROUPS).
enum class KernelFamily { trace, trace_pw, trace_pw_alpha, render_fused, render_fused_maps };
struct KernelKey {
    KernelFamily family;
    int stack;
    bool ovf, pix, stats, cull;
    int hot, blocks;
    int threads = RT_BLOCK;
};
// top-level pairs from LDS (k_trace_pw<HOT>): what 160 KB of LDS per CU leave beside the stacks. hot_pairs 1: six work-groups
// per CU, 2: five (more pairs, no spills at 96 registers)
// (the overflow-stack kernel with 16 entries in LDS keeps six work-groups AND 120 pairs: deep BVHs, see trace_kernel_key)
constexpr int hot6(int stack, bool ovf) { return ovf ? (stack == 16 ? 120 : 0) : stack == 8 ? 192 : stack == 16 ? 136 : stack == 20 ? 72 : 0; }
constexpr int hot5(int stack, bool ovf) { return ovf ? 0 : stack == 24 ? 80 : stack == 20 ? 144 : 192; }
// the wide kernel's LDS: per work-group the 21-entry stacks of its threads (+1: pushes are unconditional), 1 KB of object metadata
// (RT_META_LDS) and the table, 64 B a pair; RT_WIDE_GROUPS of them in a CU's 160 KB
constexpr uint32_t wide_group_lds(int stack, int hot, int threads) { return (uint32_t)threads * (uint32_t)(stack + 1) * 4u + 1024u + (uint32_t)hot * 64u; }
static_assert(RT_WIDE_GROUPS * wide_group_lds(20, RT_WIDE_HOT, RT_WIDE_THREADS) <= 160u * 1024u, "the wide work-groups of a CU and their tables fit its LDS");
static_assert(RT_WIDE_THREADS % RT_WAVE == 0 && RT_WIDE_THREADS <= 1024 && RT_WIDE_GROUPS * RT_WIDE_THREADS == 6 * 4 * RT_WAVE, "six waves per SIMD in whole work-groups");
KernelKey trace_kernel_key(const Tuning& t, const SceneFacts& s, const DispatchFacts& d);   // a traversal launch of the multi-kernel pipeline, rt_trace_rays or an AOV pass
KernelKey fused_kernel_key(const Tuning& t, const SceneFacts& s, const DispatchFacts& d);   // the fused pipeline's one launch

// `resident`: the work-groups of the chosen kernel the device holds at once (rt_device.hip asks the runtime)
struct TraceShape { uint32_t blocks, refillMk, wSetup; bool waveTimes; };
TraceShape trace_shape(const Tuning& t, const Measured& m, const SceneFacts& s, const DispatchFacts& d, uint32_t maxRays, uint32_t resident);

struct FusedShape {
    uint32_t pixelRefill, evenBelow;
    uint32_t batchPixelsEven, batchPixels;   // pixels per wave-private block before and after the scatter rounding
    uint32_t g, nBatches, blocks, fastLanes, wSetup, wLeaf;
    bool waveTimes;   // phase_stats: the waves' clocks are recorded
};
FusedShape fused_shape(const Tuning& t, const Measured& m, const DispatchFacts& d, uint32_t resident);
