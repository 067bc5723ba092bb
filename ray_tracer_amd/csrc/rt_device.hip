// rt_device.hip — device half of the C ABI: context, uploads, the wavefront
// render loop. Replaces the Vulkan seam of the reference (copy_buffer /
// update_buffer / run_compute, src/vk_engine.cpp:1401-1475,1623-1676) with
// hipMalloc'd buffers and HIP launches on one stream per context.
//
// There is no CPU fallback anywhere in this file: without a HIP device
// rt_create fails and nothing else can be called.

#include "rt_kernels.hip.h"
#include "bvh_build.hip.h"
#include "rt_refit.hip.h"  // the kernels of rt_update_points; mesh_refit.h: the plan they run, the checks and the rule
#include "launch_plan.h"   // every decision about how a dispatch is run: this file gathers the facts, asks there, and launches
#include "post_passes.h"   // likewise for the passes over finished frames: their checks, their input planes, the temporal history
#include "ray_queries.h"   // ... and for the ray queries and the ambient-occlusion pass: their checks and the arithmetic of a batch
#include "radiance_queries.h"   // ... and for the radiance queries: their checks, pieces, byte counts and seed
#include "host_staging.h"       // ... and for every _host form: where its arrays lie in the staging buffer
#include "rt_nearest.hip.h"     // the kernel of the point queries; point_queries.h: their checks, the arithmetic of a batch, the pruning table
#include "rt_nearest_side.hip.h"  // the side pass of the signed point queries; mesh_topology.h: its table, checks and host form
#include "point_queries.h"
#include "mesh_topology.h"
#include "rt_ray_hits.hip.h"      // the kernels of the all-hit ray queries; ray_hits.h: their checks, the arithmetic of a batch, the stack choice
#include "ray_hits.h"
#include "rt_point_within.hip.h"  // the kernels of the radius point queries; point_within.h: their checks, the arithmetic of a batch, the stack choice
#include "point_within.h"
#include "rt_sweep.hip.h"         // the kernel of the sphere sweeps; sweep_queries.h: their checks, the arithmetic of a batch, the stack choice
#include "sweep_queries.h"
#include "rt_irradiance.hip.h"    // the two kernels of the baked-light queries around the radiance pipeline; irradiance_queries.h: their checks, chunks and byte counts
#include "irradiance_queries.h"
#include "rt_texels.hip.h"        // the kernels of the lightmap texel passes; texel_queries.h: their checks, launch shapes, scan levels and byte counts
#include "texel_queries.h"
#include "rt_box_overlap.hip.h"   // the kernel of the box queries; box_queries.h: their checks, the arithmetic of a batch, the stack choice
#include "box_queries.h"
#include "rt_obb_overlap.hip.h"   // the kernel of the oriented box queries; obb_queries.h: their checks, the arithmetic of a batch, the stack choice
#include "obb_queries.h"
#include "rt_tri_overlap.hip.h"   // the kernel of the triangle queries; tri_queries.h: their checks, the arithmetic of a batch, the stack choice
#include "tri_queries.h"
#include "rt_tri_cut.hip.h"   // the kernel of the cut queries; cut_queries.h: the arithmetic of a batch, the stack choice
#include "cut_queries.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

namespace {

struct DevBuf {  // device memory that belongs to whoever holds this: move-only, freed with it
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

struct EventPair { hipEvent_t a, b; };
// A plane (or set of planes) the ctx keeps for a caller who passed NULL: the memory, the pixels of the call that last wrote it, whether
// there was one, and, where the plane has rows, the rows of the image it holds (the passes read it only as a whole frame)
struct OwnedPlane {
    DevBuf buf;
    size_t pixels = 0;
    bool valid = false;
    RowsOf rows;
    OwnedRows owned() const { return OwnedRows{buf.p, valid, rows}; }
};

}  // namespace

struct rt_ctx {
    std::string error;
    // ---- resources: device, streams, events, buffers, communicator, and the host's view of what the buffers hold. Written by
    // rt_create, the upload / update entry points, the ensure / allocate helpers and rt_destroy.
    int device = 0, numCUs = 256;
    hipStream_t ownStream = nullptr, stream = nullptr;  // rt_set_stream: the ctx stream is the caller's or the ctx's own
    // scene
    DevScene sc{};
    std::vector<DevBuf> sceneBufs;
    DevBuf texelBuf, texInfoBuf, triUVBuf, objTreeBuf, objCostBuf;
    DevBuf matBuf, sphereBuf, sphereMatBuf, objInvBuf, objFwdBuf, objMetaBuf, objBoxBuf, objSkipBuf, maskBoxBuf, emitBuf, emitPreBuf;
    SceneSources host;      // host copies of what the emitter list and the map flags are derived from (rebuild_emitters)
    DevBuf objAlphaBuf;     // per object: its material's alpha map and sampler (rebuild_emitters)
    uint32_t maxLeafDepth = 0;
    std::vector<RootInfo> rootOf;             // per reference node; idx = ~0u unless a mesh root
    bool cull = false;      // kernels with the object-skipping code (CULL) for this scene
    std::vector<RenderObject> hostObjects;    // the objects behind the object tables (set_objects): a refit lays them out again over the new root boxes
    // deforming meshes (rt_upload_scene_dynamic keeps, rt_update_points uses; a plain rt_upload_scene releases all of it): the
    // scene's points and the triangles' {v0, v1, v2, frontOnly} on the device, the refit plan with its index lists, and a pinned
    // plane the refit roots' boxes come back through
    struct Dynamic {
        bool on = false;
        RefitPlan plan;
        DevBuf points, triIdx, leaves, interior, levels;
        float4* rootHost = nullptr;   // pinned, 2 x float4 per mesh of the plan
    } dyn;
    // multi-GPU (rt_comm_*): this rank's RCCL communicator, a staging buffer on the gathering rank
    ncclComm_t comm = nullptr;
    int commRanks = 0, commRank = 0;
    DevBuf gatherBuf;
    // path state
    DevBuf stateBuf, queueBuf, counterBuf, scratchBuf;
    DevBuf hostStageBuf;    // the arrays of whichever _host form runs (staged): idle between calls, no pointer into it ever leaves the library
    OwnedPlane fb;          // the ctx framebuffer (render_impl writes it, rt_clear_framebuffer forgets it)
    DevBuf overflowBuf[RT_MAX_LANES];     // per part (Dispatch::part): the traversal stack entries beyond LDS
    // Multi-kernel pipeline in `lanes` independent parts (render_parts): the paths of a dispatch are split into contiguous slot
    // ranges, each with its own queues, counters and stream, so that one part's k_shade and the tail of its k_trace_pw launch
    // run under the other part's traversal. Part 0 is the ctx stream itself; the others fork from it and join it.
    hipStream_t sideStream[RT_MAX_LANES - 1] = {};
    hipEvent_t forkEvent = nullptr, joinEvent[RT_MAX_LANES - 1] = {}, pollEventSide[RT_MAX_LANES - 1] = {};
    uint32_t capacity = 0;  // pixels the state buffers hold
    PathState ps{}; Queues q{};
    uint32_t* hostCounts = nullptr;  // pinned, 4 words
    // profiling of the traversal kernel (rt_set_profiling switches it; prof_begin takes events from the pool, harvest_events returns them)
    bool profiling = false;
    std::vector<EventPair> evPool;
    size_t evUsed = 0;
    hipEvent_t profBase = nullptr;                         // recorded when profiling is switched on: the origin of traceSpans
    // box tests per ray of this scene, from counter snapshots copied back asynchronously after each dispatch
    DevCounters* snap = nullptr;          // pinned
    hipEvent_t snapEvent = nullptr;
    hipEvent_t pollEvent = nullptr;       // multi-kernel pipeline: the active-path count on its way back (never waited for)
    DevBuf probeBuf;        // framebuffer of the ray-cost probe
    DevBuf waveTimeBuf;     // phase_stats: per-wave start/end clocks of the last k_trace_pw launch
    // first-hit AOV passes (rt_render_aovs): the ctx-owned planes of the last pass into them, and a counter block of their own, which
    // rt_get_counters adds to the rendering counters and the ray-cost snapshots never see
    OwnedPlane aov;         // the five planes in AovPlane's order (rt_render_aovs writes them)
    DevBuf aovCounterBuf;
    // mirror-following guide planes (rt_render_guides): the ctx-owned set of the last pass into it, in the same order, and the ray
    // counts of the pass's rounds (GUIDE_COUNTS words)
    OwnedPlane guide;
    DevBuf guideCountBuf;
    // ray queries and the ambient-occlusion pass (rt_query_*, rt_render_ao): the pass's queue (one entry per ray, holes for the rays
    // that are answered without a traversal), the occluded counts of rt_render_ao's rounds and the ctx-owned plane of the last
    // rt_render_ao(..., d_ao = NULL) with its pixel count (0: never written)
    DevBuf queryQueueBuf, aoCountBuf, aoBuf;
    DevBuf objNearBuf;      // point queries: the per-object pruning table (layout_nearest), which follows the object tables (set_objects)
    // signed point queries: the topology table and the per-object orientations (rt_upload_topology), with the counts of the scene
    // they were made for. A scene upload drops them; set_objects refreshes the orientations beside objNearBuf
    struct Topology {
        bool on = false;
        TopologyCounts counts;
        DevBuf rows, orient;
    } topo;
    DevBuf hitsListBuf;     // all-hit ray queries: the lists of k_ray_hits<64, true>, whose stack leaves no LDS for them
    DevBuf withinListBuf;   // radius point queries: the lists of k_points_within<64, true>, likewise
    DevBuf boxesListBuf;    // box queries: the lists of k_boxes_overlap<64, true>, likewise
    DevBuf irradianceBuf;   // baked-light queries: a chunk's rays, ray ids and radiance records (irradiance_scratch), at most 44 bytes x the piece cap
    // lightmap texels: a bake's planes and scan (texel_scratch), the compaction's block sums, the dilation's second plane, and
    // rt_bake_lightmap's records, batch and values (lightmap_scratch)
    DevBuf bakeTexelBuf, bakeScanBuf, bakeDilateBuf, lightmapBuf;
    size_t aoPixels = 0;
    DevBuf shadeStatBuf;                  // k_shade's striped statistics (ShadeStatStripe), zero between dispatches
    // the denoiser (rt_denoise): its work planes and the ctx-owned output
    DevBuf dnWorkBuf;
    OwnedPlane dnOut;
    // temporal accumulation (rt_temporal_accumulate): the two histories a call reads and writes in turn and the ctx-owned frame and moments
    DevBuf tpHist[2];
    OwnedPlane tpOut, tpMom;
    // sample counts from the moments (rt_build_sample_map): the statistics of the last build and whether there was one
    DevBuf smStatBuf;
    bool smBuilt = false;
    // following moved objects and spheres: the motion table on the device with its pinned staging copy and the event that says the
    // copy has been read (upload_motion)
    DevBuf tpMotionBuf;
    float4* tpMotionHost = nullptr; size_t tpMotionHostBytes = 0;
    hipEvent_t tpMotionEvent = nullptr;

    // ---- the temporal history as the host sees it: which of tpHist the last accepted call wrote, at what size and through which
    // camera, the placements it saw and the ones now on the device (post_passes.h). Written through its own transitions only, by
    // rt_upload_scene, set_objects, set_spheres, rt_temporal_reset, rt_temporal_track_motion and rt_temporal_accumulate.
    TemporalHistory temporal;

    // ---- tuning: what rt_set_tuning writes (launch_plan.h: set_tuning). Nothing else assigns to it.
    Tuning tune;

    // ---- measured on earlier dispatches. Written by poll_ray_cost, request_ray_cost, probe_ray_cost, measured_new_scene and rt_reset_counters only.
    Measured meas;

    // ---- reports: written by the launch functions, harvest_events and rt_bvh_build, zeroed by rt_reset_counters, read by rt_last_* / rt_get_*.
    struct Reports {
        int lastPipeline = 0;   // what the last rt_render used
        int lastParts = 1;                    // parts the last multi-kernel dispatch ran in (rt_last_parts)
        char lastKernel[96] = "";  // the traversal kernel instantiation of the last launch, as a demangler prints it (rt_last_kernel)
        size_t waveTimesCount = 0;
        double traceMs = 0.0;
        uint64_t traceLaunches = 0;
        std::vector<std::pair<float, float>> traceSpans;       // [start, end) of every bracketed launch, ms since profBase (rt_get_trace_busy_ms)
        uint64_t traceLaunchesTotal = 0, aovLaunches = 0;      // traversal launches of the rendering dispatches and of the AOV passes
        double bvhBuildMs = 0.0; // last rt_bvh_build
    } rep;
    int fail(const std::string& m) { error = m; return -1; }
    int hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return 0;
        error = std::string(what) + ": " + hipGetErrorString(e);
        return -(int)e - 1000;
    }
};

#define RT_HIP(ctx, call)                                    \
    do {                                                     \
        int _rc = (ctx)->hip((call), #call);                 \
        if (_rc) return _rc;                                 \
    } while (0)

namespace {

int dev_alloc(rt_ctx* c, DevBuf& b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return 0;
    b.release();
    if (bytes == 0) bytes = 256;
    RT_HIP(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return 0;
}

int upload(rt_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    int rc = dev_alloc(c, b, bytes);
    if (rc) return rc;
    if (bytes) RT_HIP(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));  // src is borrowed for the call only
    return 0;
}

// A ctx-owned plane of 16-byte records to the host; blocks. fn: the entry point, never: what it says when no call ever wrote the plane
int read_plane(rt_ctx* c, const OwnedPlane* pl, const char* fn, const char* never, float* out, size_t nFloats) {
    if (!c || !out) return -1;
    if (!pl->valid) return c->fail(never);
    if (nFloats != pl->pixels * 4) return c->fail(std::string(fn) + ": size mismatch");
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipMemcpyAsync(out, pl->buf.p, nFloats * 4, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// upload a table and point its DevScene field at it
template <typename T>
int upload_table(rt_ctx* c, DevBuf& b, const std::vector<T>& v, const T*& field) {
    int rc = upload(c, b, v.data(), v.size() * sizeof(T));
    if (rc) return rc;
    field = (const T*)b.p;
    return 0;
}

// The host-memory (_host) form of a device entry point. A part is one array of the call: `up` is copied to the device before the
// pass, `down` is copied back after it (both: in/out), and a part of 0 bytes is absent: the pass sees NULL for it. The parts lie in
// hostStageBuf by the one rule of host_staging.h; `pass` runs the device form on dev[k], the device address of part k. A pass that
// returns non-zero ends the call with that code and nothing comes back; otherwise the call blocks until the results are there.
// One buffer serves every form: a form that succeeds ends with a synchronise of the ctx stream, so the buffer is idle between
// successful calls; a call that failed after launching may have left work in flight, which is why the buffer still waits before
// it grows; and no device pointer into it is ever handed to a caller.
struct StagePart { const void* up; void* down; size_t bytes; };

template <size_t N, typename Pass>
int staged(rt_ctx* c, const StagePart (&parts)[N], Pass pass) {
    static_assert(N <= RT_STAGE_MAX_PARTS, "host_staging.h: RT_STAGE_MAX_PARTS");
    size_t bytes[N];
    for (size_t k = 0; k < N; k++) bytes[k] = parts[k].bytes;
    RT_HIP(c, hipSetDevice(c->device));
    const StageLayout g = stage_layout(bytes, (int)N);
    if (c->hostStageBuf.bytes < g.bytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees arrays a pass in flight may be using
    int rc = dev_alloc(c, c->hostStageBuf, g.bytes);
    if (rc) return rc;
    void* dev[N];
    for (size_t k = 0; k < N; k++) {
        dev[k] = bytes[k] ? (char*)c->hostStageBuf.p + g.offset[k] : nullptr;
        if (dev[k] && parts[k].up) RT_HIP(c, hipMemcpyAsync(dev[k], parts[k].up, bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = pass(dev))) return rc;
    for (size_t k = 0; k < N; k++)
        if (dev[k] && parts[k].down) RT_HIP(c, hipMemcpyAsync(parts[k].down, dev[k], bytes[k], hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int ensure_state(rt_ctx* c, uint32_t nPixels) {
    if (c->capacity >= nPixels && c->stateBuf.p) return 0;
    const size_t stride4 = (((size_t)nPixels * 16) + 255) & ~(size_t)255;  // bytes per float4 array
    const size_t stride1 = (((size_t)nPixels * 4) + 255) & ~(size_t)255;
    const int nF4 = RT_STATE_F4_ARRAYS, nU1 = 2;
    int rc = dev_alloc(c, c->stateBuf, stride4 * nF4 + stride1 * nU1);
    if (rc) return rc;
    PathState& ps = c->ps;
    ps.base = (float4*)c->stateBuf.p;
    ps.pitch = (uint32_t)(stride4 / 16);
    ps.pitchStat = (uint32_t)(stride1 / 4);

    // queues: 2 x active (n) + 2 x rays (3n) + 4 counters
    const size_t qa = (((size_t)nPixels * 4) + 255) & ~(size_t)255;
    const size_t qr = (((size_t)nPixels * 3 * 4) + 255) & ~(size_t)255;
    rc = dev_alloc(c, c->queueBuf, 2 * qa + 2 * qr + 256);
    if (rc) return rc;
    char* qb = (char*)c->queueBuf.p;
    c->q.active[0] = (uint32_t*)qb;
    c->q.active[1] = (uint32_t*)(qb + qa);
    c->q.rays[0] = (uint32_t*)(qb + 2 * qa);
    c->q.rays[1] = (uint32_t*)(qb + 2 * qa + qr);
    c->q.counts = (uint32_t*)(qb + 2 * qa + 2 * qr);
    c->capacity = nPixels;
    return 0;
}

// What the launch functions need to know about the dispatch (or pass) they launch for. Whoever starts one builds it and hands it
// down; the context keeps the buffers, the tuning and the measured statistics, and nothing of a dispatch.
struct Dispatch {
    DevScene sc;         // the uploaded scene with the counts of rayTraceParams (dispatch_scene)
    bool pixStats;       // per-pixel box/triangle counts are wanted (debug heat maps)
    int phaseStats;      // rt_set_tuning("phase_stats") as it holds for this dispatch (0 for the probe and the AOV pass)
    int pipeline;        // rt_set_tuning("pipeline") as it holds for this dispatch (the probe: 1)
    bool profiled;       // its traversal launches are bracketed by events (prof_begin)
    bool probe;          // the ray-cost probe: no probe of its own, no trace in rt_last_pipeline
    uint64_t* launches;  // the counter its traversal launches are added to (null: not counted)
    // the part of a multi-kernel dispatch being launched; everything else is one part
    hipStream_t stream;
    uint32_t* counts;    // the part's counter block
    int part;            // which overflow buffer
    int gridPct;         // share of the resident work-groups a k_trace_pw launch of this part takes
    uint32_t slots;      // the paths of the whole dispatch, all its parts together (0: a pass that is not a dispatch of paths)
};
// A dispatch in one part: the ctx stream, the first counter block (which ensure_state makes), the whole grid
Dispatch one_part(rt_ctx* c, const DevScene& sc, bool pixStats) {
    return Dispatch{sc, pixStats, c->tune.phaseStats, c->tune.pipeline, c->profiling, false, &c->rep.traceLaunchesTotal, c->stream, c->q.counts, 0, 100, 0};
}

// The facts the launch plan asks for (launch_plan.h), gathered from the context and the dispatch. fp: the dispatch's frame (the
// traversal launches of rt_trace_rays and of the AOV pass have none); perRay: per-ray counters are wanted (rt_trace_rays)
SceneFacts scene_facts(const rt_ctx* c, const Dispatch& d) {
    SceneFacts s;
    s.maxLeafDepth = c->maxLeafDepth; s.cull = c->cull;
    s.mapFlags = d.sc.mapFlags; s.hotNodes = d.sc.hotNodes; s.nodeCount = d.sc.nodeCount; s.triCount = d.sc.triCount;
    return s;
}
DispatchFacts dispatch_facts(const Dispatch& d, const FrameParams* fp, bool perRay) {
    DispatchFacts f;
    if (fp) { f.nPixels = fp->nPixels; f.nFrames = fp->nFrames; f.samples = fp->samples; f.debug = fp->debug; }
    f.pixStats = d.pixStats; f.perRay = perRay; f.phaseStats = d.phaseStats; f.pipeline = d.pipeline; f.probe = d.probe; f.gridPct = d.gridPct;
    f.counted = d.launches != nullptr; f.launches = d.launches ? *d.launches : 0;
    return f;
}

// A kernel to launch, the one whose occupancy sizes the grid (no heat maps, no phase statistics), and its name as a demangler
// prints it (rt_last_kernel; tests/test_instantiations.py compares it with `nm -C`). kernel == nullptr: no such instantiation.
template <typename K> struct KernelChoice { K kernel, occupancy; char name[sizeof rt_ctx::Reports::lastKernel]; };
using TraceChoice = KernelChoice<void (*)(DevScene, PathState, TraceArgs)>;
using TracePwChoice = KernelChoice<void (*)(DevScene, PathState, TracePwArgs)>;
using FusedChoice = KernelChoice<void (*)(FusedKernArgs)>;

template <typename K, typename... A>
KernelChoice<K> kernel_choice(K kernel, K occupancy, const char* format, A... a) {
    KernelChoice<K> k{kernel, occupancy, ""};
    snprintf(k.name, sizeof k.name, format, a...);
    return k;
}
const char* tf(bool b) { return b ? "true" : "false"; }

template <int STACK>
TraceChoice trace_kernel() { return kernel_choice(k_trace<STACK>, k_trace<STACK>, "k_trace<%d>", STACK); }
template <int STACK, bool OVF, bool PIX, bool STATS, bool CULL, int HOT = 0, int BLOCKS = 6>
TracePwChoice trace_pw_kernel() {
    return kernel_choice(k_trace_pw<STACK, OVF, PIX, STATS, CULL, HOT, BLOCKS>, k_trace_pw<STACK, OVF, false, false, CULL, HOT, BLOCKS>,
                         "k_trace_pw<%d, %s, %s, %s, %s, %d, %d>", STACK, tf(OVF), tf(PIX), tf(STATS), tf(CULL), HOT, BLOCKS);
}
template <int STACK, int HOT, int THREADS>
TracePwChoice trace_pw_wide_kernel() {
    return kernel_choice(k_trace_pw_wide<STACK, HOT, THREADS>, k_trace_pw_wide<STACK, HOT, THREADS>, "k_trace_pw_wide<%d, %d, %d>", STACK, HOT, THREADS);
}
template <int STACK, bool OVF, bool PIX, bool CULL>
FusedChoice fused_kernel() {
    return kernel_choice(k_render_fused<STACK, OVF, PIX, CULL>, k_render_fused<STACK, OVF, false, CULL>,
                         "k_render_fused<%d, %s, %s, %s>", STACK, tf(OVF), tf(PIX), tf(CULL));
}

// From a kernel key (launch_plan.h) to the instantiation: the key's arguments become template arguments by a walk over the
// instantiations there are, and a key that names none of them yields no kernel (the callers fail).
template <int N> using Stack = std::integral_constant<int, N>;

// f(Stack<STACK>, bool_constant<OVF>, bool_constant<CULL>) for the stacks a family is compiled with. Only the multi-kernel
// pipeline has a 20-entry kernel. (tests/test_instantiations.py makes a scene for each depth bucket the plan maps to these)
template <bool ALLOW20, typename F>
auto with_stack(const KernelKey& k, F&& f) {
    using Yes = std::true_type; using No = std::false_type;
    auto go = [&](auto S, auto O) { return k.cull ? f(S, O, Yes{}) : f(S, O, No{}); };
    if (k.stack == 8) return k.ovf ? go(Stack<8>{}, Yes{}) : go(Stack<8>{}, No{});
    if (k.stack == 16) return k.ovf ? go(Stack<16>{}, Yes{}) : go(Stack<16>{}, No{});
    if constexpr (ALLOW20) { if (k.stack == 20 && !k.ovf) return go(Stack<20>{}, No{}); }
    if (k.stack == 24) return k.ovf ? go(Stack<24>{}, Yes{}) : go(Stack<24>{}, No{});
    return decltype(go(Stack<8>{}, No{})){};
}

template <int STACK, bool OVF, bool CULL>
TracePwChoice trace_pw_of(const KernelKey& k) {
    constexpr int HOT6 = hot6(STACK, OVF), HOT5 = hot5(STACK, OVF);
    // (if constexpr: an instantiation the tables can never select is not compiled — every kernel in the library can be
    // launched, and tests/test_instantiations.py launches every one of them against the oracle)
    if (k.hot) {
        if (k.pix || k.stats) return {};
        if constexpr (HOT6 > 0) { if (k.hot == HOT6 && k.blocks == 6) return trace_pw_kernel<STACK, OVF, false, false, CULL, HOT6, 6>(); }
        if constexpr (HOT5 > 0) { if (k.hot == HOT5 && k.blocks == 5) return trace_pw_kernel<STACK, OVF, false, false, CULL, HOT5, 5>(); }
        return {};
    }
    if (k.blocks != 6 || (k.stats && !k.pix)) return {};
    if (k.stats) return trace_pw_kernel<STACK, OVF, true, true, CULL>();
    if (k.pix) return trace_pw_kernel<STACK, OVF, true, false, CULL>();
    return trace_pw_kernel<STACK, OVF, false, false, CULL>();
}

TraceChoice trace_choice(const KernelKey& k) {
    if (k.family != KernelFamily::trace) return {};
    switch (k.stack) {
        case 8: return trace_kernel<8>();
        case 16: return trace_kernel<16>();
        case 24: return trace_kernel<24>();
        case 32: return trace_kernel<32>();
        case 48: return trace_kernel<48>();
        case 64: return trace_kernel<64>();
    }
    return {};
}
TracePwChoice trace_pw_choice(const KernelKey& k) {
    if (k.family == KernelFamily::trace_pw_alpha)
        return kernel_choice(k.pix ? k_trace_pw_alpha<true> : k_trace_pw_alpha<false>, k_trace_pw_alpha<false>, "k_trace_pw_alpha<%s>", tf(k.pix));
    if (k.family != KernelFamily::trace_pw) return {};
    if (k.threads != RT_BLOCK) {  // wide work-groups: the one instantiation there is
        if (k.threads != RT_WIDE_THREADS || k.stack != 20 || k.ovf || k.pix || k.stats || k.cull || k.hot != RT_WIDE_HOT || k.blocks != RT_WIDE_GROUPS) return {};
        return trace_pw_wide_kernel<20, RT_WIDE_HOT, RT_WIDE_THREADS>();
    }
    return with_stack<true>(k, [&](auto S, auto O, auto C) { return trace_pw_of<S, O, C>(k); });
}
FusedChoice fused_choice(const KernelKey& k) {
    if (k.family == KernelFamily::render_fused_maps)
        return kernel_choice(k.pix ? k_render_fused_maps<true> : k_render_fused_maps<false>, k_render_fused_maps<false>, "k_render_fused_maps<%s>", tf(k.pix));
    if (k.family != KernelFamily::render_fused) return {};
    return with_stack<false>(k, [&](auto S, auto O, auto C) { return k.pix ? fused_kernel<S, O, true, C>() : fused_kernel<S, O, false, C>(); });
}
int no_kernel(rt_ctx* c, const KernelKey& k) {
    char m[160];
    snprintf(m, sizeof m, "the launch plan asks for a kernel the library does not hold: family %d <stack %d, ovf %d, pix %d, stats %d, cull %d, hot %d, blocks %d, threads %d>",
             (int)k.family, k.stack, (int)k.ovf, (int)k.pix, (int)k.stats, (int)k.cull, k.hot, k.blocks, k.threads);
    return c->fail(m);
}

// threads: those of a work-group of the kernel (KernelKey::threads)
template <typename K>
uint32_t resident_blocks(const rt_ctx* c, K kernel, int threads = RT_BLOCK) {
    int perCU = c->tune.blocksPerCU;
    if (perCU <= 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, threads, 0) != hipSuccess || perCU <= 0)) perCU = std::max(1, 4 * RT_BLOCK / threads);
    return (uint32_t)perCU * (uint32_t)c->numCUs;
}

// The plan picks an OVF kernel only for a BVH deeper than its stack; the map kernels have the buffer at any depth. Each part of
// a dispatch has its own: their launches run at the same time.
int overflow_buf(rt_ctx* c, const Dispatch& d, const KernelKey& k, uint32_t resident, uint32_t** out) {
    *out = nullptr;
    if (!k.ovf || c->maxLeafDepth <= (uint32_t)k.stack) return 0;
    DevBuf& ob = c->overflowBuf[d.part];
    int rc = dev_alloc(c, ob, (size_t)(c->maxLeafDepth - k.stack) * resident * (size_t)k.threads * 4);
    if (rc) return rc;
    *out = (uint32_t*)ob.p;
    return 0;
}

int wave_time_buf(rt_ctx* c, uint32_t blocks, unsigned long long** out, int threads = RT_BLOCK) {
    c->rep.waveTimesCount = (size_t)blocks * (size_t)(threads / RT_WAVE);
    int rc = dev_alloc(c, c->waveTimeBuf, c->rep.waveTimesCount * 16);
    if (rc) return rc;
    *out = (unsigned long long*)c->waveTimeBuf.p;
    return 0;
}

// HIP events around a traversal launch while profiling (harvest_events); the end also counts the launch
int prof_begin(rt_ctx* c, const Dispatch& d, EventPair** ev) {
    *ev = nullptr;
    if (!d.profiled) return 0;
    if (c->evUsed == c->evPool.size()) {
        EventPair p;
        RT_HIP(c, hipEventCreate(&p.a));
        RT_HIP(c, hipEventCreate(&p.b));
        c->evPool.push_back(p);
    }
    *ev = &c->evPool[c->evUsed++];
    RT_HIP(c, hipEventRecord((*ev)->a, d.stream));
    return 0;
}
int prof_end(rt_ctx* c, const Dispatch& d, EventPair* ev) {
    if (ev) RT_HIP(c, hipEventRecord(ev->b, d.stream));
    if (d.launches) ++*d.launches;
    return 0;
}

// The whole dispatch in one launch of k_render_fused, or of k_render_fused_maps for a scene that binds a map (fused_maps)
int launch_fused(rt_ctx* c, const Dispatch& d, const FrameParams& fp, float4* fb) {
    const DispatchFacts df = dispatch_facts(d, &fp, false);
    const KernelKey key = fused_kernel_key(c->tune, scene_facts(c, d), df);
    const FusedChoice k = fused_choice(key);
    if (!k.kernel) return no_kernel(c, key);
    EventPair* ev;
    int rc = prof_begin(c, d, &ev);
    if (rc) return rc;
    const uint32_t resident = resident_blocks(c, k.occupancy);
    const FusedShape s = fused_shape(c->tune, c->meas, df, resident);
    uint32_t* overflow;
    if ((rc = overflow_buf(c, d, key, resident, &overflow))) return rc;
    RT_HIP(c, hipMemsetAsync(d.counts + 5, 0, 4, d.stream));
    unsigned long long* waveTimes = nullptr;
    if (s.waveTimes && (rc = wave_time_buf(c, s.blocks, &waveTimes))) return rc;
    FusedArgs fa{d.counts + 5, fb, (DevCounters*)c->counterBuf.p, overflow, (uint32_t)c->tune.refill, s.wSetup, s.wLeaf, s.fastLanes, s.batchPixels, s.g, (uint32_t)c->tune.fastShare, waveTimes, s.pixelRefill};
    const FusedKernArgs ka{d.sc, c->ps, fp, fa};
    memcpy(c->rep.lastKernel, k.name, sizeof k.name);
    hipLaunchKernelGGL(k.kernel, dim3(s.blocks), dim3(RT_BLOCK), 0, d.stream, ka);
    RT_HIP(c, hipGetLastError());
    return prof_end(c, d, ev);
}

// the work counter (counts[4]) must be zero when this is called
// boundFromSeed: the rays' seed records carry a bound the traversal must start from (the ray queries' limits): only the
// persistent-wave kernels read a seed's distance (k_trace runs the sphere loop itself and starts at the miss distance), so the kernel
// is chosen as with "trace_variant" 1, whatever the knob says (the radiance queries ask for the same, so that every query pass runs one
// kernel family)
int launch_trace(rt_ctx* c, const Dispatch& d, uint32_t maxRays, const TraceArgs& ta, bool boundFromSeed = false) {
    if (maxRays == 0) return 0;
    const SceneFacts sf = scene_facts(c, d);
    DispatchFacts df = dispatch_facts(d, nullptr, ta.perRayBox != nullptr);
    df.nPixels = d.slots;   // (no frame here: the dispatch's paths, which decide between the 256-thread and the wide work-groups)
    Tuning keyTune = c->tune;
    if (boundFromSeed) keyTune.traceVariant = 1;
    const KernelKey key = trace_kernel_key(keyTune, sf, df);
    df.groupThreads = (uint32_t)key.threads;
    EventPair* ev;
    int rc;
    if (key.family == KernelFamily::trace) {  // one ray per lane, whole stack in LDS
        const TraceChoice k = trace_choice(key);
        if (!k.kernel) return no_kernel(c, key);
        if ((rc = prof_begin(c, d, &ev))) return rc;
        memcpy(c->rep.lastKernel, k.name, sizeof k.name);
        hipLaunchKernelGGL(k.kernel, dim3((maxRays + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, d.stream, d.sc, c->ps, ta);
    } else {  // persistent waves
        const TracePwChoice k = trace_pw_choice(key);
        if (!k.kernel) return no_kernel(c, key);
        if ((rc = prof_begin(c, d, &ev))) return rc;
        const uint32_t resident = resident_blocks(c, k.occupancy, key.threads);
        const TraceShape s = trace_shape(c->tune, c->meas, sf, df, maxRays, resident);
        uint32_t* overflow;
        if ((rc = overflow_buf(c, d, key, resident, &overflow))) return rc;
        unsigned long long* waveTimes = nullptr;
        if (s.waveTimes && (rc = wave_time_buf(c, s.blocks, &waveTimes, key.threads))) return rc;
        const TracePwArgs pa{ta.queue, ta.count, d.counts + 4, s.refillMk, (uint32_t)c->tune.chunk, s.wSetup, (uint32_t)c->tune.wLeaf, (uint32_t)c->tune.fastLanes, (uint32_t)c->tune.fastShare,
                             ta.perRayBox, ta.perRayTri, ta.counters, (unsigned long long*)((char*)c->counterBuf.p + sizeof(DevCounters)), waveTimes, overflow, ta.countAux, ta.countAux2, ta.auxOffset};
        memcpy(c->rep.lastKernel, k.name, sizeof k.name);
        hipLaunchKernelGGL(k.kernel, dim3(s.blocks), dim3((uint32_t)key.threads), 0, d.stream, d.sc, c->ps, pa);
    }
    RT_HIP(c, hipGetLastError());
    return prof_end(c, d, ev);
}

// the counters the measurements are taken from (launch_plan.h: fold_snapshot, fold_probe)
RayCounters ray_counters(const DevCounters& dc) { return RayCounters{dc.boxTests, dc.skippedBoxTests, dc.raysTraced, dc.segments, dc.paths}; }

// Fold in the counter snapshot of an earlier dispatch if its copy has arrived (never waits).
void poll_ray_cost(rt_ctx* c) {
    if (!c->meas.snapPending || hipEventQuery(c->snapEvent) != hipSuccess) return;
    c->meas.snapPending = false;
    fold_snapshot(c->meas, ray_counters(*c->snap));
}
// Queue the next snapshot behind the dispatch just enqueued.
void request_ray_cost(rt_ctx* c) {
    if (c->meas.snapPending) return;
    if (hipMemcpyAsync(c->snap, c->counterBuf.p, sizeof(DevCounters), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return;
    if (hipEventRecord(c->snapEvent, c->stream) != hipSuccess) return;
    c->meas.snapPending = true;
}
// What the measured statistics keep of the previous scene when a new one is uploaded (the stream is idle)
void measured_new_scene(rt_ctx* c) {
    if (c->meas.snapPending) { c->meas.snapBox = c->snap->boxTests; c->meas.snapRays = c->snap->raysTraced; c->meas.snapPending = false; }
    c->meas.boxPerRay = -1.0;  // a new scene: its ray cost is not known yet
}

// sum finished event pairs; the stream must be idle
int harvest_events(rt_ctx* c) {
    for (size_t i = 0; i < c->evUsed; i++) {
        float ms = 0.f;
        RT_HIP(c, hipEventElapsedTime(&ms, c->evPool[i].a, c->evPool[i].b));
        c->rep.traceMs += ms;
        c->rep.traceLaunches++;
        float t0 = 0.f;
        if (c->profBase && hipEventElapsedTime(&t0, c->profBase, c->evPool[i].a) == hipSuccess) c->rep.traceSpans.emplace_back(t0, t0 + ms);
    }
    c->evUsed = 0;
    return 0;
}

// The map flags, every object's alpha map and the emitter list of the light queries (scene_layout.h: layout_maps, layout_emitters).
// They follow the texture table, the materials, the spheres and the objects: called whenever one of the four is replaced.
int rebuild_emitters(rt_ctx* c) {
    c->sc.emitCount = 0; c->sc.emitSphereMask = 0; c->sc.emitMode = 0;
    const MapLayout maps = layout_maps(c->host, c->sc.texCount);
    int rc = upload_table(c, c->objAlphaBuf, maps.objAlpha, c->sc.objAlpha);
    if (rc) return rc;
    c->sc.mapFlags = maps.mapFlags;
    if (!c->tune.lightQueries) return 0;
    const EmitterLayout e = layout_emitters(c->host, c->rootOf, c->sc.texCount);
    if (!e.mode) return 0;
    if (!e.tris.empty()) {
        if ((rc = upload_table(c, c->emitBuf, e.tris, c->sc.emitTris))) return rc;
    } else {
        if ((rc = dev_alloc(c, c->emitBuf, 256))) return rc;
        c->sc.emitTris = (const uint2*)c->emitBuf.p;
    }
    // the ray-independent part of every listed triangle's test, computed on the device with the traversal's own operations
    if ((rc = dev_alloc(c, c->emitPreBuf, std::max<size_t>(e.tris.size(), 1) * 4 * sizeof(float4)))) return rc;
    if (!e.tris.empty()) {
        hipLaunchKernelGGL(k_emit_precompute, dim3(((uint32_t)e.tris.size() + 63u) / 64u), dim3(64), 0, c->stream, c->sc.triPos, c->sc.emitTris, (uint32_t)e.tris.size(), (float4*)c->emitPreBuf.p);
        RT_HIP(c, hipGetLastError());
        RT_HIP(c, hipStreamSynchronize(c->stream));  // set-up time; the renders may go to another stream later (rt_set_stream)
    }
    c->sc.emitPre = (const float4*)c->emitPreBuf.p;
    c->sc.emitCount = (uint32_t)e.tris.size();
    c->sc.emitSphereMask = e.sphereMask;
    c->sc.emitMode = 1;
    return 0;
}

// The tables that rt_upload_scene replaces after the meshes and the update entry points replace on their own. Their input has
// been checked by the time these run: only HIP can fail here.
int set_materials(rt_ctx* c, const RayMaterial* m, uint32_t n) {
    int rc = upload_table(c, c->matBuf, layout_materials(m, n), c->sc.mats);
    if (rc) return rc;
    c->sc.materialCount = n;
    c->host.mats.assign(m, m + n);
    return rebuild_emitters(c);
}

int set_spheres(rt_ctx* c, const Sphere* s, uint32_t n) {
    const SphereLayout l = layout_spheres(s, n);
    int rc = upload_table(c, c->sphereBuf, l.spheres, c->sc.spheres);
    if (rc) return rc;
    if ((rc = upload_table(c, c->sphereMatBuf, l.mat, c->sc.sphereMat))) return rc;
    c->sc.sphereCount = n;
    c->sc.sphereTestMask = l.testMask;
    c->host.sphereMat.assign(l.mat.begin(), l.mat.begin() + n);
    c->temporal.set_sphere_placements(l.spheres.data(), n);
    return rebuild_emitters(c);
}

int set_objects(rt_ctx* c, const ObjectLayout& l, const RenderObject* o, uint32_t n) {
    if (l.treeLevels && getenv("RT_DEBUG_OBJTREE")) dump_object_tree(l, n);
    int rc;
    if ((rc = upload_table(c, c->objInvBuf, l.inv, c->sc.objInv))) return rc;
    if ((rc = upload_table(c, c->objFwdBuf, l.fwd, c->sc.objFwd))) return rc;
    if ((rc = upload_table(c, c->objMetaBuf, l.meta, c->sc.objMeta))) return rc;
    if ((rc = upload_table(c, c->objBoxBuf, l.box, c->sc.objBox))) return rc;
    if ((rc = upload_table(c, c->maskBoxBuf, l.maskBox, c->sc.maskBox))) return rc;
    if ((rc = upload_table(c, c->objSkipBuf, l.skipCost, c->sc.objSkipCost))) return rc;
    if ((rc = upload_table(c, c->objTreeBuf, l.tree, c->sc.objTree))) return rc;
    if ((rc = upload_table(c, c->objCostBuf, l.cost, c->sc.objCost))) return rc;
    const std::vector<float4> nearTable = layout_nearest(l, o, n, c->rootOf);
    if ((rc = upload(c, c->objNearBuf, nearTable.data(), nearTable.size() * sizeof(float4)))) return rc;
    if (c->topo.on) {
        const std::vector<int32_t> orient = layout_orientation(o, n);
        if ((rc = upload(c, c->topo.orient, orient.data(), orient.size() * sizeof(int32_t)))) return rc;
        c->topo.counts.objects = n;
    }
    for (int k = 0; k <= RT_OBJTREE_LEVELS; k++) c->sc.objTreeOff[k] = l.treeOff[k];
    c->sc.objTreeLevels = l.treeLevels;
    c->sc.reachCount = l.reachCount;
    c->sc.maskBase = l.maskBase;
    c->sc.cullOriginLimit = l.cullOriginLimit;
    c->cull = l.cull;
    c->sc.objectCount = n;
    c->host.objMat.resize(n); c->host.objRoot.resize(n); c->host.objSampler.resize(n);
    for (uint32_t i = 0; i < n; i++) { c->host.objMat[i] = o[i].materialIndex; c->host.objRoot[i] = o[i].bvhIndex; c->host.objSampler[i] = o[i].samplerIndex; }
    if (o != c->hostObjects.data()) c->hostObjects.assign(o, o + n);
    c->temporal.set_object_placements(l.fwd.data(), l.inv.data(), c->host.objRoot.data(), n);
    return rebuild_emitters(c);
}

}  // namespace

extern "C" {

int rt_device_count(int* out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (out) *out = (e == hipSuccess) ? n : 0;
    return e == hipSuccess ? 0 : -1;
}

int rt_create(int device, rt_ctx** out) {
    if (!out) return -1;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -2;  // no GPU: fail loudly, no fallback
    if (device < 0 || device >= n) return -3;
    if (hipSetDevice(device) != hipSuccess) return -4;
    rt_ctx* c = new rt_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking) != hipSuccess) { c->ownStream = nullptr; rt_destroy(c); return -5; }
    c->stream = c->ownStream;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->numCUs = prop.multiProcessorCount;
    }
    // every failure below goes through rt_destroy, which releases whatever exists by then (stream, pinned buffers, event)
    if (hipHostMalloc((void**)&c->hostCounts, 64, hipHostMallocDefault) != hipSuccess) { c->hostCounts = nullptr; rt_destroy(c); return -6; }
    if (hipHostMalloc((void**)&c->snap, sizeof(DevCounters), hipHostMallocDefault) != hipSuccess) { c->snap = nullptr; rt_destroy(c); return -6; }
    if (hipEventCreateWithFlags(&c->snapEvent, hipEventDisableTiming) != hipSuccess) { c->snapEvent = nullptr; rt_destroy(c); return -6; }
    if (hipEventCreateWithFlags(&c->pollEvent, hipEventDisableTiming) != hipSuccess) { c->pollEvent = nullptr; rt_destroy(c); return -6; }
    if (dev_alloc(c, c->counterBuf, sizeof(DevCounters) + 256) != 0) { rt_destroy(c); return -7; }
    (void)hipMemsetAsync(c->counterBuf.p, 0, sizeof(DevCounters) + 256, c->stream);
    if (dev_alloc(c, c->aovCounterBuf, sizeof(DevCounters)) != 0) { rt_destroy(c); return -7; }
    (void)hipMemsetAsync(c->aovCounterBuf.p, 0, sizeof(DevCounters), c->stream);
    if (dev_alloc(c, c->shadeStatBuf, sizeof(ShadeStatStripe) * RT_STAT_STRIPES) != 0) { rt_destroy(c); return -7; }
    (void)hipMemsetAsync(c->shadeStatBuf.p, 0, sizeof(ShadeStatStripe) * RT_STAT_STRIPES, c->stream);
    (void)hipStreamSynchronize(c->stream);
    *out = c;
    return 0;
}

void rt_destroy(rt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)rt_comm_destroy(c);
    for (auto& e : c->evPool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (c->hostCounts) (void)hipHostFree(c->hostCounts);
    if (c->snap) (void)hipHostFree(c->snap);
    if (c->tpMotionHost) (void)hipHostFree(c->tpMotionHost);
    if (c->dyn.rootHost) (void)hipHostFree(c->dyn.rootHost);
    if (c->tpMotionEvent) (void)hipEventDestroy(c->tpMotionEvent);
    for (hipEvent_t e : {c->snapEvent, c->pollEvent, c->forkEvent, c->profBase})
        if (e) (void)hipEventDestroy(e);
    for (int l = 0; l < RT_MAX_LANES - 1; l++) {
        if (c->joinEvent[l]) (void)hipEventDestroy(c->joinEvent[l]);
        if (c->pollEventSide[l]) (void)hipEventDestroy(c->pollEventSide[l]);
        if (c->sideStream[l]) (void)hipStreamDestroy(c->sideStream[l]);
    }
    if (c->ownStream) (void)hipStreamDestroy(c->ownStream);
    delete c;  // every DevBuf frees itself
}

const char* rt_last_error(const rt_ctx* c) { return c ? c->error.c_str() : "null ctx"; }

int rt_set_stream(rt_ctx* c, void* s) {
    if (!c) return -1;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->ownStream;
    return 0;
}

// The entry points that replace scene tables: check the arguments, derive the tables on the host (scene_layout.h), upload.
// Nothing of the context is written before the layout has succeeded, so a refused input leaves it as it was.
int rt_upload_textures(rt_ctx* c, const RtTexture* tex, uint32_t n) {
    if (!c || (!tex && n)) return -1;
    const TextureLayout l = layout_textures(tex, n);
    if (!l.error.empty()) return c->fail(l.error);
    RT_HIP(c, hipSetDevice(c->device));
    int rc = upload_table(c, c->texelBuf, l.texels, c->sc.texels);
    if (rc) return rc;
    if ((rc = upload_table(c, c->texInfoBuf, l.info, c->sc.texInfo))) return rc;
    c->sc.texCount = n;
    return rebuild_emitters(c);   // (which maps are bound follows the table's size; an emitter with an alpha map leaves the emitter list)
}

int rt_update_materials(rt_ctx* c, const RayMaterial* m, uint32_t n) {
    if (!c || (!m && n)) return -1;
    RT_HIP(c, hipSetDevice(c->device));
    return set_materials(c, m, n);
}

int rt_update_spheres(rt_ctx* c, const Sphere* s, uint32_t n) {
    if (!c || (!s && n)) return -1;
    RT_HIP(c, hipSetDevice(c->device));
    return set_spheres(c, s, n);
}

int rt_update_objects(rt_ctx* c, const RenderObject* o, uint32_t n) {
    if (!c || (!o && n)) return -1;
    if (c->rootOf.empty() && n) return c->fail("rt_update_objects before rt_upload_scene");
    const ObjectLayout l = layout_objects(o, n, c->rootOf, c->sc.materialCount, c->tune.objTreeMin, c->tune.maskIdentity);
    if (!l.error.empty()) return c->fail(l.error);
    RT_HIP(c, hipSetDevice(c->device));
    return set_objects(c, l, o, n);
}

}  // extern "C"

namespace {

void release_dynamic(rt_ctx* c) {
    rt_ctx::Dynamic& d = c->dyn;
    if (d.rootHost) (void)hipHostFree(d.rootHost);
    d.rootHost = nullptr;
    d.on = false;
    d.plan = RefitPlan{};
    for (DevBuf* b : {&d.points, &d.triIdx, &d.leaves, &d.interior, &d.levels}) b->release();
}

// What rt_upload_scene_dynamic keeps beside the scene tables. The stream is idle when it returns.
int keep_dynamic(rt_ctx* c, const RtSceneArrays& s, RefitPlan&& plan) {
    rt_ctx::Dynamic& d = c->dyn;
    std::vector<uint4> triIdx(std::max(s.triangleCount, 1u), make_uint4(0u, 0u, 0u, 0u));
    for (uint32_t t = 0; t < s.triangleCount; t++) triIdx[t] = make_uint4(s.triangles[t].v0, s.triangles[t].v1, s.triangles[t].v2, s.triangles[t].frontOnly);
    int rc;
    if ((rc = upload(c, d.points, s.triPoints, (size_t)s.triPointCount * sizeof(TrianglePoint)))) return rc;
    if ((rc = upload(c, d.triIdx, triIdx.data(), triIdx.size() * sizeof(uint4)))) return rc;
    if ((rc = upload(c, d.leaves, plan.leaves.data(), plan.leaves.size() * sizeof(uint32_t)))) return rc;
    if ((rc = upload(c, d.interior, plan.interior.data(), plan.interior.size() * sizeof(uint32_t)))) return rc;
    if ((rc = upload(c, d.levels, plan.levels.data(), plan.levels.size() * sizeof(uint32_t)))) return rc;
    RT_HIP(c, hipHostMalloc((void**)&d.rootHost, std::max<size_t>(plan.meshes.size(), 1) * 2 * sizeof(float4), hipHostMallocDefault));
    d.plan = std::move(plan);
    d.on = true;
    return 0;
}

int upload_scene(rt_ctx* c, const RtSceneArrays* s, bool dynamic) {
    if (!c || !s) return -1;
    SceneLayout l = layout_scene(*s, c->tune.objTreeMin, c->tune.maskIdentity);
    if (!l.error.empty()) return c->fail(l.error);
    MeshLayout& m = l.meshes;
    RefitPlan plan;
    if (dynamic) {
        plan = plan_refit(*s, m);
        if (!plan.error.empty()) return c->fail("rt_upload_scene_dynamic: " + plan.error);
    }

    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    measured_new_scene(c);
    c->temporal.reset();  // a new scene: nothing of the old one's frames is its history (rt_temporal_accumulate)
    c->host = SceneSources{};
    c->sc.emitMode = 0; c->sc.emitCount = 0; c->sc.emitSphereMask = 0;
    c->sc.mapFlags = 0;
    c->sc.texCount = 0;  // texture slots belong to the scene's materials: rt_upload_textures follows a new scene
    release_dynamic(c);
    c->topo.on = false;   // the table belongs to the scene it was made for: rt_upload_topology follows a new scene
    c->topo.rows.release(); c->topo.orient.release();
    c->sceneBufs.clear();
    c->sceneBufs.resize(5);
    int rc;
    if ((rc = upload_table(c, c->triUVBuf, m.triUV, c->sc.triUV))) return rc;
    if ((rc = upload_table(c, c->sceneBufs[0], m.nodes, c->sc.nodes))) return rc;
    if ((rc = upload_table(c, c->sceneBufs[1], m.triPos, c->sc.triPos))) return rc;
    if ((rc = upload_table(c, c->sceneBufs[2], m.triNrm, c->sc.triNrm))) return rc;
    if ((rc = upload_table(c, c->sceneBufs[3], m.leafFirst, c->sc.leafFirst))) return rc;
    if ((rc = upload_table(c, c->sceneBufs[4], m.nodesPk, c->sc.nodesPk))) return rc;
    c->sc.nodeCount = m.nodeCount;
    c->sc.triCount = s->triangleCount;
    c->sc.hotNodes = m.hotNodes;
    c->maxLeafDepth = m.maxLeafDepth;
    c->rootOf = std::move(m.rootOf);

    if ((rc = set_materials(c, s->materials, s->materialCount))) return rc;
    if ((rc = set_spheres(c, s->spheres, s->sphereCount))) return rc;
    if ((rc = set_objects(c, l.objects, s->objects, s->objectCount))) return rc;
    return dynamic ? keep_dynamic(c, *s, std::move(plan)) : 0;
}

// The refit of one mesh, enqueued on the ctx stream: gather, leaves, levels deepest first, pack (rt_refit.hip.h), and the root's
// new box on its way to rootHost[2 * slot]. Every index the kernels read comes from the plan, which was checked against the
// tables' sizes when the scene was uploaded.
int enqueue_refit(rt_ctx* c, const RefitMesh& m, uint32_t slot) {
    const rt_ctx::Dynamic& d = c->dyn;
    float4 *nodes = (float4*)c->sc.nodes, *nodesPk = (float4*)c->sc.nodesPk;
    const uint32_t* leaves = (const uint32_t*)d.leaves.p + m.leafOff;
    const uint32_t* interior = (const uint32_t*)d.interior.p + m.interiorOff;
    const uint32_t* levelsDev = (const uint32_t*)d.levels.p + m.levelOff;
    const uint32_t* levels = d.plan.levels.data() + m.levelOff;
    auto blocks = [](uint32_t n, uint32_t per) { return dim3((n + per - 1) / per); };
    if (m.triCount)
        hipLaunchKernelGGL(k_refit_gather, blocks(m.triCount, 256), dim3(256), 0, c->stream, (const uint4*)d.triIdx.p, (const float4*)d.points.p, m.triFirst,
                           m.triCount, (float4*)c->sc.triPos, (float4*)c->sc.triNrm, (float4*)c->sc.triUV);
    if (m.inlineLeaves)
        hipLaunchKernelGGL(k_refit_leaves_inline, blocks(m.inlineLeaves, 256), dim3(256), 0, c->stream, leaves, m.inlineLeaves, c->sc.triPos, nodes);
    if (m.bigLeaves)
        hipLaunchKernelGGL(k_refit_leaves_big, blocks(m.bigLeaves, 4), dim3(256), 0, c->stream, leaves + m.inlineLeaves, m.bigLeaves, c->sc.leafFirst,
                           c->sc.triPos, nodes);
    // the levels towards the root that one block covers in one pass each (at most 256 nodes) go into one launch: measured, 0.187
    // against 0.230 ms per call on Cornell + bunny and 2.19 against 2.74 ms on the Sponza stand-in ("Deforming meshes")
    uint32_t fold = m.levelCount;
    while (fold > 0 && levels[fold] - levels[fold - 1] <= 256u) fold--;
    if (m.levelCount - fold < 2u) fold = m.levelCount;
    for (uint32_t l = 0; l < fold; l++) {
        const uint32_t n = levels[l + 1] - levels[l];
        hipLaunchKernelGGL(k_refit_level, blocks(n, 256), dim3(256), 0, c->stream, interior + levels[l], n, nodes);
    }
    if (fold < m.levelCount) hipLaunchKernelGGL(k_refit_top, dim3(1), dim3(256), 0, c->stream, interior, levelsDev + fold, m.levelCount - fold, nodes);
    hipLaunchKernelGGL(k_refit_pack, blocks(m.interiorCount + 1, 256), dim3(256), 0, c->stream, interior, m.interiorCount, m.rootDev, c->sc.nodeCount,
                       (const float4*)nodes, nodesPk);
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipMemcpyAsync(d.rootHost + 2 * (size_t)slot, nodes + 2 * (size_t)m.rootDev, 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

}  // namespace

extern "C" {

int rt_upload_scene(rt_ctx* c, const RtSceneArrays* s) { return upload_scene(c, s, false); }

int rt_upload_scene_dynamic(rt_ctx* c, const RtSceneArrays* s) { return upload_scene(c, s, true); }

int rt_update_points(rt_ctx* c, const TrianglePoint* points, uint32_t first, uint32_t count) {
    if (!c) return -1;
    if (!c->dyn.on) return c->fail("rt_update_points: the scene was not uploaded with rt_upload_scene_dynamic");
    const RefitPlan& plan = c->dyn.plan;
    const std::string refused = check_update_points("rt_update_points", plan.pointCount, points, first, count);
    if (!refused.empty()) return c->fail(refused);
    if (count == 0) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    const std::vector<uint32_t> touched = touched_meshes(plan.meshes, first, count);
    RT_HIP(c, hipMemcpyAsync((TrianglePoint*)c->dyn.points.p + first, points, (size_t)count * sizeof(TrianglePoint), hipMemcpyHostToDevice, c->stream));
    int rc;
    for (size_t k = 0; k < touched.size(); k++)
        if ((rc = enqueue_refit(c, plan.meshes[touched[k]], (uint32_t)k))) return rc;
    RT_HIP(c, hipStreamSynchronize(c->stream));   // one wait for the refit and its read-back: `points` is borrowed for the call, and the roots' boxes have arrived
    if (touched.empty()) return 0;
    // the object tables follow the roots' boxes (padded world boxes, mask boxes, the object hierarchy, cullOriginLimit) and the
    // emitter list's precomputed triangles follow triPos: both through rt_update_objects' own synchronous path (set_objects waits
    // after each of its tables)
    std::vector<uint32_t> roots;
    for (size_t k = 0; k < touched.size(); k++) {
        const RefitMesh& m = plan.meshes[touched[k]];
        const float4 lo = c->dyn.rootHost[2 * k], hi = c->dyn.rootHost[2 * k + 1];
        RootInfo& r = c->rootOf[m.root];
        r.lo[0] = lo.x; r.lo[1] = lo.y; r.lo[2] = lo.z;
        r.hi[0] = hi.x; r.hi[1] = hi.y; r.hi[2] = hi.z;
        roots.push_back(m.root);
    }
    const uint32_t n = (uint32_t)c->hostObjects.size();
    const ObjectLayout l = layout_objects(c->hostObjects.data(), n, c->rootOf, c->sc.materialCount, c->tune.objTreeMin, c->tune.maskIdentity);
    if (!l.error.empty()) return c->fail(l.error);
    if ((rc = set_objects(c, l, c->hostObjects.data(), n))) return rc;
    c->temporal.meshes_refit(roots.data(), (uint32_t)roots.size());   // their objects have no history in the next rt_temporal_accumulate
    return 0;
}

int rt_sync(rt_ctx* c) {
    if (!c) return -1;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return harvest_events(c);
}

}  // extern "C"

namespace {
// The checks rt_render, rt_render_aovs and rt_render_guides share (post_passes.h: check_tile)
UploadedScene uploaded_scene(const rt_ctx* c) { return UploadedScene{c->sc.nodes != nullptr, c->sc.sphereCount, c->sc.objectCount}; }
int check_tile(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride, uint32_t nRows,
               const char* fn) {
    const std::string e = check_tile(fn, pc->rayTraceParams, width, height, row0, rowStride, nRows, uploaded_scene(c));
    return e.empty() ? 0 : c->fail(e);
}

// The scene of a dispatch: the uploaded one with the counts of rayTraceParams
DevScene dispatch_scene(const rt_ctx* c, const RayTracerData& td) {
    DevScene sc = c->sc;
    sc.sphereCount = td.sphereCount;
    sc.objectCount = td.objectCount;
    if (sc.objectCount < c->sc.objectCount) { sc.reachCount = 0; sc.objTreeLevels = 0; }  // a dispatch with fewer objects than were uploaded: no masks, no object hierarchy
    return sc;
}

// The camera and tile of a dispatch (post_passes.h: camera_plane)
FrameParams frame_camera(const rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                         uint32_t nRows, uint32_t nPixels) {
    FrameParams fp{};
    const CameraPlane plane = camera_plane(pc->camInfo);
    memcpy(fp.camRot, pc->camInfo.cameraRotation, 64);
    memcpy(fp.camPos, pc->camInfo.pos, 12);
    fp.planeHeight = plane.planeHeight;
    fp.planeWidth = plane.planeWidth;
    memcpy(fp.bottomLeft, plane.bottomLeft, 12);
    fp.tiled = (c->tune.tileSlots && (width % 8u) == 0u) ? 1u : 0u;
    fp.width = width; fp.height = height; fp.row0 = row0; fp.rowStride = rowStride; fp.nRows = nRows; fp.nPixels = nPixels;
    return fp;
}

// The side streams and events of parts 1..nLanes-1, made when first needed; returns the parts there are streams for
int ensure_part_streams(rt_ctx* c, int nLanes) {
    for (int l = 1; l < nLanes; l++) {
        if (!c->sideStream[l - 1]) {
            if (hipStreamCreateWithFlags(&c->sideStream[l - 1], hipStreamNonBlocking) != hipSuccess) { c->sideStream[l - 1] = nullptr; nLanes = l; break; }
            if (hipEventCreateWithFlags(&c->joinEvent[l - 1], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->pollEventSide[l - 1], hipEventDisableTiming) != hipSuccess) { nLanes = l; break; }
        }
    }
    if (nLanes > 1 && !c->forkEvent && hipEventCreateWithFlags(&c->forkEvent, hipEventDisableTiming) != hipSuccess) { c->forkEvent = nullptr; nLanes = 1; }
    return nLanes;
}

// One part of a multi-kernel dispatch: what its launches are built with (d), its slots [begin, begin + n) and the state of its rounds
struct Lane { Dispatch d; hipEvent_t poll; uint32_t begin, n, ubActive; int cur; bool pollPending, done; };
// The parts of a dispatch as the plan slices it, each with its stream, counter block and poll event
void make_parts(rt_ctx* c, const Dispatch& d, const PartSlices& p, uint32_t nSlots, int nLanes, Lane* lane) {
    for (int l = 0; l < nLanes; l++) {
        lane[l] = Lane{d, l ? c->pollEventSide[l - 1] : c->pollEvent, p.begin[l], p.n[l], p.n[l], 0, false, p.n[l] == 0};
        lane[l].d.stream = l ? c->sideStream[l - 1] : c->stream; lane[l].d.counts = c->q.counts + 16 * l; lane[l].d.part = l;
        lane[l].d.gridPct = p.gridPct;
        lane[l].d.slots = nSlots;
    }
}

// What the rounds shade with and count into. A dispatch of pixels: k_shade / k_shade_maps and the rendering counters. A radiance
// query (origins != nullptr): k_shade_rays / k_shade_rays_maps, which restart a sample from the caller's origins (`first`: the ray in
// slot 0), and the AOV passes' counter block, which the ray-cost measurement never reads.
struct ShadePass { DevCounters* counters; const float* origins; uint32_t first; };
ShadePass pixel_shading(rt_ctx* c) { return ShadePass{(DevCounters*)c->counterBuf.p, nullptr, 0u}; }
void launch_shade(const ShadePass& sp, uint32_t blocks, hipStream_t stream, const DevScene& sc, const PathState& ps, const ShadeArgs& sa, const FrameParams& fp) {
    const bool maps = (sc.mapFlags & (RT_MAP_METALNESS | RT_MAP_BUMP)) != 0;
    if (sp.origins) {
        if (maps) hipLaunchKernelGGL(k_shade_rays_maps, dim3(blocks), dim3(RT_BLOCK), 0, stream, sc, ps, sa, fp, sp.origins, sp.first);
        else hipLaunchKernelGGL(k_shade_rays, dim3(blocks), dim3(RT_BLOCK), 0, stream, sc, ps, sa, fp, sp.origins, sp.first);
    } else {
        if (maps) hipLaunchKernelGGL(k_shade_maps, dim3(blocks), dim3(RT_BLOCK), 0, stream, sc, ps, sa, fp);
        else hipLaunchKernelGGL(k_shade, dim3(blocks), dim3(RT_BLOCK), 0, stream, sc, ps, sa, fp);
    }
}

// The rounds of the multi-kernel pipeline: the parts fork from the ctx stream, each runs traversal, then shading, until none of its
// paths is active, and they join it again
int render_rounds(rt_ctx* c, const FrameParams& fp, Lane* lane, int nLanes, const ShadePass& sp) {
    DevCounters* dc = sp.counters;
    int rc = 0;
    if (nLanes > 1) {
        RT_HIP(c, hipEventRecord(c->forkEvent, c->stream));
        for (int l = 1; l < nLanes; l++) RT_HIP(c, hipStreamWaitEvent(lane[l].d.stream, c->forkEvent, 0));
    }
    // The whole dispatch is enqueued without waiting for the device (rt_amd.h: "asynchronous on the ctx stream"): every
    // kernel reads its queue length from device memory and leaves at once when the queue is empty, so the loop may
    // simply run to the most rounds a pixel can need, samples * (bounceLimit + 1). The active-path count is copied
    // back now and then without ever being waited for; a copy that has arrived shrinks the grids of the launches still
    // to be enqueued (active paths never increase, so a stale count is a valid upper bound) and ends the part at zero.
    const uint64_t maxRounds = (uint64_t)fp.samples * ((uint64_t)fp.bounceLimit + 1);
    for (uint64_t it = 0; it < maxRounds; it++) {
        bool any = false;
        for (int l = 0; l < nLanes; l++) {
            Lane& L = lane[l];
            if (L.done) continue;
            any = true;
            const hipStream_t stream = L.d.stream; uint32_t* const counts = L.d.counts;
            const int cur = L.cur, nxt = cur ^ 1;
            uint32_t* const active[2] = {c->q.active[0] + L.begin, c->q.active[1] + L.begin};
            uint32_t* const rays[2] = {c->q.rays[0] + 3 * (size_t)L.begin, c->q.rays[1] + 3 * (size_t)L.begin};
            hipLaunchKernelGGL(k_zero_counts, dim3(1), dim3(64), 0, stream, counts + nxt, counts + 2 + nxt, counts + 4, counts + 5 + nxt, counts + 7 + nxt);
            TraceArgs ta{rays[cur], counts + 2 + cur, nullptr, nullptr, dc, counts + 5 + cur, counts + 7 + cur, L.n};
            const uint64_t ubRays = std::min<uint64_t>((uint64_t)L.ubActive * 3, (uint64_t)L.n * 3);
            if ((rc = launch_trace(c, L.d, (uint32_t)ubRays, ta, sp.origins != nullptr))) break;   // (a radiance query: the persistent-wave kernels whatever "trace_variant" says, as the ray queries)
            ShadeArgs sa{active[cur], counts + cur, active[nxt], rays[nxt], counts + nxt, counts + 2 + nxt, (ShadeStatStripe*)c->shadeStatBuf.p, counts + 5 + nxt, counts + 7 + nxt, L.n};
            launch_shade(sp, (L.ubActive + RT_BLOCK - 1) / RT_BLOCK, stream, L.d.sc, c->ps, sa, fp);
            L.cur = nxt;
            if (L.pollPending && hipEventQuery(L.poll) == hipSuccess) {
                L.pollPending = false;
                L.ubActive = std::min(L.ubActive, c->hostCounts[8 + l]);
                if (L.ubActive == 0) { L.done = true; continue; }
            }
            if (!L.pollPending && (it & 7u) == 7u) {
                if (hipMemcpyAsync(c->hostCounts + 8 + l, counts + L.cur, 4, hipMemcpyDeviceToHost, stream) == hipSuccess &&
                    hipEventRecord(L.poll, stream) == hipSuccess)
                    L.pollPending = true;
            }
        }
        if (!any || rc) break;
    }
    // (a copy still in flight when the loop ends is harmless: the stream orders it before the next dispatch's own
    // copies, and the slot is only read after the event of the copy that filled it)
    for (int l = 1; l < nLanes; l++) {  // (also when a launch failed: nothing of this dispatch is left running beside the ctx stream)
        RT_HIP(c, hipEventRecord(c->joinEvent[l - 1], lane[l].d.stream));
        RT_HIP(c, hipStreamWaitEvent(c->stream, c->joinEvent[l - 1], 0));
    }
    // all parts are back on the ctx stream: their k_shade launches' statistics into the counters (also after a failed launch)
    hipLaunchKernelGGL(k_fold_shade_stats, dim3(1), dim3(RT_STAT_STRIPES), 0, c->stream, (ShadeStatStripe*)c->shadeStatBuf.p, dc);
    return rc;
}

// The multi-kernel pipeline: the dispatch in `nLanes` independent parts: contiguous slot ranges (whole 256-slot blocks of all the frames of a tile
// block), each with its own region of the queues, its own counters and its own stream. A pixel's path depends on nothing but
// its slot, so the parts give the same bits as the whole; what they buy is overlap: one part's k_shade (bound by the path
// state it streams) and the draining tail of its k_trace_pw launch run under the other part's traversal (bound by latency).
// Part 0 runs on the ctx stream, the others fork from it after the ray generation and join it before the image is written.
int render_parts(rt_ctx* c, const FrameParams& fp, const Dispatch& d, uint32_t nSlots, float4* fb) {
    const int nLanes = ensure_part_streams(c, choose_parts(c->tune, c->meas, scene_facts(c, d), dispatch_facts(d, &fp, false)));
    c->rep.lastParts = nLanes;
    Lane lane[RT_MAX_LANES];
    make_parts(c, d, slice_parts(c->tune, nSlots, fp.nFrames, nLanes), nSlots, nLanes, lane);
    for (int l = 0; l < nLanes; l++) {
        const Lane& L = lane[l];
        if (!L.n) continue;
        hipLaunchKernelGGL(k_raygen, dim3((L.n + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps,
                           c->q.active[0] + L.begin, c->q.rays[0] + 3 * (size_t)L.begin, fp, L.begin, L.begin + L.n);
        // counts: [0],[1] active paths of buffer 0/1; [2],[3] main rays of buffer 0/1; [4] the traversal's work counter; [5],[6] NEE rays, [7],[8] cosine probes of buffer 0/1
        if (fp.samples > 0) hipLaunchKernelGGL(k_init_counts, dim3(1), dim3(64), 0, c->stream, L.d.counts, L.n);
    }
    RT_HIP(c, hipGetLastError());
    if (fp.samples > 0)
        if (int rc = render_rounds(c, fp, lane, nLanes, pixel_shading(c))) return rc;
    const uint32_t blocksPix = (fp.nPixels + RT_BLOCK - 1) / RT_BLOCK;
    if (fp.nFrames > 1u) hipLaunchKernelGGL(k_blend_frames, dim3(blocksPix), dim3(RT_BLOCK), 0, c->stream, c->ps, fp, fb);
    else hipLaunchKernelGGL(k_resolve, dim3(blocksPix), dim3(RT_BLOCK), 0, c->stream, c->ps, fp, fb);
    RT_HIP(c, hipGetLastError());
    return 0;
}

int probe_ray_cost(rt_ctx* c, const FrameParams& fp, const Dispatch& d);

// A dispatch whose arguments are checked and whose path state and image exist: measure, choose, launch
int render_dispatch(rt_ctx* c, const FrameParams& fp, const Dispatch& d, float4* fb) {
    const uint32_t nSlots = (uint32_t)dispatch_slots(fp.nPixels, fp.nFrames);
    int rc;
    poll_ray_cost(c);
    const SceneFacts sf = scene_facts(c, d);
    const DispatchFacts df = dispatch_facts(d, &fp, false);
    if (probe_first(c->tune, c->meas, sf, df) && (rc = probe_ray_cost(c, fp, d))) return rc;
    const int pipeline = choose_pipeline(c->tune, c->meas, sf, df);
    if (!d.probe) c->rep.lastPipeline = pipeline;
    if (pipeline == 1) {  // wave-private fused pipeline: one launch for the whole dispatch
        rc = launch_fused(c, d, fp, fb);
        if (!rc && fp.nFrames > 1u) {
            hipLaunchKernelGGL(k_blend_frames, dim3((fp.nPixels + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, c->ps, fp, fb);
            rc = c->hip(hipGetLastError(), "k_blend_frames");
        }
    } else {
        rc = render_parts(c, fp, d, nSlots, fb);
    }
    if (!rc) request_ray_cost(c);
    return rc;
}

// The ray-cost probe (launch_plan.h: probe_first, probe_rows): a few rows of the same tile, rendered once with one sample per
// pixel into a scratch image, and the counters put back.
// (fp, d: the big dispatch's. The probe's path state fits in its, and its scene counts are the same.)
int probe_ray_cost(rt_ctx* c, const FrameParams& fp, const Dispatch& d) {
    const TileRows rows = probe_rows(TileRows{fp.row0, fp.rowStride, fp.nRows});
    FrameParams p = fp;
    p.samples = 1; p.progressive = 0; p.debug = -1; p.nFrames = 1;
    p.sampleMap = nullptr;  // (rt_render_sampled's map covers the big dispatch's rows, not these)
    p.row0 = rows.row0; p.rowStride = rows.rowStride; p.nRows = rows.nRows; p.nPixels = rows.nRows * fp.width;
    Dispatch pd = d;  // fused pipeline, no profiling, no phase statistics, launches not counted
    pd.probe = true; pd.pipeline = 1; pd.profiled = false; pd.phaseStats = 0; pd.launches = nullptr;
    int rc = dev_alloc(c, c->probeBuf, (size_t)p.nPixels * sizeof(float4));
    if (rc) return rc;
    DevCounters before, after;
    RT_HIP(c, hipMemcpyAsync(&before, c->counterBuf.p, sizeof(DevCounters), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = render_dispatch(c, p, pd, (float4*)c->probeBuf.p))) return rc;
    RT_HIP(c, hipMemcpyAsync(&after, c->counterBuf.p, sizeof(DevCounters), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    RT_HIP(c, hipMemcpyAsync(c->counterBuf.p, &before, sizeof(DevCounters), hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->meas.snapPending = false;  // the probe's own snapshot request: its copy has arrived, and it is not wanted
    fold_probe(c->meas, ray_counters(before), ray_counters(after));
    return 0;
}

// rt_render (nFrames = 1), rt_render_frames and rt_render_sampled (sampleMap): the checks, the path state and the image, then render_dispatch
int render_impl(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                uint32_t nRows, uint32_t nFrames, const uint32_t* sampleMap, float* d_rgba) {
    if (!c || !pc) return -1;
    int rc = check_tile(c, pc, width, height, row0, rowStride, nRows, "rt_render");
    if (rc) return rc;
    const RayTracerData& td = pc->rayTraceParams;
    const std::string refused = check_sampled(td, sampleMap != nullptr);
    if (!refused.empty()) return c->fail(refused);
    if (td.bounceLimit >= (1u << 28) - 1u) return c->fail("rayTraceParams.bounceLimit needs more than 28 bits");
    const uint64_t np64 = (uint64_t)nRows * width;
    if (frame_slots(np64) * nFrames >= (1ull << 30)) return c->fail("tile too large (slot ids are 30 bits)");
    const uint32_t nPixels = (uint32_t)np64;
    RT_HIP(c, hipSetDevice(c->device));
    if (nPixels == 0) return 0;

    rc = ensure_state(c, (uint32_t)dispatch_slots(nPixels, nFrames));
    if (rc) return rc;
    float4* fb = (float4*)d_rgba;
    if (!fb) {
        const bool fresh = !c->fb.buf.p || c->fb.pixels != nPixels;
        if ((rc = dev_alloc(c, c->fb.buf, (size_t)nPixels * sizeof(float4)))) return rc;
        if (fresh) RT_HIP(c, hipMemsetAsync(c->fb.buf.p, 0, (size_t)nPixels * sizeof(float4), c->stream));
        c->fb.pixels = nPixels;
        fb = (float4*)c->fb.buf.p;
        c->fb.valid = true;
        c->fb.rows = RowsOf{width, height, row0, rowStride, nRows};
    }

    // ---- per-frame constants (host side of raytrace.comp:547-564)
    FrameParams fp = frame_camera(c, pc, width, height, row0, rowStride, nRows, nPixels);
    uint32_t lol = pc->frameCount;
    fp.startingSeed = (uint32_t)(rt_random(&lol) * 23892183.f);
    fp.samples = td.singleRender ? td.sampleLimit : td.raysPerPixel;
    fp.bounceLimit = td.bounceLimit;
    fp.progressive = td.progressive;
    fp.frameCount = pc->frameCount;
    fp.nFrames = nFrames;
    fp.camReuse = (c->tune.cameraReuse && td.debug < 0) ? 1u : 0u;
    fp.debug = td.debug;
    fp.boxCap = td.boxCap;
    fp.triCap = td.triangleCap;
    fp.env = pc->environment;
    fp.sampleMap = sampleMap;
    return render_dispatch(c, fp, one_part(c, dispatch_scene(c, td), td.debug >= 0), fb);
}

// How the side passes begin: the first-hit AOVs, the guides, the ray queries with the AO plane, the radiance queries. A pass's rays
// live in path-state slots [0, nSlots) and its ray count in the first part's counters: the ctx stream orders it after a dispatch
// still in flight (whose parts join the ctx stream before it ends). Growing the path state frees the old one, so that waits for
// the device first. The pass runs on `sc` in one part, with no per-pixel statistics and no phase statistics, and its traversal
// launches are counted apart, in rep.aovLaunches.
int side_pass_begin(rt_ctx* c, uint32_t nSlots, const DevScene& sc, Dispatch* d) {
    RT_HIP(c, hipSetDevice(c->device));
    if (c->capacity < nSlots || !c->stateBuf.p) RT_HIP(c, hipStreamSynchronize(c->stream));
    int rc = ensure_state(c, nSlots);
    if (rc) return rc;
    *d = one_part(c, sc, false);
    d->phaseStats = 0; d->launches = &c->rep.aovLaunches;
    return 0;
}

// The ctx-owned set of five planes (in AovPlane's order) for a pass that was given none: nPixels pixels of these rows
int claim_planes(rt_ctx* c, OwnedPlane& own, uint32_t nPixels, const RowsOf& rows) {
    int rc = dev_alloc(c, own.buf, (size_t)nPixels * sizeof(float4) * AOV_PLANES);
    if (rc) return rc;
    own.pixels = nPixels;
    own.valid = true;
    own.rows = rows;
    return 0;
}
AovOut aov_out(const RtAovBuffers* given, const void* owned, size_t nPixels) {   // given NULL: the ctx-owned set; both NULL: no plane
    const auto plane = [&](AovPlane k) -> void* { return given ? aov_plane(*given, k) : owned ? aov_plane(owned, k, nPixels) : nullptr; };
    return AovOut{(float4*)plane(AOV_NORMAL_DEPTH), (float4*)plane(AOV_POSITION), (float4*)plane(AOV_ALBEDO), (float4*)plane(AOV_RAY_DIR), (uint4*)plane(AOV_IDS)};
}
}  // namespace

extern "C" {

int rt_render(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
              uint32_t nRows, float* d_rgba) {
    return render_impl(c, pc, width, height, row0, rowStride, nRows, 1u, nullptr, d_rgba);
}

int rt_render_frames(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                     uint32_t nRows, uint32_t nFrames, float* d_rgba) {
    return rt_render_sampled(c, pc, width, height, row0, rowStride, nRows, nFrames, nullptr, d_rgba);
}

// (d_sampleMap NULL is rt_render_frames: the map is one more frame constant, and without it every kernel takes the uniform count)
int rt_render_sampled(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                      uint32_t nRows, uint32_t nFrames, const uint32_t* d_sampleMap, float* d_rgba) {
    if (!c || !pc) return -1;
    if (nFrames == 0) return 0;
    // The frames of one call are one dispatch, or several when they are too many paths for one (launch_plan.h: frames_per_dispatch)
    const uint32_t per = frames_per_dispatch(c->tune, (uint64_t)nRows * width, nFrames, pc->rayTraceParams.debug);
    PushConstants p = *pc;
    for (uint32_t f = 0; f < nFrames; f += per) {
        const uint32_t n = std::min(per, nFrames - f);
        p.frameCount = pc->frameCount + f;
        int rc = render_impl(c, &p, width, height, row0, rowStride, nRows, n, d_sampleMap, d_rgba);
        if (rc) return rc;
    }
    return 0;
}

int rt_clear_framebuffer(rt_ctx* c) {
    if (!c) return -1;
    c->fb.pixels = 0;  // the next rt_render(..., NULL) starts from a zeroed image
    c->fb.valid = false;
    return 0;
}

int rt_read_rgba_f32(rt_ctx* c, float* out, size_t nFloats) {
    return read_plane(c, c ? &c->fb : nullptr, "rt_read_rgba_f32", NO_OWNED_FRAMEBUFFER, out, nFloats);
}

int rt_read_rgba8_srgb(rt_ctx* c, uint8_t* out, size_t nBytes) {
    if (!c || !out) return -1;
    if (!c->fb.valid || nBytes != c->fb.pixels * 4) return c->fail("rt_read_rgba8_srgb: size mismatch");
    std::vector<float> tmp(c->fb.pixels * 4);
    int rc = rt_read_rgba_f32(c, tmp.data(), tmp.size());
    if (rc) return rc;
    // display encoding only; parity is defined on the fp32 buffer
    for (size_t i = 0; i < tmp.size(); i++) {
        float v = tmp[i];
        if (!(v > 0.f)) v = 0.f;
        if (v > 1.f) v = 1.f;
        if ((i & 3) != 3) v = v <= 0.0031308f ? 12.92f * v : 1.055f * rt_pow(v, 1.f / 2.4f) - 0.055f;
        out[i] = (uint8_t)(v * 255.f + 0.5f);
    }
    return 0;
}

int rt_trace_rays(rt_ctx* c, uint32_t n, const float* origins, const float* dirs, RtHit* hitsOut) {
    if (!c || !origins || !dirs || !hitsOut) return -1;
    if (!c->sc.nodes) return c->fail("rt_trace_rays before rt_upload_scene");
    if (n == 0) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    int rc = ensure_state(c, n);
    if (rc) return rc;
    std::vector<float4> ho(n), hd(n);
    for (uint32_t i = 0; i < n; i++) {
        ho[i] = make_float4(origins[(size_t)i * 3], origins[(size_t)i * 3 + 1], origins[(size_t)i * 3 + 2], 0.f);
        hd[i] = make_float4(dirs[(size_t)i * 3], dirs[(size_t)i * 3 + 1], dirs[(size_t)i * 3 + 2], 0.f);
    }
    RT_HIP(c, hipMemcpyAsync(c->ps.rayO(), ho.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync(c->ps.rayD(), hd.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    size_t need = (size_t)n * 8 + (size_t)n * sizeof(RtHit) + 256;
    if ((rc = dev_alloc(c, c->scratchBuf, need))) return rc;
    uint32_t* prb = (uint32_t*)c->scratchBuf.p;
    uint32_t* prt = prb + n;
    RtHit* dh = (RtHit*)((char*)c->scratchBuf.p + (((size_t)n * 8 + 255) & ~(size_t)255));
    c->hostCounts[0] = n; c->hostCounts[1] = 0; c->hostCounts[2] = 0; c->hostCounts[3] = 0; c->hostCounts[4] = 0;
    RT_HIP(c, hipMemcpyAsync(c->q.counts, c->hostCounts, 20, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipMemsetAsync(c->ps.statBox(), 0, (size_t)n * 4, c->stream));
    RT_HIP(c, hipMemsetAsync(c->ps.statTri(), 0, (size_t)n * 4, c->stream));
    hipLaunchKernelGGL(k_seed_rays, dim3((n + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, c->sc, c->ps, n);
    TraceArgs ta{nullptr, c->q.counts, prb, prt, (DevCounters*)c->counterBuf.p};
    if ((rc = launch_trace(c, one_part(c, c->sc, false), n, ta))) return rc;  // (perRayBox: the kernels with per-ray counters)
    hipLaunchKernelGGL(k_hit_details, dim3((n + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, c->sc, c->ps, n, prb, prt, dh);
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipMemcpyAsync(hitsOut, dh, (size_t)n * sizeof(RtHit), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return harvest_events(c);
}

int rt_render_aovs(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                   uint32_t nRows, const RtAovBuffers* d_out) {
    if (!c || !pc) return -1;
    int rc = check_tile(c, pc, width, height, row0, rowStride, nRows, "rt_render_aovs");
    if (rc) return rc;
    const std::string tooLarge = check_tile_slots("rt_render_aovs", width, nRows);
    if (!tooLarge.empty()) return c->fail(tooLarge);
    const uint32_t nPixels = nRows * width;
    RT_HIP(c, hipSetDevice(c->device));   // (also for a tile without pixels)
    if (nPixels == 0) return 0;
    Dispatch d;   // with the scene counts of this call
    if ((rc = side_pass_begin(c, nPixels, dispatch_scene(c, pc->rayTraceParams), &d))) return rc;
    if (!d_out && (rc = claim_planes(c, c->aov, nPixels, RowsOf{width, height, row0, rowStride, nRows}))) return rc;
    const AovOut out = aov_out(d_out, c->aov.buf.p, nPixels);
    FrameParams fp = frame_camera(c, pc, width, height, row0, rowStride, nRows, nPixels);
    fp.nFrames = 1;
    const uint32_t blocks = (nPixels + RT_BLOCK - 1) / RT_BLOCK;
    hipLaunchKernelGGL(k_aov_rays, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, fp);
    hipLaunchKernelGGL(k_init_counts, dim3(1), dim3(64), 0, c->stream, c->q.counts, nPixels);
    RT_HIP(c, hipGetLastError());
    const TraceArgs ta{nullptr, c->q.counts, nullptr, nullptr, (DevCounters*)c->aovCounterBuf.p};
    if ((rc = launch_trace(c, d, nPixels, ta))) return rc;
    hipLaunchKernelGGL(k_aov_resolve, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, fp, out);
    RT_HIP(c, hipGetLastError());
    return 0;
}
}  // extern "C"

namespace {
// a ctx-owned set of five planes (OwnedPlane in AovPlane's order) to the non-NULL host fields; blocks
int read_planes(rt_ctx* c, const OwnedPlane& pl, const char* fn, const char* never, const RtAovBuffers* out, size_t nPixels) {
    if (!c || !out) return -1;
    if (!pl.valid) return c->fail(never);
    if (nPixels != pl.pixels) return c->fail(std::string(fn) + ": size mismatch");
    RT_HIP(c, hipSetDevice(c->device));
    for (int k = 0; k < AOV_PLANES; k++)
        if (void* dst = aov_plane(*out, (AovPlane)k))
            RT_HIP(c, hipMemcpyAsync(dst, aov_plane(pl.buf.p, (AovPlane)k, nPixels), nPixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
enum { GUIDE_COUNTS = 16 };   // words of guideCountBuf: [j] the rays of round j, j = 1 .. RT_GUIDE_MAX_BOUNCES + 1 (the last one stays 0)
static_assert(RT_GUIDE_MAX_BOUNCES + 2 <= GUIDE_COUNTS, "a count per round");
}  // namespace

extern "C" {
int rt_read_aovs(rt_ctx* c, const RtAovBuffers* out, size_t nPixels) {
    return c ? read_planes(c, c->aov, "rt_read_aovs", NO_OWNED_AOVS, out, nPixels) : -1;
}

// Round 0 is rt_render_aovs' own (k_aov_rays, the traversal over every slot). After each round k_guide_follow writes the records of
// the chains that end there and queues the reflected rays of the others; round j > 0 traces that queue, whose length only the
// device knows: every round is enqueued, and one without rays costs its launches.
int rt_render_guides(rt_ctx* c, const PushConstants* pc, uint32_t width, uint32_t height, uint32_t row0, uint32_t rowStride,
                     uint32_t nRows, uint32_t maxBounces, const RtAovBuffers* d_guides, const RtAovBuffers* d_firstHit) {
    if (!c || !pc) return -1;
    const std::string refusal = check_guides(pc->rayTraceParams, width, height, row0, rowStride, nRows, maxBounces, d_guides, d_firstHit, uploaded_scene(c));
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t nPixels = nRows * width;
    RT_HIP(c, hipSetDevice(c->device));   // (also for a tile without pixels)
    if (nPixels == 0) return 0;
    int rc;
    Dispatch d;   // with the scene counts of this call
    if ((rc = side_pass_begin(c, nPixels, dispatch_scene(c, pc->rayTraceParams), &d))) return rc;
    if ((rc = dev_alloc(c, c->guideCountBuf, GUIDE_COUNTS * sizeof(uint32_t)))) return rc;
    if (!d_guides && (rc = claim_planes(c, c->guide, nPixels, RowsOf{width, height, row0, rowStride, nRows}))) return rc;
    FrameParams fp = frame_camera(c, pc, width, height, row0, rowStride, nRows, nPixels);
    fp.nFrames = 1;
    const uint32_t blocks = (nPixels + RT_BLOCK - 1) / RT_BLOCK;
    uint32_t* const counts = (uint32_t*)c->guideCountBuf.p;
    GuideArgs ga{nullptr, nullptr, nullptr, nullptr, d.counts + 4, 0u, maxBounces, aov_out(d_guides, c->guide.buf.p, nPixels), aov_out(d_firstHit, nullptr, 0)};
    RT_HIP(c, hipMemsetAsync(counts, 0, GUIDE_COUNTS * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_aov_rays, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, fp);
    hipLaunchKernelGGL(k_init_counts, dim3(1), dim3(64), 0, c->stream, c->q.counts, nPixels);
    RT_HIP(c, hipGetLastError());
    for (uint32_t j = 0; j <= maxBounces; j++) {
        ga.round = j;
        ga.queue = j ? c->q.rays[j & 1u] : nullptr;
        ga.count = j ? counts + j : c->q.counts;
        ga.outQueue = c->q.rays[(j + 1u) & 1u];
        ga.outCount = counts + j + 1;
        const TraceArgs ta{ga.queue, ga.count, nullptr, nullptr, (DevCounters*)c->aovCounterBuf.p};
        if ((rc = launch_trace(c, d, nPixels, ta))) return rc;
        hipLaunchKernelGGL(k_guide_follow, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, fp, ga);
        RT_HIP(c, hipGetLastError());
    }
    return 0;
}

int rt_read_guides(rt_ctx* c, const RtAovBuffers* out, size_t nPixels) {
    return c ? read_planes(c, c->guide, "rt_read_guides", NO_OWNED_GUIDES, out, nPixels) : -1;
}
}  // extern "C"

// ---- ray queries and the ambient-occlusion plane (ray_queries.h has the checks and the arithmetic; DESIGN.md, "Ray queries")
namespace {
// A side pass on the uploaded scene with a queue of n entries on top; a queue that grows waits for the device as the path state does
int query_begin(rt_ctx* c, uint32_t n, Dispatch* d) {
    const size_t queueBytes = query_shape(n, RT_BLOCK).queueBytes;
    int rc = side_pass_begin(c, n, c->sc, d);
    if (rc) return rc;
    if (c->queryQueueBuf.bytes < queueBytes) RT_HIP(c, hipStreamSynchronize(c->stream));
    return dev_alloc(c, c->queryQueueBuf, queueBytes);
}
// the traversal of the pass's queue: n entries, holes among them
int query_trace(rt_ctx* c, const Dispatch& d, uint32_t n) {
    const TraceArgs ta{(const uint32_t*)c->queryQueueBuf.p, c->q.counts, nullptr, nullptr, (DevCounters*)c->aovCounterBuf.p};
    return launch_trace(c, d, n, ta, true);
}

int query_device(rt_ctx* c, const char* fn, const RtRayBatch* rays, void* d_out, bool occlusion) {
    if (!c) return -1;
    const std::string refusal = check_ray_query(fn, c->sc.nodes != nullptr, rays, d_out);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    Dispatch d;
    int rc = query_begin(c, n, &d);
    if (rc) return rc;
    const uint32_t blocks = query_shape(n, RT_BLOCK).blocks;
    const QueryRays q{rays->origins, rays->dirs, rays->tmax, n, occlusion ? 1u : 0u, (uint32_t*)c->queryQueueBuf.p};
    hipLaunchKernelGGL(k_query_rays, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, q);
    hipLaunchKernelGGL(k_init_counts, dim3(1), dim3(64), 0, c->stream, c->q.counts, n);
    RT_HIP(c, hipGetLastError());
    if ((rc = query_trace(c, d, n))) return rc;
    if (occlusion) hipLaunchKernelGGL(k_query_occluded, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->ps, n, (uint8_t*)d_out);
    else hipLaunchKernelGGL(k_query_hits, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, n, (RtHit*)d_out);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged)
int query_host(rt_ctx* c, const char* fn, const RtRayBatch* rays, void* out, bool occlusion) {
    if (!c) return -1;
    const std::string refusal = check_ray_query(fn, c->sc.nodes != nullptr, rays, out);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    const QueryShape qs = query_shape(n, RT_BLOCK);
    const StagePart parts[] = {{rays->origins, nullptr, qs.vecBytes}, {rays->dirs, nullptr, qs.vecBytes}, {rays->tmax, nullptr, rays->tmax ? qs.tmaxBytes : 0},
                               {nullptr, out, occlusion ? qs.occludedBytes : qs.hitBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtRayBatch dev{(const float*)d[0], (const float*)d[1], (const float*)d[2], n};
        return query_device(c, fn, &dev, d[3], occlusion);
    });
}
}  // namespace

extern "C" {
int rt_query_closest(rt_ctx* c, const RtRayBatch* d_rays, RtHit* d_hits) { return query_device(c, "rt_query_closest", d_rays, d_hits, false); }
int rt_query_occluded(rt_ctx* c, const RtRayBatch* d_rays, uint8_t* d_occluded) { return query_device(c, "rt_query_occluded", d_rays, d_occluded, true); }
int rt_query_closest_host(rt_ctx* c, const RtRayBatch* rays, RtHit* hits) { return query_host(c, "rt_query_closest_host", rays, hits, false); }
int rt_query_occluded_host(rt_ctx* c, const RtRayBatch* rays, uint8_t* occluded) { return query_host(c, "rt_query_occluded_host", rays, occluded, true); }
}  // extern "C"

// ---- point queries (point_queries.h has the checks, the arithmetic and the pruning table; DESIGN.md, "Point queries")
namespace {
template <int STACK, bool RETEST>
void launch_nearest(rt_ctx* c, uint32_t blocks, const NearestArgs& na) {
    hipLaunchKernelGGL((k_nearest_points<STACK, RETEST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, na);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_nearest_points<%d, %s>", STACK, tf(RETEST));
}

int nearest_device(rt_ctx* c, const char* fn, const RtPointBatch* pts, RtNearest* d_out) {
    if (!c) return -1;
    const std::string refusal = check_point_query(fn, c->sc.nodes != nullptr, pts, d_out);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = pts->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = nearest_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const NearestArgs na{pts->points, pts->maxDist, n, (const float4*)c->objNearBuf.p, (float4*)d_out, (DevCounters*)c->aovCounterBuf.p};
    const uint32_t blocks = point_shape(n, RT_BLOCK).blocks;
    if (stack == (uint32_t)RT_NEAREST_STACK) launch_nearest<RT_NEAREST_STACK, true>(c, blocks, na);
    else launch_nearest<RT_NEAREST_STACK_DEEP, false>(c, blocks, na);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged)
int nearest_host(rt_ctx* c, const char* fn, const RtPointBatch* pts, RtNearest* out) {
    if (!c) return -1;
    const std::string refusal = check_point_query(fn, c->sc.nodes != nullptr, pts, out);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = pts->n;
    if (n == 0) return 0;
    const PointShape ps = point_shape(n, RT_BLOCK);
    const StagePart parts[] = {{pts->points, nullptr, ps.pointBytes}, {pts->maxDist, nullptr, pts->maxDist ? ps.limitBytes : 0}, {nullptr, out, ps.outBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtPointBatch dev{(const float*)d[0], (const float*)d[1], n};
        return nearest_device(c, fn, &dev, (RtNearest*)d[2]);
    });
}
}  // namespace

extern "C" {
int rt_query_nearest(rt_ctx* c, const RtPointBatch* d_points, RtNearest* d_out) { return nearest_device(c, "rt_query_nearest", d_points, d_out); }
int rt_query_nearest_host(rt_ctx* c, const RtPointBatch* points, RtNearest* out) { return nearest_host(c, "rt_query_nearest_host", points, out); }
}  // extern "C"

// ---- signed point queries (mesh_topology.h has the table, the checks and the host form; DESIGN.md, "Signed point queries")
namespace {
std::string signed_refusal(const rt_ctx* c, const char* fn, const RtPointBatch* pts, const void* out, const void* side) {
    const TopologyCounts scene{c->sc.objectCount, c->sc.triCount, (uint32_t)c->rootOf.size()};   // (rootOf: one entry per node of the host arrays)
    return check_signed_query(fn, c->sc.nodes != nullptr, c->topo.on, c->topo.counts, scene, pts, out, side);
}

// the search, then the side pass on what it wrote
int signed_device(rt_ctx* c, const char* fn, const RtPointBatch* pts, RtNearest* d_out, int8_t* d_side) {
    if (!c) return -1;
    const std::string refusal = signed_refusal(c, fn, pts, d_out, d_side);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = pts->n;
    if (n == 0) return 0;
    int rc = nearest_device(c, fn, pts, d_out);
    if (rc) return rc;
    const SideArgs sa{pts->points, n, (const float4*)d_out, (const uint4*)c->topo.rows.p, (const int32_t*)c->topo.orient.p, d_side, (DevCounters*)c->aovCounterBuf.p};
    hipLaunchKernelGGL(k_nearest_side<RT_BLOCK>, dim3(point_shape(n, RT_BLOCK).blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, sa);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_nearest_side<%d>", (int)RT_BLOCK);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): the point query's parts and one more, the bytes of side
int signed_host(rt_ctx* c, const char* fn, const RtPointBatch* pts, RtNearest* out, int8_t* side) {
    if (!c) return -1;
    const std::string refusal = signed_refusal(c, fn, pts, out, side);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = pts->n;
    if (n == 0) return 0;
    const PointShape ps = point_shape(n, RT_BLOCK);
    const StagePart parts[] = {{pts->points, nullptr, ps.pointBytes}, {pts->maxDist, nullptr, pts->maxDist ? ps.limitBytes : 0}, {nullptr, out, ps.outBytes}, {nullptr, side, (size_t)n}};
    return staged(c, parts, [&](void* const* d) {
        const RtPointBatch dev{(const float*)d[0], (const float*)d[1], n};
        return signed_device(c, fn, &dev, (RtNearest*)d[2], (int8_t*)d[3]);
    });
}
}  // namespace

extern "C" {
int rt_upload_topology(rt_ctx* c, const RtSceneArrays* s) {
    if (!c || !s) return -1;
    if (!c->sc.nodes) return c->fail("rt_upload_topology before rt_upload_scene");
    const TopologyTables t = build_topology("rt_upload_topology", *s);
    if (!t.error.empty()) return c->fail(t.error);
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipStreamSynchronize(c->stream));   // a side pass in flight may be reading the tables this replaces
    c->topo.on = false;
    int rc;
    if ((rc = upload(c, c->topo.rows, t.rows.data(), t.rows.size() * sizeof(uint4)))) return rc;
    if ((rc = upload(c, c->topo.orient, t.orientation.data(), t.orientation.size() * sizeof(int32_t)))) return rc;
    c->topo.counts = TopologyCounts{s->objectCount, s->triangleCount, s->bvhNodeCount};
    c->topo.on = true;
    return 0;
}
int rt_query_nearest_signed(rt_ctx* c, const RtPointBatch* d_points, RtNearest* d_out, int8_t* d_side) {
    return signed_device(c, "rt_query_nearest_signed", d_points, d_out, d_side);
}
int rt_query_nearest_signed_host(rt_ctx* c, const RtPointBatch* points, RtNearest* out, int8_t* side) {
    return signed_host(c, "rt_query_nearest_signed_host", points, out, side);
}
}  // extern "C"

// ---- all-hit ray queries (ray_hits.h has the checks, the arithmetic and the stack choice; DESIGN.md, "All-hit ray queries")
namespace {
template <int STACK, bool GLIST>
void launch_ray_hits(rt_ctx* c, uint32_t blocks, const RayHitsArgs& ha) {
    hipLaunchKernelGGL((k_ray_hits<STACK, GLIST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, ha);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_ray_hits<%d, %s>", STACK, tf(GLIST));
}

// the search, then with k > 0 the resolve pass on what it left in the records
int hits_device(rt_ctx* c, const char* fn, const RtRayBatch* rays, uint32_t k, RtHit* d_hits, uint32_t* d_counts) {
    if (!c) return -1;
    const std::string refusal = check_hits_query(fn, c->sc.nodes != nullptr, rays, k, d_hits, d_counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = hits_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const HitsShape hs = hits_shape(n, k, RT_BLOCK);
    const bool glist = stack != (uint32_t)RT_HITS_STACK;
    if (glist && k) {
        if (c->hitsListBuf.bytes < hs.listBytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees lists a search in flight may be using
        int rc = dev_alloc(c, c->hitsListBuf, hs.listBytes);
        if (rc) return rc;
    }
    const RayHitsArgs ha{rays->origins, rays->dirs, rays->tmax, n, k, (uint32_t*)d_hits, d_counts, (uint32_t*)c->hitsListBuf.p, (DevCounters*)c->aovCounterBuf.p};
    if (glist) launch_ray_hits<RT_HITS_STACK_DEEP, true>(c, hs.searchBlocks, ha);
    else launch_ray_hits<RT_HITS_STACK, false>(c, hs.searchBlocks, ha);
    if (k) hipLaunchKernelGGL(k_ray_hits_resolve<RT_BLOCK>, dim3(hs.resolveBlocks), dim3(RT_BLOCK), 0, c->stream, c->sc, ha);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): origins, dirs, tmax, hits, counts
int hits_host(rt_ctx* c, const char* fn, const RtRayBatch* rays, uint32_t k, RtHit* hits, uint32_t* counts) {
    if (!c) return -1;
    const std::string refusal = check_hits_query(fn, c->sc.nodes != nullptr, rays, k, hits, counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    const HitsShape hs = hits_shape(n, k, RT_BLOCK);
    const StagePart parts[] = {{rays->origins, nullptr, hs.vecBytes}, {rays->dirs, nullptr, hs.vecBytes}, {rays->tmax, nullptr, rays->tmax ? hs.tmaxBytes : 0},
                               {nullptr, hits, hs.hitBytes}, {nullptr, counts, hs.countBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtRayBatch dev{(const float*)d[0], (const float*)d[1], (const float*)d[2], n};
        return hits_device(c, fn, &dev, k, (RtHit*)d[3], (uint32_t*)d[4]);
    });
}
}  // namespace

extern "C" {
int rt_query_hits(rt_ctx* c, const RtRayBatch* d_rays, uint32_t k, RtHit* d_hits, uint32_t* d_counts) {
    return hits_device(c, "rt_query_hits", d_rays, k, d_hits, d_counts);
}
int rt_query_hits_host(rt_ctx* c, const RtRayBatch* rays, uint32_t k, RtHit* hits, uint32_t* counts) {
    return hits_host(c, "rt_query_hits_host", rays, k, hits, counts);
}
}  // extern "C"

// ---- radius point queries (point_within.h has the checks, the arithmetic and the stack choice; DESIGN.md, "Radius point queries")
namespace {
template <int STACK, bool GLIST>
void launch_points_within(rt_ctx* c, uint32_t blocks, const WithinArgs& wa) {
    hipLaunchKernelGGL((k_points_within<STACK, GLIST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, wa);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_points_within<%d, %s>", STACK, tf(GLIST));
}

// the search, then with k > 0 the resolve pass on what it left in the records
int within_device(rt_ctx* c, const char* fn, const RtPointBatch* pts, uint32_t k, RtNearest* d_out, uint32_t* d_counts) {
    if (!c) return -1;
    const std::string refusal = check_within_query(fn, c->sc.nodes != nullptr, pts, k, d_out, d_counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = pts->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = within_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const WithinShape ws = within_shape(n, k, RT_BLOCK);
    const bool glist = stack != (uint32_t)RT_WITHIN_STACK;
    if (glist && k) {
        if (c->withinListBuf.bytes < ws.listBytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees lists a search in flight may be using
        int rc = dev_alloc(c, c->withinListBuf, ws.listBytes);
        if (rc) return rc;
    }
    const WithinArgs wa{pts->points, pts->maxDist, n, k, (const float4*)c->objNearBuf.p, (uint32_t*)d_out, d_counts, (uint32_t*)c->withinListBuf.p, (DevCounters*)c->aovCounterBuf.p};
    if (glist) launch_points_within<RT_WITHIN_STACK_DEEP, true>(c, ws.searchBlocks, wa);
    else launch_points_within<RT_WITHIN_STACK, false>(c, ws.searchBlocks, wa);
    if (k) hipLaunchKernelGGL(k_points_within_resolve<RT_BLOCK>, dim3(ws.resolveBlocks), dim3(RT_BLOCK), 0, c->stream, c->sc, wa);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): points, maxDist, out, counts
int within_host(rt_ctx* c, const char* fn, const RtPointBatch* pts, uint32_t k, RtNearest* out, uint32_t* counts) {
    if (!c) return -1;
    const std::string refusal = check_within_query(fn, c->sc.nodes != nullptr, pts, k, out, counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = pts->n;
    if (n == 0) return 0;
    const WithinShape ws = within_shape(n, k, RT_BLOCK);
    const StagePart parts[] = {{pts->points, nullptr, ws.pointBytes}, {pts->maxDist, nullptr, pts->maxDist ? ws.limitBytes : 0}, {nullptr, out, ws.outBytes}, {nullptr, counts, ws.countBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtPointBatch dev{(const float*)d[0], (const float*)d[1], n};
        return within_device(c, fn, &dev, k, (RtNearest*)d[2], (uint32_t*)d[3]);
    });
}
}  // namespace

extern "C" {
int rt_query_within(rt_ctx* c, const RtPointBatch* d_points, uint32_t k, RtNearest* d_out, uint32_t* d_counts) {
    return within_device(c, "rt_query_within", d_points, k, d_out, d_counts);
}
int rt_query_within_host(rt_ctx* c, const RtPointBatch* points, uint32_t k, RtNearest* out, uint32_t* counts) {
    return within_host(c, "rt_query_within_host", points, k, out, counts);
}
}  // extern "C"

// ---- sphere sweeps (sweep_queries.h has the checks, the arithmetic and the stack choice; DESIGN.md, "Sphere sweeps")
namespace {
template <int STACK, bool RETEST>
void launch_sweep(rt_ctx* c, uint32_t blocks, const SweepArgs& sa) {
    hipLaunchKernelGGL((k_sweep_spheres<STACK, RETEST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, sa);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_sweep_spheres<%d, %s>", STACK, tf(RETEST));
}

int sweep_device(rt_ctx* c, const char* fn, const RtSweepBatch* b, RtSweep* d_out) {
    if (!c) return -1;
    const std::string refusal = check_sweep_query(fn, c->sc.nodes != nullptr, b, d_out);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = b->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = sweep_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const SweepArgs sa{b->origins, b->dirs, b->radius, b->tmax, n, (const float4*)c->objNearBuf.p, (float4*)d_out, (DevCounters*)c->aovCounterBuf.p};
    const uint32_t blocks = sweep_shape(n, RT_BLOCK).blocks;
    if (stack == (uint32_t)RT_SWEEP_STACK) launch_sweep<RT_SWEEP_STACK, true>(c, blocks, sa);
    else launch_sweep<RT_SWEEP_STACK_DEEP, false>(c, blocks, sa);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): origins, dirs, radius, tmax, out
int sweep_host(rt_ctx* c, const char* fn, const RtSweepBatch* b, RtSweep* out) {
    if (!c) return -1;
    const std::string refusal = check_sweep_query(fn, c->sc.nodes != nullptr, b, out);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = b->n;
    if (n == 0) return 0;
    const SweepShape ss = sweep_shape(n, RT_BLOCK);
    const StagePart parts[] = {{b->origins, nullptr, ss.vecBytes}, {b->dirs, nullptr, ss.vecBytes}, {b->radius, nullptr, ss.scalarBytes},
                               {b->tmax, nullptr, b->tmax ? ss.scalarBytes : 0}, {nullptr, out, ss.outBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtSweepBatch dev{(const float*)d[0], (const float*)d[1], (const float*)d[2], (const float*)d[3], n};
        return sweep_device(c, fn, &dev, (RtSweep*)d[4]);
    });
}
}  // namespace

extern "C" {
int rt_query_sweep(rt_ctx* c, const RtSweepBatch* d_batch, RtSweep* d_out) { return sweep_device(c, "rt_query_sweep", d_batch, d_out); }
int rt_query_sweep_host(rt_ctx* c, const RtSweepBatch* batch, RtSweep* out) { return sweep_host(c, "rt_query_sweep_host", batch, out); }
}  // extern "C"

// ---- radiance queries (radiance_queries.h has the checks and the arithmetic; DESIGN.md, "Radiance queries")
namespace {
// One piece of a batch through the multi-kernel pipeline, as render_parts runs a dispatch of pixels: ray generation per part,
// k_init_counts, the rounds, k_radiance_resolve. Nothing of it is reported as a dispatch: rt_last_parts stays.
int radiance_parts(rt_ctx* c, const FrameParams& fp, const Dispatch& d, const RadianceRays& q, float4* out) {
    const int nLanes = ensure_part_streams(c, choose_parts(c->tune, c->meas, scene_facts(c, d), dispatch_facts(d, &fp, false)));
    Lane lane[RT_MAX_LANES];
    make_parts(c, d, slice_parts(c->tune, q.n, 1u, nLanes), q.n, nLanes, lane);
    for (int l = 0; l < nLanes; l++) {
        const Lane& L = lane[l];
        if (!L.n) continue;
        hipLaunchKernelGGL(k_radiance_rays, dim3((L.n + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps,
                           c->q.active[0] + L.begin, c->q.rays[0] + 3 * (size_t)L.begin, fp, q, L.begin, L.begin + L.n);
        hipLaunchKernelGGL(k_init_counts, dim3(1), dim3(64), 0, c->stream, L.d.counts, L.n);
    }
    RT_HIP(c, hipGetLastError());
    if (int rc = render_rounds(c, fp, lane, nLanes, ShadePass{(DevCounters*)c->aovCounterBuf.p, q.origins, q.first})) return rc;
    hipLaunchKernelGGL(k_radiance_resolve, dim3((q.n + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, c->ps, fp, q.first, out);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The most rays of one piece (rt_set_tuning("radiance_max_kslots"); by default what "frames_max_mslots" allows a dispatch)
uint64_t radiance_max_slots(const rt_ctx* c) { return c->tune.radianceMaxSlots ? c->tune.radianceMaxSlots : c->tune.framesMaxSlots; }

int radiance_device(rt_ctx* c, const char* fn, const RtRayBatch* rays, const uint32_t* d_ids, const RtRadianceParams* params,
                    const EnvironmentData* env, float* d_radiance) {
    if (!c) return -1;
    const std::string refusal = check_radiance_query(fn, c->sc.nodes != nullptr, rays, params, d_radiance);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    const uint64_t maxSlots = radiance_max_slots(c);
    Dispatch d;   // the pieces' paths live in slots [0, cap); the uploaded scene's counts; always the multi-kernel pipeline
    int rc = side_pass_begin(c, std::min(n, radiance_piece_cap(maxSlots)), c->sc, &d);
    if (rc) return rc;
    d.pipeline = 0;
    FrameParams fp{};   // (the camera fields are unused: the rays are the caller's)
    fp.startingSeed = radiance_starting_seed(params->frameCount);
    fp.samples = params->samples;
    fp.bounceLimit = params->bounceLimit;
    fp.progressive = params->progressive;
    fp.frameCount = params->frameCount;
    fp.nFrames = 1;
    fp.camReuse = c->tune.cameraReuse ? 1u : 0u;
    fp.debug = -1;
    if (env) fp.env = *env;   // (NULL: environment.enabled == 0)
    fp.sampleMap = nullptr;
    const uint32_t pieces = radiance_piece_count(n, maxSlots);
    for (uint32_t k = 0; k < pieces; k++) {
        const RadiancePiece pc = radiance_piece(n, maxSlots, k);
        fp.nPixels = pc.n;
        const RadianceRays q{rays->origins, rays->dirs, d_ids, pc.first, pc.n};
        if ((rc = radiance_parts(c, fp, d, q, (float4*)d_radiance))) return rc;
    }
    return 0;
}
}  // namespace

extern "C" {
int rt_query_radiance(rt_ctx* c, const RtRayBatch* d_rays, const uint32_t* d_ids, const RtRadianceParams* params, const EnvironmentData* env,
                      float* d_radiance) {
    return radiance_device(c, "rt_query_radiance", d_rays, d_ids, params, env, d_radiance);
}

// The host-memory form (staged). What `radiance` holds goes up as well when the result is blended with it.
int rt_query_radiance_host(rt_ctx* c, const RtRayBatch* rays, const uint32_t* ids, const RtRadianceParams* params, const EnvironmentData* env,
                           float* radiance) {
    if (!c) return -1;
    const char* const fn = "rt_query_radiance_host";
    const std::string refusal = check_radiance_query(fn, c->sc.nodes != nullptr, rays, params, radiance);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = rays->n;
    if (n == 0) return 0;
    const RadianceShape rs = radiance_shape(n, ids != nullptr);
    const StagePart parts[] = {{rays->origins, nullptr, rs.vecBytes}, {rays->dirs, nullptr, rs.vecBytes}, {ids, nullptr, rs.idBytes},
                               {params->progressive ? radiance : nullptr, radiance, rs.outBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtRayBatch dev{(const float*)d[0], (const float*)d[1], nullptr, n};
        return radiance_device(c, fn, &dev, (const uint32_t*)d[2], params, env, (float*)d[3]);
    });
}
}  // extern "C"

// ---- baked-light queries (irradiance_queries.h has the checks, the chunks and the byte counts; include/rt_irradiance.h the rule;
// DESIGN.md, "Irradiance and SH probes")
namespace {
// Chunk by chunk: k_irradiance_rays into the ctx scratch, the chunk's rays through radiance_device() as one piece (one path per
// ray, not blended), k_irradiance_gather into the caller's array. Everything is enqueued on the ctx stream; the only wait is the
// one before the scratch grows.
template <bool SPHERE>
int irradiance_device(rt_ctx* c, const char* fn, const RtPointNormalBatch* b, const uint32_t* d_ids, const RtIrradianceParams* params,
                      const EnvironmentData* env, float* d_out) {
    if (!c) return -1;
    const uint64_t maxSlots = radiance_max_slots(c);
    const std::string refusal = check_irradiance_query(fn, SPHERE, c->sc.nodes != nullptr, b, params, d_out, maxSlots);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = b->n, S = params->samples;
    if (n == 0) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    const uint32_t most = std::min(n, irradiance_chunk_points(S, maxSlots));   // points of the largest chunk
    const IrradianceScratch sl = irradiance_scratch(most * S);
    if (c->irradianceBuf.bytes < sl.bytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees arrays a pass in flight may be using
    int rc = dev_alloc(c, c->irradianceBuf, sl.bytes);
    if (rc) return rc;
    char* const base = (char*)c->irradianceBuf.p;
    IrradianceArgs a{b->points, b->normals, d_ids, 0u, 0u, S, params->frameCount, params->bias, (float*)(base + sl.origins),
                     (float*)(base + sl.dirs), (uint32_t*)(base + sl.ids), (const float4*)(base + sl.radiance), d_out,
                     params->progressive, params->frameCount};
    const RtRadianceParams rp{1u, params->bounceLimit, 0u, params->frameCount};
    const uint32_t chunks = irradiance_chunk_count(n, S, maxSlots);
    for (uint32_t k = 0; k < chunks; k++) {
        const IrradianceChunk ch = irradiance_chunk(n, S, maxSlots, k);
        a.first = ch.first; a.count = ch.n;
        const uint32_t rays = ch.n * S;
        hipLaunchKernelGGL((k_irradiance_rays<SPHERE>), dim3((rays + RT_IRR_BLOCK - 1) / RT_IRR_BLOCK), dim3(RT_IRR_BLOCK), 0, c->stream, a);
        RT_HIP(c, hipGetLastError());
        const RtRayBatch rb{a.origins, a.dirs, nullptr, rays};
        if ((rc = radiance_device(c, fn, &rb, a.rayIds, &rp, env, (float*)(base + sl.radiance)))) return rc;
        const uint32_t groups = (ch.n + RT_IRR_BLOCK / 64 - 1) / (RT_IRR_BLOCK / 64);
        hipLaunchKernelGGL((k_irradiance_gather<SPHERE>), dim3(groups), dim3(RT_IRR_BLOCK), 0, c->stream, a);
        RT_HIP(c, hipGetLastError());
    }
    return 0;
}

// The host-memory form (staged): points, normals, ids, and the result, which goes up as well when it is blended with
template <bool SPHERE>
int irradiance_host(rt_ctx* c, const char* fn, const RtPointNormalBatch* b, const uint32_t* ids, const RtIrradianceParams* params,
                    const EnvironmentData* env, float* out) {
    if (!c) return -1;
    const std::string refusal = check_irradiance_query(fn, SPHERE, c->sc.nodes != nullptr, b, params, out, radiance_max_slots(c));
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = b->n;
    if (n == 0) return 0;
    const IrradianceShape g = irradiance_shape(n, ids != nullptr, SPHERE);
    const StagePart parts[] = {{b->points, nullptr, g.vecBytes}, {b->normals, nullptr, !SPHERE ? g.vecBytes : 0}, {ids, nullptr, g.idBytes},
                               {params->progressive ? out : nullptr, out, g.outBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtPointNormalBatch dev{(const float*)d[0], (const float*)d[1], n};
        return irradiance_device<SPHERE>(c, fn, &dev, (const uint32_t*)d[2], params, env, (float*)d[3]);
    });
}
}  // namespace

extern "C" {
int rt_query_irradiance(rt_ctx* c, const RtPointNormalBatch* d_batch, const uint32_t* d_ids, const RtIrradianceParams* params,
                        const EnvironmentData* env, float* d_out) {
    return irradiance_device<false>(c, "rt_query_irradiance", d_batch, d_ids, params, env, d_out);
}
int rt_query_irradiance_host(rt_ctx* c, const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params,
                             const EnvironmentData* env, float* out) {
    return irradiance_host<false>(c, "rt_query_irradiance_host", batch, ids, params, env, out);
}
int rt_query_sh_probes(rt_ctx* c, const RtPointNormalBatch* d_batch, const uint32_t* d_ids, const RtIrradianceParams* params,
                       const EnvironmentData* env, float* d_out) {
    return irradiance_device<true>(c, "rt_query_sh_probes", d_batch, d_ids, params, env, d_out);
}
int rt_query_sh_probes_host(rt_ctx* c, const RtPointNormalBatch* batch, const uint32_t* ids, const RtIrradianceParams* params,
                            const EnvironmentData* env, float* out) {
    return irradiance_host<true>(c, "rt_query_sh_probes_host", batch, ids, params, env, out);
}
}  // extern "C"

// ---- lightmap texels (texel_queries.h has the checks, the launch shapes, the scan's levels and the byte counts; include/rt_texels.h
// the rule; DESIGN.md, "Lightmap texels")
namespace {
// a ctx scratch of at least `bytes`; growing frees memory a pass in flight may be using, so it waits first
int texel_buffer(rt_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes < bytes) RT_HIP(c, hipStreamSynchronize(c->stream));
    return dev_alloc(c, b, bytes);
}

// The exclusive scan of n values (load(i)) into excl (NULL: only the scanned block sums are wanted), level by level through
// `sums` (scan_levels(n).elems values). Afterwards sums[0 .. ceil(n / 256)) holds what precedes each block of level 0.
template <typename T, typename LOAD>
int scan_exclusive(rt_ctx* c, LOAD load, uint64_t n, T* excl, T* sums) {
    const ScanLevels L = scan_levels(n);
    hipLaunchKernelGGL((k_scan_local<T, LOAD>), dim3(texel_groups(L.count[0], RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, load,
                       (unsigned long long)L.count[0], excl, sums + L.offset[0]);
    for (int l = 1; l < L.levels; l++) {
        T* const vals = sums + L.offset[l - 1];
        hipLaunchKernelGGL((k_scan_local<T, ScanLoadSame<T>>), dim3(texel_groups(L.count[l], RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream,
                           ScanLoadSame<T>{vals}, (unsigned long long)L.count[l], vals, sums + L.offset[l]);
    }
    for (int l = L.levels - 2; l >= 1; l--)
        hipLaunchKernelGGL((k_scan_add<T>), dim3(texel_groups(L.count[l], RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, sums + L.offset[l - 1],
                           (unsigned long long)L.count[l], (const T*)(sums + L.offset[l]));
    if (excl)
        hipLaunchKernelGGL((k_scan_add<T>), dim3(texel_groups(L.count[0], RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, excl,
                           (unsigned long long)L.count[0], (const T*)(sums + L.offset[0]));
    RT_HIP(c, hipGetLastError());
    return 0;
}

uint32_t texel_tri_total(const rt_ctx* c, uint32_t object) {
    return object < c->hostObjects.size() && c->hostObjects[object].bvhIndex < c->rootOf.size() ? c->rootOf[c->hostObjects[object].bvhIndex].triTotal : 0u;
}

// Enqueues the bake; the statistics stay in the ctx scratch (*d_stats) for whoever wants them
int bake_texels_device(rt_ctx* c, const char* fn, uint32_t object, uint32_t width, uint32_t height, RtTexel* d_texels, const uint32_t** d_stats) {
    if (!c) return -1;
    const std::string refusal = check_texel_bake(fn, c->sc.nodes != nullptr, d_texels, object, c->sc.objectCount, width, height, texel_tri_total(c, object));
    if (!refusal.empty()) return c->fail(refusal);
    if (object >= c->hostObjects.size()) return c->fail(std::string(fn) + ": object " + std::to_string(object) + " is not among the uploaded objects");
    RT_HIP(c, hipSetDevice(c->device));
    const RootInfo& root = c->rootOf[c->hostObjects[object].bvhIndex];
    const TexelScratch sl = texel_scratch(root.triTotal, width, height);
    int rc = texel_buffer(c, c->bakeTexelBuf, sl.bytes);
    if (rc) return rc;
    char* const base = (char*)c->bakeTexelBuf.p;
    const size_t n = (size_t)width * height;
    TexelArgs a{object, root.triFirst, root.triTotal, width, height, (uint32_t*)(base + sl.owner), (uint8_t*)(base + sl.overlapped),
                (uint32_t*)(base + sl.counts), (unsigned long long*)(base + sl.offsets), (uint32_t*)(base + sl.stats), (float4*)d_texels};
    RT_HIP(c, hipMemsetAsync(a.stats, 0, sizeof(RtTexelStats), c->stream));
    RT_HIP(c, hipMemsetAsync(a.owner, 0xff, 4 * n, c->stream));
    RT_HIP(c, hipMemsetAsync(a.overlapped, 0, n, c->stream));
    hipLaunchKernelGGL(k_texel_bins, dim3(texel_groups((uint64_t)root.triTotal + 1, RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, c->sc, a);
    RT_HIP(c, hipGetLastError());
    if ((rc = scan_exclusive<unsigned long long>(c, ScanLoadU32{a.counts}, (uint64_t)root.triTotal + 1, a.offsets, (unsigned long long*)(base + sl.sums)))) return rc;
    hipLaunchKernelGGL(k_texel_cover, dim3((uint32_t)c->numCUs * 8u), dim3(RT_TEXEL_GROUP), 0, c->stream, c->sc, a);
    RT_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_texel_resolve, dim3(texel_groups(n, RT_TEXEL_RESOLVE * RT_TEXEL_RESOLVE_RUNS)), dim3(RT_TEXEL_RESOLVE), 0, c->stream, c->sc, a);
    RT_HIP(c, hipGetLastError());
    if (d_stats) *d_stats = a.stats;
    return 0;
}

int texels_compact_device(rt_ctx* c, const char* fn, uint32_t nTexels, const RtTexel* d_texels, float* d_points, float* d_normals, uint32_t* d_index,
                          uint32_t* d_countOut) {
    if (!c) return -1;
    if (!c->sc.nodes) return c->fail(std::string(fn) + " before rt_upload_scene");
    const std::string refusal = check_texel_pass(fn, d_texels && d_points && d_normals && d_index && d_countOut, nTexels, 0u, 0u);
    if (!refusal.empty()) return c->fail(refusal);
    RT_HIP(c, hipSetDevice(c->device));
    int rc = texel_buffer(c, c->bakeScanBuf, sizeof(uint32_t) * (size_t)scan_levels(nTexels).elems);
    if (rc) return rc;
    uint32_t* const sums = (uint32_t*)c->bakeScanBuf.p;
    if ((rc = scan_exclusive<uint32_t>(c, ScanLoadCovered{(const float4*)d_texels}, nTexels, (uint32_t*)nullptr, sums))) return rc;
    const TexelCompactArgs a{nTexels, (const float4*)d_texels, sums, d_points, d_normals, d_index, d_countOut};
    hipLaunchKernelGGL(k_texel_compact, dim3(texel_groups(nTexels, RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, a);
    RT_HIP(c, hipGetLastError());
    return 0;
}

int texels_scatter_device(rt_ctx* c, const char* fn, uint32_t nTexels, uint32_t nCovered, const uint32_t* d_index, const float* d_values4, float* d_rgba,
                          uint8_t* d_fill) {
    if (!c) return -1;
    if (!c->sc.nodes) return c->fail(std::string(fn) + " before rt_upload_scene");
    const std::string refusal = check_texel_pass(fn, d_rgba && d_fill && (nCovered == 0 || (d_index && d_values4)), nTexels, nCovered, 0u);
    if (!refusal.empty()) return c->fail(refusal);
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipMemsetAsync(d_rgba, 0, 16 * (size_t)nTexels, c->stream));
    RT_HIP(c, hipMemsetAsync(d_fill, 0, nTexels, c->stream));
    if (nCovered) {
        hipLaunchKernelGGL(k_texel_scatter, dim3(texel_groups(nCovered, RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, nCovered, d_index,
                           (const float4*)d_values4, (float4*)d_rgba, d_fill, nTexels);
        RT_HIP(c, hipGetLastError());
    }
    return 0;
}

// `passes` passes in ping-pong between the caller's planes and a ctx pair; an odd count ends with a copy back
int dilate_texels_device(rt_ctx* c, const char* fn, uint32_t width, uint32_t height, uint32_t passes, float* d_rgba, uint8_t* d_fill) {
    if (!c) return -1;
    if (!c->sc.nodes) return c->fail(std::string(fn) + " before rt_upload_scene");
    std::string refusal = check_texel_pass(fn, d_rgba && d_fill, 1u, 0u, passes);
    if (refusal.empty()) refusal = check_texel_size(fn, width, height);
    if (!refusal.empty()) return c->fail(refusal);
    if (passes == 0) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)width * height;
    int rc = texel_buffer(c, c->bakeDilateBuf, 17 * n);
    if (rc) return rc;
    float* planes[2] = {d_rgba, (float*)c->bakeDilateBuf.p};
    uint8_t* fills[2] = {d_fill, (uint8_t*)c->bakeDilateBuf.p + 16 * n};
    for (uint32_t k = 1; k <= passes; k++) {
        const int from = (int)((k - 1u) & 1u), to = from ^ 1;
        hipLaunchKernelGGL(k_texel_dilate, dim3(texel_groups(n, RT_TEXEL_GROUP)), dim3(RT_TEXEL_GROUP), 0, c->stream, width, height, k,
                           (const float*)planes[from], (const uint8_t*)fills[from], (float4*)planes[to], fills[to]);
        RT_HIP(c, hipGetLastError());
    }
    if (passes & 1u) {
        RT_HIP(c, hipMemcpyAsync(d_rgba, planes[1], 16 * n, hipMemcpyDeviceToDevice, c->stream));
        RT_HIP(c, hipMemcpyAsync(d_fill, fills[1], n, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}
}  // namespace

extern "C" {
int rt_bake_texels(rt_ctx* c, uint32_t object, uint32_t width, uint32_t height, RtTexel* d_texels, RtTexelStats* statsOut) {
    const uint32_t* d_stats = nullptr;
    const int rc = bake_texels_device(c, "rt_bake_texels", object, width, height, d_texels, &d_stats);
    if (rc || !statsOut) return rc;
    RT_HIP(c, hipMemcpyAsync(statsOut, d_stats, sizeof(RtTexelStats), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int rt_bake_texels_host(rt_ctx* c, uint32_t object, uint32_t width, uint32_t height, RtTexel* texels, RtTexelStats* stats) {
    if (!c) return -1;
    const char* fn = "rt_bake_texels_host";
    const std::string refusal = check_texel_bake(fn, c->sc.nodes != nullptr, texels, object, c->sc.objectCount, width, height, texel_tri_total(c, object));
    if (!refusal.empty()) return c->fail(refusal);
    const StagePart parts[] = {{nullptr, texels, sizeof(RtTexel) * (size_t)width * height}, {nullptr, stats, stats ? sizeof(RtTexelStats) : 0}};
    return staged(c, parts, [&](void* const* d) {
        const uint32_t* d_stats = nullptr;
        const int rc = bake_texels_device(c, fn, object, width, height, (RtTexel*)d[0], &d_stats);
        if (rc || !d[1]) return rc;
        RT_HIP(c, hipMemcpyAsync(d[1], d_stats, sizeof(RtTexelStats), hipMemcpyDeviceToDevice, c->stream));
        return 0;
    });
}

int rt_texels_compact(rt_ctx* c, uint32_t nTexels, const RtTexel* d_texels, float* d_points, float* d_normals, uint32_t* d_index, uint32_t* d_countOut) {
    return texels_compact_device(c, "rt_texels_compact", nTexels, d_texels, d_points, d_normals, d_index, d_countOut);
}
int rt_texels_scatter(rt_ctx* c, uint32_t nTexels, uint32_t nCovered, const uint32_t* d_index, const float* d_values4, float* d_rgba, uint8_t* d_fill) {
    return texels_scatter_device(c, "rt_texels_scatter", nTexels, nCovered, d_index, d_values4, d_rgba, d_fill);
}
int rt_dilate_texels(rt_ctx* c, uint32_t width, uint32_t height, uint32_t passes, float* d_rgba, uint8_t* d_fill) {
    return dilate_texels_device(c, "rt_dilate_texels", width, height, passes, d_rgba, d_fill);
}

// The five passes in order through lightmapBuf. The one wait is for the count of covered texels: the irradiance query's batch
// size is read on the host.
int rt_bake_lightmap(rt_ctx* c, uint32_t object, uint32_t width, uint32_t height, const RtIrradianceParams* params, const EnvironmentData* env,
                     uint32_t dilatePasses, float* d_rgba, uint8_t* d_fill, RtTexelStats* statsOut) {
    if (!c) return -1;
    const char* fn = "rt_bake_lightmap";
    std::string refusal = check_texel_bake(fn, c->sc.nodes != nullptr, d_rgba, object, c->sc.objectCount, width, height, texel_tri_total(c, object));
    if (refusal.empty()) refusal = check_lightmap(fn, params, dilatePasses, d_fill);
    if (refusal.empty()) {
        const RtPointNormalBatch any{(const float*)d_rgba, (const float*)d_rgba, 1u};   // (never read: the refusals that do not depend on the batch)
        refusal = check_irradiance_query(fn, false, true, &any, params, d_rgba, radiance_max_slots(c));
    }
    if (!refusal.empty()) return c->fail(refusal);
    RT_HIP(c, hipSetDevice(c->device));
    const LightmapScratch sl = lightmap_scratch(width, height);
    int rc = texel_buffer(c, c->lightmapBuf, sl.bytes);
    if (rc) return rc;
    char* const base = (char*)c->lightmapBuf.p;
    const uint32_t nTexels = width * height;
    RtTexel* const texels = (RtTexel*)(base + sl.texels);
    float* const points = (float*)(base + sl.points);
    float* const normals = (float*)(base + sl.normals);
    uint32_t* const index = (uint32_t*)(base + sl.index);
    uint32_t* const count = (uint32_t*)(base + sl.count);
    float* const values = (float*)(base + sl.values);
    const uint32_t* d_stats = nullptr;
    if ((rc = bake_texels_device(c, fn, object, width, height, texels, &d_stats))) return rc;
    if ((rc = texels_compact_device(c, fn, nTexels, texels, points, normals, index, count))) return rc;
    uint32_t nCovered = 0;
    RtTexelStats stats;
    RT_HIP(c, hipMemcpyAsync(&nCovered, count, sizeof nCovered, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipMemcpyAsync(&stats, d_stats, sizeof stats, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (nCovered > nTexels) return c->fail(std::string(fn) + ": internal: " + std::to_string(nCovered) + " covered texels of " + std::to_string(nTexels));
    const RtPointNormalBatch batch{points, normals, nCovered};
    if ((rc = irradiance_device<false>(c, fn, &batch, index, params, env, values))) return rc;
    if ((rc = texels_scatter_device(c, fn, nTexels, nCovered, index, values, d_rgba, d_fill))) return rc;
    if ((rc = dilate_texels_device(c, fn, width, height, dilatePasses, d_rgba, d_fill))) return rc;
    if (statsOut) *statsOut = stats;
    return 0;
}
}  // extern "C"

extern "C" {
// `samples` rounds of {k_ao_rays, the traversal, k_ao_count}, all enqueued without waiting for the device, then k_ao_resolve
int rt_render_ao(rt_ctx* c, uint32_t nPixels, const RtAovBuffers* d_aovs, const RtAoParams* params, float* d_ao) {
    if (!c) return -1;
    RtAoParams p;
    rt_ao_params_default(&p);
    if (params) p = *params;
    const std::string refusal = check_ao("rt_render_ao", c->sc.nodes != nullptr, nPixels, p, d_aovs, c->aov.valid, c->aov.pixels);
    if (!refusal.empty()) return c->fail(refusal);
    Dispatch d;
    int rc = query_begin(c, nPixels, &d);
    if (rc) return rc;
    const size_t countBytes = (size_t)nPixels * sizeof(uint32_t), aoBytes = (size_t)nPixels * sizeof(float);
    if (c->aoCountBuf.bytes < countBytes || (!d_ao && c->aoBuf.bytes < aoBytes)) RT_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = dev_alloc(c, c->aoCountBuf, countBytes))) return rc;
    if (!d_ao) {
        if ((rc = dev_alloc(c, c->aoBuf, aoBytes))) return rc;
        c->aoPixels = nPixels;
    }
    const AovOut in = aov_out(d_aovs, c->aov.buf.p, nPixels);
    AoArgs a{in.position, in.normalDepth, in.ids, nPixels, 0u, p.samples, p.seed,
             p.radius, (uint32_t*)c->queryQueueBuf.p, (uint32_t*)c->aoCountBuf.p, d.counts + 4};
    const uint32_t blocks = query_shape(nPixels, RT_BLOCK).blocks;
    hipLaunchKernelGGL(k_init_counts, dim3(1), dim3(64), 0, c->stream, c->q.counts, nPixels);
    for (uint32_t s = 0; s < p.samples; s++) {
        a.sample = s;
        hipLaunchKernelGGL(k_ao_rays, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, d.sc, c->ps, a);
        RT_HIP(c, hipGetLastError());
        if ((rc = query_trace(c, d, nPixels))) return rc;
        hipLaunchKernelGGL(k_ao_count, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->ps, a);
        RT_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_ao_resolve, dim3(blocks), dim3(RT_BLOCK), 0, c->stream, a, d_ao ? d_ao : (float*)c->aoBuf.p);
    RT_HIP(c, hipGetLastError());
    return 0;
}

int rt_read_ao(rt_ctx* c, float* out, size_t nFloats) {
    if (!c || !out) return -1;
    if (!c->aoPixels) return c->fail("no ctx-owned AO plane: rt_render_ao was never called with d_ao = NULL");
    if (nFloats != c->aoPixels) return c->fail("rt_read_ao: size mismatch");
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipMemcpyAsync(out, c->aoBuf.p, nFloats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}
}  // extern "C"

// ---- the passes over finished frames: denoising and temporal accumulation. Each reads as: check, resolve the inputs, check the
// outputs against them (post_passes.h), allocate, launch.
namespace {
// The parameters of a pass: the caller's, or the defaults
template <typename P>
P params_or(const P* given, void (*defaults)(P*)) { P p; defaults(&p); return given ? *given : p; }

// The output of a pass: the caller's plane, or the ctx's own for `n` pixels (the caller has synchronised if that grows it)
int output_plane(rt_ctx* c, float* d_out, OwnedPlane& own, size_t n, float4** out) {
    *out = (float4*)d_out;
    if (d_out) return 0;
    int rc = dev_alloc(c, own.buf, n * sizeof(float4));
    if (rc) return rc;
    *out = (float4*)own.buf.p;
    own.pixels = n;
    own.valid = true;
    return 0;
}

// The motion table onto the device, on the ctx stream: stream order keeps the copy behind the launch that still reads the table of
// the call before, and the call stays asynchronous. The pinned staging copy is this call's until the event says the copy engine has
// read it; only a second upload before that waits.
int upload_motion(rt_ctx* c, const MotionTable& mt, TemporalMotion& mo) {
    const size_t ob = mt.objects.size() * sizeof(float4), sb = mt.spheres.size() * sizeof(float4), bytes = ob + sb;
    if (!c->tpMotionEvent) RT_HIP(c, hipEventCreateWithFlags(&c->tpMotionEvent, hipEventDisableTiming));
    else RT_HIP(c, hipEventSynchronize(c->tpMotionEvent));
    if (c->tpMotionHostBytes < bytes) {
        if (c->tpMotionHost) (void)hipHostFree(c->tpMotionHost);
        c->tpMotionHost = nullptr; c->tpMotionHostBytes = 0;
        RT_HIP(c, hipHostMalloc((void**)&c->tpMotionHost, bytes, hipHostMallocDefault));
        c->tpMotionHostBytes = bytes;
    }
    if (c->tpMotionBuf.bytes < bytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // a table that grows frees the one a launch may still read
    int rc = dev_alloc(c, c->tpMotionBuf, bytes);
    if (rc) return rc;
    memcpy(c->tpMotionHost, mt.objects.data(), ob);
    memcpy((char*)c->tpMotionHost + ob, mt.spheres.data(), sb);
    RT_HIP(c, hipMemcpyAsync(c->tpMotionBuf.p, c->tpMotionHost, bytes, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipEventRecord(c->tpMotionEvent, c->stream));
    mo.objects = (const float4*)c->tpMotionBuf.p;
    mo.spheres = (const float4*)((const char*)c->tpMotionBuf.p + ob);
    mo.objectCount = mt.objectCount;
    mo.sphereCount = mt.sphereCount;
    return 0;
}
}  // namespace

extern "C" {

void rt_denoise_params_default(RtDenoiseParams* p) {
    if (p) *p = RtDenoiseParams{5u, 4.f, 128.f, 1.f};
}

int rt_denoise(rt_ctx* c, uint32_t width, uint32_t height, const float* d_rgba, const RtAovBuffers* d_aovs, const RtDenoiseParams* params,
               float* d_out) {
    if (!c) return -1;
    const RtDenoiseParams p = params_or(params, rt_denoise_params_default);
    std::string m = check_denoise(width, height, p, c->sc.nodes != nullptr, "rt_denoise");
    if (!m.empty()) return c->fail(m);
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    const PassInputs in = resolve_inputs("rt_denoise", width, height, d_rgba, d_aovs, false, c->fb.owned(), c->aov.owned());
    if (!in.error.empty()) return c->fail(in.error);
    const NamedPlane outs[1] = {{"d_out", d_out}};
    if (!(m = check_overlap("rt_denoise", in, "d_out", outs, 1, bytes)).empty()) return c->fail(m);
    RT_HIP(c, hipSetDevice(c->device));
    // growing a plane frees the old one, which a denoise still in flight may be using
    const size_t workBytes = 2 * bytes + n * sizeof(float2);
    if ((p.iterations && c->dnWorkBuf.bytes < workBytes) || (!d_out && c->dnOut.buf.bytes < bytes)) RT_HIP(c, hipStreamSynchronize(c->stream));
    float4* out;
    int rc = output_plane(c, d_out, c->dnOut, n, &out);
    if (rc) return rc;
    if (p.iterations == 0) {
        RT_HIP(c, hipMemcpyAsync(out, in.rgba, bytes, hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
    if ((rc = dev_alloc(c, c->dnWorkBuf, workBytes))) return rc;
    float4* const work[2] = {(float4*)c->dnWorkBuf.p, (float4*)c->dnWorkBuf.p + n};
    const DenoiseFrame f{in.rgba, in.normalDepth, in.albedo, in.ids, (float2*)(work[1] + n), width, height};
    const dim3 grid((width + 15u) / 16u, (height + 15u) / 16u), block(RT_DN_BLOCK);
    hipLaunchKernelGGL(k_dn_demod, grid, block, 0, c->stream, f, c->sc.mats, c->sc.materialCount, work[0]);
    hipLaunchKernelGGL(k_dn_variance, grid, block, 0, c->stream, f, (const float4*)work[0], work[1]);
    for (uint32_t k = 0; k < p.iterations; k++) {   // pass k reads work[1 - k % 2] and writes work[k % 2], the last one `out`
        const float4* src = work[1 - (k & 1u)];
        if (k + 1 < p.iterations)
            hipLaunchKernelGGL(k_dn_atrous<false>, grid, block, 0, c->stream, f, src, work[k & 1u], (float4*)nullptr, 1 << k, p.sigmaLuminance,
                               p.sigmaNormal, p.sigmaDepth);
        else
            hipLaunchKernelGGL(k_dn_atrous<true>, grid, block, 0, c->stream, f, src, (float4*)nullptr, out, 1 << k, p.sigmaLuminance,
                               p.sigmaNormal, p.sigmaDepth);
    }
    RT_HIP(c, hipGetLastError());
    return 0;
}

int rt_read_denoised_rgba_f32(rt_ctx* c, float* out, size_t nFloats) {
    return read_plane(c, c ? &c->dnOut : nullptr, "rt_read_denoised_rgba_f32", "no ctx-owned denoised frame: rt_denoise was never called with d_out = NULL", out, nFloats);
}

int rt_denoise_host(rt_ctx* c, uint32_t width, uint32_t height, const float* rgba, const RtAovBuffers* aovs, const RtDenoiseParams* params,
                    float* out) {
    if (!c) return -1;
    const RtDenoiseParams p = params_or(params, rt_denoise_params_default);
    const std::string m = check_denoise(width, height, p, c->sc.nodes != nullptr, "rt_denoise_host");
    if (!m.empty()) return c->fail(m);
    if (!rgba || !out) return c->fail("rt_denoise_host: rgba and out are required");
    if (!aovs || !aovs->normalDepth || !aovs->albedo || !aovs->ids) return c->fail("rt_denoise_host: aovs needs the normalDepth, albedo and ids planes");
    const size_t bytes = (size_t)width * height * sizeof(float4);
    const StagePart parts[] = {{rgba, nullptr, bytes}, {aovs->normalDepth, nullptr, bytes}, {aovs->albedo, nullptr, bytes}, {aovs->ids, nullptr, bytes},
                               {nullptr, out, bytes}};
    return staged(c, parts, [&](void* const* d) {
        RtAovBuffers planes{};
        planes.normalDepth = (float*)d[1];
        planes.albedo = (float*)d[2];
        planes.ids = (uint32_t*)d[3];
        return rt_denoise(c, width, height, (const float*)d[0], &planes, &p, (float*)d[4]);
    });
}

void rt_temporal_params_default(RtTemporalParams* p) {
    if (p) *p = RtTemporalParams{32u, 0.9f, 0.02f};
}

int rt_temporal_reset(rt_ctx* c) {
    if (!c) return -1;
    c->temporal.reset();
    return 0;
}

int rt_temporal_track_motion(rt_ctx* c, int enabled) {
    if (!c) return -1;
    c->temporal.set_tracking(enabled != 0);
    return 0;
}

int rt_temporal_motion_state(const rt_ctx* c, uint32_t* movedObjects, uint32_t* replacedObjects, uint32_t* movedSpheres) {
    if (!c) return -1;
    const uint32_t* moved = c->temporal.moved_counts();
    if (movedObjects) *movedObjects = moved[0];
    if (replacedObjects) *replacedObjects = moved[1];
    if (movedSpheres) *movedSpheres = moved[2];
    return 0;
}

int rt_temporal_accumulate(rt_ctx* c, uint32_t width, uint32_t height, const CameraInfo* cam, const float* d_rgba, const RtAovBuffers* d_aovs,
                           const RtTemporalParams* params, float* d_out, float* d_moments) {
    if (!c) return -1;
    const RtTemporalParams p = params_or(params, rt_temporal_params_default);
    std::string m = check_temporal(width, height, cam, p, c->sc.nodes != nullptr, "rt_temporal_accumulate");
    if (!m.empty()) return c->fail(m);
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    const PassInputs in = resolve_inputs("rt_temporal_accumulate", width, height, d_rgba, d_aovs, true, c->fb.owned(), c->aov.owned());
    if (!in.error.empty()) return c->fail(in.error);
    const NamedPlane outs[2] = {{"d_out", d_out}, {"d_moments", d_moments}};
    if (!(m = check_overlap("rt_temporal_accumulate", in, "an output", outs, 2, bytes)).empty()) return c->fail(m);
    RT_HIP(c, hipSetDevice(c->device));
    // growing a plane frees the old one, which a call still in flight may be using
    const bool historyFits = c->tpHist[0].bytes >= 3 * bytes && c->tpHist[1].bytes >= 3 * bytes;
    if (!historyFits || (!d_out && c->tpOut.buf.bytes < bytes) || (!d_moments && c->tpMom.buf.bytes < bytes)) RT_HIP(c, hipStreamSynchronize(c->stream));
    float4 *out, *mom;
    int rc;
    if ((rc = dev_alloc(c, c->tpHist[0], 3 * bytes)) || (rc = dev_alloc(c, c->tpHist[1], 3 * bytes)) ||
        (rc = output_plane(c, d_out, c->tpOut, n, &out)) || (rc = output_plane(c, d_moments, c->tpMom, n, &mom))) {
        if (!historyFits) c->temporal.reset();   // a history buffer may be gone
        return rc;
    }
    const TemporalHistory::Step step = c->temporal.begin(width, height, historyFits);
    const TemporalFrame f{in.rgba, in.normalDepth, in.position, in.albedo, in.ids, step.read < 0 ? nullptr : (const float4*)c->tpHist[step.read].p,
                          (float4*)c->tpHist[step.write].p, out, mom, width, height};
    const dim3 grid((width + 15u) / 16u, (height + 15u) / 16u), block(RT_DN_BLOCK);
    const TemporalCamera& prevCam = c->temporal.camera();   // of the call that wrote step.read
    if (step.motion.any()) {
        TemporalMotion mo{};
        if ((rc = upload_motion(c, step.motion, mo))) return rc;
        hipLaunchKernelGGL(k_tp_accumulate_motion, grid, block, 0, c->stream, f, prevCam, c->sc.mats, c->sc.materialCount, (float)p.maxHistory,
                           p.normalCos, p.depthTolerance, mo);
    } else {
        hipLaunchKernelGGL(k_tp_accumulate, grid, block, 0, c->stream, f, prevCam, c->sc.mats, c->sc.materialCount, (float)p.maxHistory, p.normalCos,
                           p.depthTolerance);
    }
    RT_HIP(c, hipGetLastError());
    c->temporal.commit(*cam);
    if (!d_moments) c->tpMom.rows = RowsOf{width, height, 0u, 1u, height};   // (rt_build_sample_map reads the plane as this frame)
    return 0;
}

int rt_read_temporal_rgba_f32(rt_ctx* c, float* out, size_t nFloats) {
    return read_plane(c, c ? &c->tpOut : nullptr, "rt_read_temporal_rgba_f32", "no ctx-owned accumulated frame: rt_temporal_accumulate was never called with d_out = NULL", out, nFloats);
}

int rt_read_temporal_moments(rt_ctx* c, float* out, size_t nFloats) {
    return read_plane(c, c ? &c->tpMom : nullptr, "rt_read_temporal_moments", "no ctx-owned moments: rt_temporal_accumulate was never called with d_moments = NULL", out, nFloats);
}

int rt_temporal_accumulate_host(rt_ctx* c, uint32_t width, uint32_t height, const CameraInfo* cam, const float* rgba, const RtAovBuffers* aovs,
                                const RtTemporalParams* params, float* out, float* moments) {
    if (!c) return -1;
    const RtTemporalParams p = params_or(params, rt_temporal_params_default);
    const std::string m = check_temporal(width, height, cam, p, c->sc.nodes != nullptr, "rt_temporal_accumulate_host");
    if (!m.empty()) return c->fail(m);
    if (!rgba || !out) return c->fail("rt_temporal_accumulate_host: rgba and out are required");
    if (!aovs || !aovs->normalDepth || !aovs->position || !aovs->albedo || !aovs->ids)
        return c->fail("rt_temporal_accumulate_host: aovs needs the normalDepth, position, albedo and ids planes");
    const size_t bytes = (size_t)width * height * sizeof(float4);
    // (a NULL `moments` is not wanted back; the pass still writes the plane)
    const StagePart parts[] = {{rgba, nullptr, bytes}, {aovs->normalDepth, nullptr, bytes}, {aovs->position, nullptr, bytes}, {aovs->albedo, nullptr, bytes},
                               {aovs->ids, nullptr, bytes}, {nullptr, out, bytes}, {nullptr, moments, bytes}};
    return staged(c, parts, [&](void* const* d) {
        RtAovBuffers planes{};
        planes.normalDepth = (float*)d[1];
        planes.position = (float*)d[2];
        planes.albedo = (float*)d[3];
        planes.ids = (uint32_t*)d[4];
        return rt_temporal_accumulate(c, width, height, cam, (const float*)d[0], &planes, &p, (float*)d[5], (float*)d[6]);
    });
}

void rt_sample_map_params_default(RtSampleMapParams* p) {
    if (p) *p = RtSampleMapParams{4u, 1u, 16u, 0.05f, 0.01f};
}

int rt_build_sample_map(rt_ctx* c, uint32_t width, uint32_t height, const float* d_moments, const RtSampleMapParams* params, uint32_t* d_map) {
    if (!c) return -1;
    const RtSampleMapParams p = params_or(params, rt_sample_map_params_default);
    const std::string m = check_sample_map(width, height, p, d_moments != nullptr, c->tpMom.owned(), "rt_build_sample_map");
    if (!m.empty()) return c->fail(m);
    if (!d_map) return c->fail("rt_build_sample_map: d_map is required");
    RT_HIP(c, hipSetDevice(c->device));
    int rc = dev_alloc(c, c->smStatBuf, RT_SM_STRIPES * sizeof(SampleMapStatsDev));
    if (rc) return rc;
    RT_HIP(c, hipMemsetAsync(c->smStatBuf.p, 0, RT_SM_STRIPES * sizeof(SampleMapStatsDev), c->stream));
    const SampleMapArgs a{d_moments ? (const float4*)d_moments : (const float4*)c->tpMom.buf.p, d_map, (SampleMapStatsDev*)c->smStatBuf.p, width, height,
                          p.baseSamples, p.minSamples, p.maxSamples, p.targetRelError, p.luminanceFloor};
    hipLaunchKernelGGL(k_sample_map, dim3((width + 15u) / 16u, (height + 15u) / 16u), dim3(RT_DN_BLOCK), 0, c->stream, a);
    RT_HIP(c, hipGetLastError());
    c->smBuilt = true;
    return 0;
}

int rt_sample_map_stats(rt_ctx* c, RtSampleMapStats* out) {
    if (!c || !out) return -1;
    if (!c->smBuilt) return c->fail("rt_sample_map_stats: rt_build_sample_map was never called");
    RT_HIP(c, hipSetDevice(c->device));
    SampleMapStatsDev h[RT_SM_STRIPES];   // the kernel's striped copies (k_sample_map)
    RT_HIP(c, hipMemcpyAsync(h, c->smStatBuf.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    *out = RtSampleMapStats{};
    for (const SampleMapStatsDev& s : h) {
        out->samples += s.samples; out->pixels += s.pixels; out->unknown += s.unknown; out->aboveMin += s.aboveMin; out->atMax += s.atMax;
    }
    return 0;
}

int rt_build_sample_map_host(rt_ctx* c, uint32_t width, uint32_t height, const float* moments, const RtSampleMapParams* params, uint32_t* map) {
    if (!c) return -1;
    const RtSampleMapParams p = params_or(params, rt_sample_map_params_default);
    if (!moments || !map) return c->fail("rt_build_sample_map_host: moments and map are required");
    const std::string m = check_sample_map(width, height, p, true, OwnedRows{}, "rt_build_sample_map_host");
    if (!m.empty()) return c->fail(m);
    const size_t n = (size_t)width * height;
    const StagePart parts[] = {{moments, nullptr, n * sizeof(float4)}, {nullptr, map, n * sizeof(uint32_t)}};
    return staged(c, parts, [&](void* const* d) { return rt_build_sample_map(c, width, height, (const float*)d[0], &p, (uint32_t*)d[1]); });
}

int rt_get_counters(rt_ctx* c, RtCounters* out) {
    if (!c || !out) return -1;
    RT_HIP(c, hipSetDevice(c->device));
    DevCounters h, a;
    RT_HIP(c, hipMemcpyAsync(&h, c->counterBuf.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipMemcpyAsync(&a, c->aovCounterBuf.p, sizeof(a), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    // the AOV passes' block: traversal work only from rt_render_aovs, the guides and the ray queries (their other fields stay 0), and
    // every field from the radiance queries
    out->boxTests = h.boxTests + a.boxTests; out->triTests = h.triTests + a.triTests;
    out->raysTraced = h.raysTraced + a.raysTraced; out->raysHit = h.raysHit + a.raysHit;
    out->raysReference = h.raysReference + a.raysReference; out->paths = h.paths + a.paths; out->segments = h.segments + a.segments;
    out->traceLaunches = c->rep.traceLaunchesTotal + c->rep.aovLaunches;
    out->emitterTests = h.emitterTests + a.emitterTests;
    out->skippedBoxTests = h.skippedBoxTests + a.skippedBoxTests;
    if (c->tune.phaseStats) {
        unsigned long long ps[21];
        RT_HIP(c, hipMemcpy(ps, (char*)c->counterBuf.p + sizeof(DevCounters), sizeof(ps), hipMemcpyDeviceToHost));
        static const char* nm[4] = {"refill", "setup", "interior", "leaf"};
        for (int k = 0; k < 4; k++)
            fprintf(stderr, "[phase_stats] %-8s rounds %12llu lanes %14llu avg active %.1f  clocks/round %8.0f  share of wave time %.1f %%\n", nm[k], ps[k], ps[4 + k],
                    ps[k] ? (double)ps[4 + k] / ps[k] : 0.0, ps[k] ? (double)ps[8 + k] / ps[k] : 0.0,
                    100.0 * ps[8 + k] / std::max(1.0, (double)(ps[8] + ps[9] + ps[10] + ps[11])));
        fprintf(stderr, "[phase_stats] clocks per round from the step's first load to its data: refill (queue entry, incl. the atomic) %.0f, setup (ray, seed) %.0f, interior (child pair) %.0f, leaf (triangles) %.0f\n",
                ps[0] ? (double)ps[16] / ps[0] : 0.0, ps[1] ? (double)ps[17] / ps[1] : 0.0, ps[2] ? (double)ps[18] / ps[2] : 0.0, ps[3] ? (double)ps[19] / ps[3] : 0.0);
        fprintf(stderr, "[phase_stats] trips of the set-up step's object-skipping loop: %llu (%.1f per lane and set-up step)\n", ps[20], ps[5] ? (double)ps[20] / ps[5] : 0.0);
        fprintf(stderr, "[phase_stats] lanes sitting out interior rounds: %.1f at a leaf, %.1f in set-up states, %.1f without a ray (of 64, average)\n",
                ps[2] ? (double)ps[12] / ps[2] : 0.0, ps[2] ? (double)ps[13] / ps[2] : 0.0, ps[2] ? (double)ps[14] / ps[2] : 0.0);
        if (c->rep.waveTimesCount && c->waveTimeBuf.p) {  // the last k_trace_pw launch: when did its waves finish?
            std::vector<unsigned long long> t(c->rep.waveTimesCount * 2);
            RT_HIP(c, hipMemcpy(t.data(), c->waveTimeBuf.p, t.size() * 8, hipMemcpyDeviceToHost));
            unsigned long long t0 = ~0ull, t1 = 0;
            for (size_t w = 0; w < c->rep.waveTimesCount; w++) { t0 = std::min(t0, t[2 * w]); t1 = std::max(t1, t[2 * w + 1]); }
            std::vector<double> end(c->rep.waveTimesCount);
            double busy = 0;
            const double span = (double)(t1 - t0);
            for (size_t w = 0; w < c->rep.waveTimesCount; w++) { end[w] = (t[2 * w + 1] - t0) / span; busy += (t[2 * w + 1] - t[2 * w]) / span; }
            std::sort(end.begin(), end.end());
            auto q = [&](double f) { return end[std::min(end.size() - 1, (size_t)(f * end.size()))]; };
            fprintf(stderr, "[phase_stats] last launch: %zu waves, span %.3f ms (100 MHz clock), mean wave lifetime %.1f %% of it; waves finished by 10/25/50/75/90/99 %% : %.2f %.2f %.2f %.2f %.2f %.2f of the span\n",
                    c->rep.waveTimesCount, span / 1e5, 100.0 * busy / c->rep.waveTimesCount, q(0.10), q(0.25), q(0.50), q(0.75), q(0.90), q(0.99));
        }
    }
    return 0;
}

int rt_reset_counters(rt_ctx* c) {
    if (!c) return -1;
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    poll_ray_cost(c);  // a snapshot of the last dispatch's counters has arrived by now: what it says about the scene's rays is kept
    RT_HIP(c, hipMemsetAsync(c->counterBuf.p, 0, sizeof(DevCounters) + 256, c->stream));
    RT_HIP(c, hipMemsetAsync(c->aovCounterBuf.p, 0, sizeof(DevCounters), c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->meas.snapPending = false;
    c->meas.snapBox = 0; c->meas.snapRays = 0; c->meas.snapSeg = 0; c->meas.snapPaths = 0;
    int rc = harvest_events(c);
    c->rep.traceMs = 0.0; c->rep.traceLaunches = 0; c->rep.traceLaunchesTotal = 0; c->rep.aovLaunches = 0;
    c->rep.traceSpans.clear();
    return rc;
}

int rt_set_profiling(rt_ctx* c, int on) {
    if (!c) return -1;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    int rc = harvest_events(c);
    c->profiling = on != 0;
    if (on) {
        if (!c->profBase) RT_HIP(c, hipEventCreate(&c->profBase));
        RT_HIP(c, hipEventRecord(c->profBase, c->stream));
        c->rep.traceSpans.clear();
    }
    return rc;
}

int rt_get_trace_busy_ms(rt_ctx* c, double* ms) {
    if (!c || !ms) return -1;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    int rc = harvest_events(c);
    std::vector<std::pair<float, float>> v = c->rep.traceSpans;
    std::sort(v.begin(), v.end());
    double busy = 0.0, end = -1e300;
    for (const auto& iv : v) {
        if ((double)iv.first > end) { busy += (double)iv.second - (double)iv.first; end = iv.second; }
        else if ((double)iv.second > end) { busy += (double)iv.second - end; end = iv.second; }
    }
    *ms = busy;
    return rc;
}

int rt_get_trace_time_ms(rt_ctx* c, double* ms, uint64_t* launches) {
    if (!c) return -1;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    int rc = harvest_events(c);
    if (ms) *ms = c->rep.traceMs;
    if (launches) *launches = c->rep.traceLaunches;
    return rc;
}

const char* rt_last_kernel(const rt_ctx* c) { return c ? c->rep.lastKernel : ""; }
int rt_last_parts(const rt_ctx* c) { return c ? c->rep.lastParts : 0; }

int rt_set_tuning(rt_ctx* c, const char* key, int value) {
    if (!c || !key) return -1;
    const TuningChange ch = set_tuning(c->tune, key, value);
    if (!ch.error.empty()) return c->fail(ch.error);
    return ch.rebuildEmitters ? rebuild_emitters(c) : 0;
}

int rt_last_pipeline(const rt_ctx* c) { return c ? c->rep.lastPipeline : -1; }
double rt_ray_cost(const rt_ctx* c) { return c ? c->meas.boxPerRay : -1.0; }

// ---------------------------------------------------------------- GPU BVH build (bvh_build.hip.h)
int rt_bvh_build(rt_ctx* c, const TrianglePoint* points, uint32_t pointCount, Triangle* triangles, float* centroids, uint32_t count,
                 uint32_t triIndex0, uint32_t nodeBase, BVHNode* nodesOut, uint32_t nodeCapacity, uint32_t* nodeCountOut, uint32_t statsOut[3]) {
    if (!c || !points || !triangles || !centroids || !nodesOut || !nodeCountOut) return -1;
    if (count == 0) return c->fail("rt_bvh_build: a mesh with 0 triangles");
    if (nodeCapacity < 2u * count - 1u) return c->fail("rt_bvh_build: node capacity below 2 * count - 1");
    RT_HIP(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    const bool dbg = getenv("RT_BVH_DEBUG") != nullptr;
    auto mark = [&](const char* what) { if (dbg) fprintf(stderr, "[rt_bvh_build] %-12s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); };
    std::vector<float> verts((size_t)count * 9);
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t vi[3] = {triangles[i].v0, triangles[i].v1, triangles[i].v2};
        for (int k = 0; k < 3; k++) {
            if (vi[k] >= pointCount) return c->fail("rt_bvh_build: triangle point index out of range");
            memcpy(&verts[(size_t)i * 9 + 3 * k], points[vi[k]].position, 12);
        }
    }
    const size_t nNodesMax = 2 * (size_t)count - 1;
    DevBuf bVerts, bCent, bPerm, bTmp, bHole, bNodes, bList, bCtr, bWide;
    const uint32_t maxChunks = (count + RT_BVH_CHUNK - 1) / RT_BVH_CHUNK;
    int rc;
    if ((rc = upload(c, bVerts, verts.data(), verts.size() * 4)) || (rc = upload(c, bCent, centroids, (size_t)count * 12)) ||
        (rc = dev_alloc(c, bPerm, (size_t)count * 4)) || (rc = dev_alloc(c, bTmp, (size_t)count * 4)) || (rc = dev_alloc(c, bHole, (size_t)count * 4)) ||
        (rc = dev_alloc(c, bNodes, nNodesMax * sizeof(BNode))) || (rc = dev_alloc(c, bList, 2 * (size_t)(count + 1) * 4)) || (rc = dev_alloc(c, bCtr, 64)) ||
        (rc = dev_alloc(c, bWide, RT_BVH_WIDE_NODES * sizeof(WideAcc) + (size_t)RT_BVH_WIDE_NODES * maxChunks * 4)))
        return rc;
    mark("uploaded");
    BvhBuildArgs a{(const float*)bVerts.p, (const float*)bCent.p, (uint32_t*)bPerm.p, (uint32_t*)bTmp.p, (uint32_t*)bHole.p, (BNode*)bNodes.p, (uint32_t*)bCtr.p};
    uint32_t* lists[2] = {(uint32_t*)bList.p, (uint32_t*)bList.p + (count + 1)};
    uint32_t* nextCount = (uint32_t*)bCtr.p + 1;
    hipLaunchKernelGGL(k_bvh_root, dim3(1), dim3(RT_BVH_BLOCK), 0, c->stream, a, count);
    uint32_t zero = 0, nCur = 1;
    hipError_t e = hipMemcpyAsync(lists[0], &zero, 4, hipMemcpyHostToDevice, c->stream);  // the root is node 0
    int cur = 0;
    std::vector<uint32_t> levelStart{0u, 1u};  // arrival numbers of the nodes of level l: [levelStart[l], levelStart[l + 1])
    for (uint32_t level = 0; e == hipSuccess && nCur && level <= 64; level++) {
        e = hipMemsetAsync(nextCount, 0, 4, c->stream);
        if (e != hipSuccess) break;
        // threads per node by the size of the level's nodes: the whole mesh is spread over nCur of them
        if (nCur <= RT_BVH_WIDE_NODES && count >= 8192u) {  // big nodes: many work-groups per node (bvh_build.hip.h, wide path)
            const WideArgs w{a, lists[cur], (WideAcc*)bWide.p, (uint32_t*)((char*)bWide.p + RT_BVH_WIDE_NODES * sizeof(WideAcc)), maxChunks, lists[cur ^ 1], nextCount};
            const dim3 gc(maxChunks, nCur), gn(nCur);
            hipLaunchKernelGGL(w_init, gn, dim3(64), 0, c->stream, w);
            hipLaunchKernelGGL(w_minmax, gc, dim3(256), 0, c->stream, w);
            hipLaunchKernelGGL(w_bins, gc, dim3(256), 0, c->stream, w);
            hipLaunchKernelGGL(w_sweep, gn, dim3(64), 0, c->stream, w);
            hipLaunchKernelGGL(w_count, gc, dim3(256), 0, c->stream, w);
            hipLaunchKernelGGL(w_scan, gn, dim3(64), 0, c->stream, w);
            hipLaunchKernelGGL(w_left, gc, dim3(256), 0, c->stream, w);
            hipLaunchKernelGGL(w_right, gc, dim3(256), 0, c->stream, w);
            hipLaunchKernelGGL(w_commit, gc, dim3(256), 0, c->stream, w);
            hipLaunchKernelGGL(w_finish, gn, dim3(64), 0, c->stream, w);
        }
        else if (nCur <= 32) hipLaunchKernelGGL(k_bvh_level<1024>, dim3(nCur), dim3(1024), 0, c->stream, a, lists[cur], lists[cur ^ 1], nextCount);
        else if (count / nCur >= 128) hipLaunchKernelGGL(k_bvh_level<256>, dim3(nCur), dim3(256), 0, c->stream, a, lists[cur], lists[cur ^ 1], nextCount);
        else hipLaunchKernelGGL(k_bvh_level<64>, dim3(nCur), dim3(64), 0, c->stream, a, lists[cur], lists[cur ^ 1], nextCount);
        e = hipMemcpyAsync(&nCur, nextCount, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (nCur) levelStart.push_back(levelStart.back() + nCur);
        cur ^= 1;
    }
    if (e == hipSuccess) e = hipGetLastError();
    mark("levels done");
    uint32_t nNodes = 0;
    if (e == hipSuccess) e = hipMemcpy(&nNodes, bCtr.p, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && (nNodes == 0 || nNodes > nNodesMax || nNodes != levelStart.back())) return c->fail("rt_bvh_build: node counter out of range");

    // ---- the reference's numbering (bvh_build.hip.h): interior counts bottom-up, slots top-down, nodes written in place
    DevBuf bNum, bOut;
    uint32_t hstats[3] = {0u, 0xffffffffu, 0u};
    if (e == hipSuccess && ((rc = dev_alloc(c, bNum, 3 * (size_t)nNodes * 4 + 64)) || (rc = dev_alloc(c, bOut, (size_t)nNodes * sizeof(BVHNode)))))
        return rc;
    std::vector<uint32_t> perm(count);
    if (e == hipSuccess) {
        uint32_t* nb = (uint32_t*)bNum.p;
        uint32_t* dstats = nb + 3 * (size_t)nNodes;
        BvhNumberArgs na{(const BNode*)bNodes.p, nb, nb + nNodes, nb + 2 * (size_t)nNodes, (BVHNode*)bOut.p, dstats, triIndex0, nodeBase};
        e = hipMemcpyAsync(dstats, hstats, 12, hipMemcpyHostToDevice, c->stream);
        const int nLevels = (int)levelStart.size() - 1;
        for (int l = nLevels - 1; l >= 0 && e == hipSuccess; l--) {
            const uint32_t b0 = levelStart[l], b1 = levelStart[l + 1];
            hipLaunchKernelGGL(k_bvh_count, dim3((b1 - b0 + 255) / 256), dim3(256), 0, c->stream, na, b0, b1);
        }
        for (int l = 0; l < nLevels && e == hipSuccess; l++) {
            const uint32_t b0 = levelStart[l], b1 = levelStart[l + 1];
            hipLaunchKernelGGL(k_bvh_number, dim3((b1 - b0 + 255) / 256), dim3(256), 0, c->stream, na, b0, b1);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(nodesOut, bOut.p, (size_t)nNodes * sizeof(BVHNode), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hstats, dstats, 12, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(perm.data(), bPerm.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipGetLastError();
    }
    mark("numbered");
    for (DevBuf* b : {&bVerts, &bCent, &bPerm, &bTmp, &bHole, &bNodes, &bList, &bCtr, &bWide, &bNum, &bOut}) b->release();  // now, not at the return: the host's part follows
    if (e != hipSuccess) return c->fail(std::string("rt_bvh_build: ") + hipGetErrorString(e));
    *nodeCountOut = nNodes;
    if (statsOut) { statsOut[0] = hstats[0]; statsOut[1] = hstats[1]; statsOut[2] = hstats[2]; }

    // ---- triangles and centroids into the order the partition loops leave them in
    std::vector<Triangle> tOld(triangles, triangles + count);
    std::vector<float> cOld(centroids, centroids + (size_t)count * 3);
    for (uint32_t k2 = 0; k2 < count; k2++) {
        if (perm[k2] >= count) return c->fail("rt_bvh_build: bad permutation");
        triangles[k2] = tOld[perm[k2]];
        memcpy(centroids + 3 * (size_t)k2, &cOld[3 * (size_t)perm[k2]], 12);
    }
    mark("permuted");
    c->rep.bvhBuildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int rt_bvh_hook(void* ctx, const TrianglePoint* points, uint32_t pointCount, Triangle* triangles, float* centroids, uint32_t count,
                uint32_t triIndex0, uint32_t nodeBase, BVHNode* nodesOut, uint32_t nodeCapacity, uint32_t* nodeCountOut, uint32_t statsOut[3]) {
    return rt_bvh_build((rt_ctx*)ctx, points, pointCount, triangles, centroids, count, triIndex0, nodeBase, nodesOut, nodeCapacity, nodeCountOut, statsOut);
}

double rt_bvh_last_build_ms(const rt_ctx* c) { return c ? c->rep.bvhBuildMs : 0.0; }

int rt_device_selftest(rt_ctx* c, uint32_t* bitsOut) {
    if (!c || !bitsOut) return -1;
    RT_HIP(c, hipSetDevice(c->device));
    const uint32_t n = 4096;
    std::vector<float> a(n), b(n);
    uint32_t st = 12345u;
    for (uint32_t i = 0; i < n; i++) { a[i] = rt_random(&st); b[i] = rt_random(&st) + 1e-3f; }
    const float kat[7] = {1.0001220703125f, 0.9998779296875f, -1.f, 3.f, 1e-30f, 1e-10f, 2.f};
    size_t bytes = (size_t)n * 12 + 64 + 64;
    int rc = dev_alloc(c, c->scratchBuf, bytes);
    if (rc) return rc;
    float* da = (float*)c->scratchBuf.p;
    float* db = da + n;
    uint32_t* dh = (uint32_t*)(db + n);
    uint32_t* dbits = dh + n;
    float* dkat = (float*)(dbits + 8);
    RT_HIP(c, hipMemcpyAsync(da, a.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync(db, b.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync(dkat, kat, sizeof(kat), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_selftest, dim3(n / 256), dim3(256), 0, c->stream, da, db, n, dh, dbits, dkat);
    RT_HIP(c, hipGetLastError());
    std::vector<uint32_t> h(n);
    uint32_t bits = 0;
    RT_HIP(c, hipMemcpyAsync(h.data(), dh, n * 4, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipMemcpyAsync(&bits, dbits, 4, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t mismatches = 0;
    for (uint32_t i = 0; i < n; i++)
        if (h[i] != selftest_one(a[i], b[i])) mismatches++;
    // bit 31 set: device and host disagree on some primitive
    *bitsOut = bits | (mismatches ? 0x80000000u : 0u);
    if (mismatches) return c->fail("device/host deterministic-math mismatch in " + std::to_string(mismatches) + " of 4096 probes");
    return 0;
}

// ---------------------------------------------------------------- multi-GPU: the final gather over RCCL
// One process per GPU, one rt_ctx per process. RCCL is loaded when the first rt_comm_* call needs it (a host that
// renders on one GPU never touches it); the typed function pointers keep the calls checked against <rccl/rccl.h>.
namespace {
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("RCCL not found: ") + dlerror(); return false; }
        getUniqueId = (decltype(getUniqueId))dlsym(lib, "ncclGetUniqueId");
        commInitRank = (decltype(commInitRank))dlsym(lib, "ncclCommInitRank");
        commDestroy = (decltype(commDestroy))dlsym(lib, "ncclCommDestroy");
        groupStart = (decltype(groupStart))dlsym(lib, "ncclGroupStart");
        groupEnd = (decltype(groupEnd))dlsym(lib, "ncclGroupEnd");
        send = (decltype(send))dlsym(lib, "ncclSend");
        recv = (decltype(recv))dlsym(lib, "ncclRecv");
        errorString = (decltype(errorString))dlsym(lib, "ncclGetErrorString");
        if (!getUniqueId || !commInitRank || !commDestroy || !groupStart || !groupEnd || !send || !recv || !errorString) {
            err = "RCCL library lacks a required symbol";
            dlclose(lib); lib = nullptr;
            return false;
        }
        return true;
    }
} g_rccl;

int rccl_fail(rt_ctx* c, ncclResult_t r, const char* what) {
    c->error = std::string(what) + ": " + (g_rccl.errorString ? g_rccl.errorString(r) : "?");
    return -2000 - (int)r;
}
}  // namespace

static_assert(RT_COMM_ID_BYTES == sizeof(ncclUniqueId), "rt_amd.h: RT_COMM_ID_BYTES must be sizeof(ncclUniqueId)");

int rt_comm_unique_id(void* idOut) {
    if (!idOut) return -1;
    if (!g_rccl.load()) return -2;
    ncclUniqueId id;
    if (g_rccl.getUniqueId(&id) != ncclSuccess) return -3;
    memcpy(idOut, &id, sizeof(id));
    return 0;
}

int rt_comm_init(rt_ctx* c, const void* id, int nRanks, int rank) {
    if (!c || !id) return -1;
    if (nRanks < 1 || rank < 0 || rank >= nRanks) return c->fail("rt_comm_init: rank out of range");
    if (c->comm) return c->fail("rt_comm_init: this context already has a communicator");
    if (!g_rccl.load()) return c->fail(g_rccl.err);
    RT_HIP(c, hipSetDevice(c->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclResult_t r = g_rccl.commInitRank(&c->comm, nRanks, uid, rank);
    if (r != ncclSuccess) { c->comm = nullptr; return rccl_fail(c, r, "ncclCommInitRank"); }
    c->commRanks = nRanks; c->commRank = rank;
    return 0;
}

int rt_comm_destroy(rt_ctx* c) {
    if (!c) return -1;
    if (c->comm) {
        (void)hipStreamSynchronize(c->stream);
        g_rccl.commDestroy(c->comm);
        c->comm = nullptr;
    }
    c->commRanks = 0;
    return 0;
}

int rt_gather_strips(rt_ctx* c, const float* d_strip, uint32_t width, uint32_t height, int root, float* d_frame) {
    if (!c || !d_strip) return -1;
    if (!c->comm) return c->fail("rt_gather_strips before rt_comm_init");
    const int N = c->commRanks, me = c->commRank;
    if (root < 0 || root >= N) return c->fail("rt_gather_strips: root out of range");
    if (me == root && !d_frame) return c->fail("rt_gather_strips: the root needs d_frame");
    RT_HIP(c, hipSetDevice(c->device));
    auto rows_of = [&](int r) { return (uint32_t)r < height ? (height - (uint32_t)r + (uint32_t)N - 1u) / (uint32_t)N : 0u; };
    const size_t rowFloats = (size_t)width * 4;
    float* stage = nullptr;
    if (me == root) {
        int rc = dev_alloc(c, c->gatherBuf, (size_t)height * rowFloats * sizeof(float));
        if (rc) return rc;
        stage = (float*)c->gatherBuf.p;
    }
    // every rank's strip goes to the root over its own link: one send per rank, N receives on the root, one group
    ncclResult_t r = g_rccl.groupStart();
    if (r != ncclSuccess) return rccl_fail(c, r, "ncclGroupStart");
    if (rows_of(me)) r = g_rccl.send(d_strip, (size_t)rows_of(me) * rowFloats, ncclFloat, root, c->comm, c->stream);
    if (r == ncclSuccess && me == root) {
        size_t at = 0;
        for (int k = 0; k < N && r == ncclSuccess; k++) {
            if (rows_of(k)) r = g_rccl.recv(stage + at, (size_t)rows_of(k) * rowFloats, ncclFloat, k, c->comm, c->stream);
            at += (size_t)rows_of(k) * rowFloats;
        }
    }
    ncclResult_t e = g_rccl.groupEnd();
    if (r != ncclSuccess) return rccl_fail(c, r, "ncclSend/ncclRecv");
    if (e != ncclSuccess) return rccl_fail(c, e, "ncclGroupEnd");
    if (me == root) {  // strips (rank-major) -> image rows: row y came from rank y % N, its row y / N
        return rt_deinterleave_strips(c, stage, width, height, N, d_frame);
    }
    return 0;
}

int rt_deinterleave_strips(rt_ctx* c, const float* d_strips, uint32_t width, uint32_t height, int nRanks, float* d_frame) {
    if (!c || !d_strips || !d_frame) return -1;
    if (nRanks < 1 || width == 0 || height == 0) return c->fail("rt_deinterleave_strips: bad geometry");
    RT_HIP(c, hipSetDevice(c->device));
    const size_t n4 = (size_t)height * width;
    hipLaunchKernelGGL(k_deinterleave_rows, dim3((unsigned)((n4 + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, c->stream,
                       (const float4*)d_strips, (float4*)d_frame, width, height, (uint32_t)nRanks);
    RT_HIP(c, hipGetLastError());
    return 0;
}

int rt_deinterleave_strips_host(rt_ctx* c, const float* strips, uint32_t width, uint32_t height, int nRanks, float* frame) {
    if (!c || !strips || !frame) return -1;
    if (nRanks < 1 || width == 0 || height == 0) return c->fail("rt_deinterleave_strips: bad geometry");   // (the device form's words: an empty frame has no arrays to stage)
    const size_t bytes = (size_t)width * height * sizeof(float4);
    const StagePart parts[] = {{strips, nullptr, bytes}, {nullptr, frame, bytes}};
    return staged(c, parts, [&](void* const* d) { return rt_deinterleave_strips(c, (const float*)d[0], width, height, nRanks, (float*)d[1]); });
}

int rt_device_math_probe(rt_ctx* c, uint32_t n, const float* in, float* out) {
    if (!c || !in || !out) return -1;
    if (n == 0) return 0;
    const StagePart parts[] = {{in, nullptr, (size_t)n * 32 * 4}, {nullptr, out, (size_t)n * 64 * 4}};
    return staged(c, parts, [&](void* const* d) {
        hipLaunchKernelGGL(k_math_probe, dim3((n + 63) / 64), dim3(64), 0, c->stream, (const float*)d[0], (float*)d[1], n);
        RT_HIP(c, hipGetLastError());
        return 0;
    });
}

int rt_measure_copy_bandwidth(rt_ctx* c, size_t bytes, int iters, double* gbps) {
    if (!c || !gbps || iters <= 0) return -1;
    RT_HIP(c, hipSetDevice(c->device));
    bytes &= ~(size_t)255;
    if (bytes < 4096) return c->fail("copy size too small");
    void *src = nullptr, *dst = nullptr;
    RT_HIP(c, hipMalloc(&src, bytes));
    if (hipMalloc(&dst, bytes) != hipSuccess) { (void)hipFree(src); return c->fail("hipMalloc failed"); }
    (void)hipMemsetAsync(src, 1, bytes, c->stream);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    size_t n = bytes / 16;
    hipLaunchKernelGGL(k_copy_f4, dim3(256 * 8), dim3(256), 0, c->stream, (const float4*)src, (float4*)dst, n);
    (void)hipEventRecord(e0, c->stream);
    for (int i = 0; i < iters; i++)
        hipLaunchKernelGGL(k_copy_f4, dim3(256 * 8), dim3(256), 0, c->stream, (const float4*)src, (float4*)dst, n);
    (void)hipEventRecord(e1, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(src); (void)hipFree(dst);
    if (e != hipSuccess) return c->hip(e, "copy bandwidth");
    *gbps = (2.0 * (double)bytes * iters) / (ms * 1e-3) / 1e9;  // read + write
    return 0;
}

}  // extern "C"

// ---- box queries (box_queries.h has the checks, the arithmetic and the stack choice; DESIGN.md, "Box queries")
namespace {
template <int STACK, bool GLIST>
void launch_boxes_overlap(rt_ctx* c, uint32_t blocks, const BoxesArgs& ba) {
    hipLaunchKernelGGL((k_boxes_overlap<STACK, GLIST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, ba);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_boxes_overlap<%d, %s>", STACK, tf(GLIST));
}

// the search; it writes the records itself
int boxes_device(rt_ctx* c, const char* fn, const RtBoxBatch* boxes, uint32_t k, RtOverlap* d_out, uint32_t* d_counts) {
    if (!c) return -1;
    const std::string refusal = check_boxes_query(fn, c->sc.nodes != nullptr, boxes, k, d_out, d_counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = boxes->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = boxes_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const BoxesShape bs = boxes_shape(n, k, RT_BLOCK);
    const bool glist = stack != (uint32_t)RT_BOXES_STACK;
    if (glist && k) {
        if (c->boxesListBuf.bytes < bs.listBytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees lists a search in flight may be using
        int rc = dev_alloc(c, c->boxesListBuf, bs.listBytes);
        if (rc) return rc;
    }
    const BoxesArgs ba{boxes->lo, boxes->hi, n, k, (const float4*)c->objNearBuf.p, (uint4*)d_out, d_counts, (uint32_t*)c->boxesListBuf.p, (DevCounters*)c->aovCounterBuf.p};
    if (glist) launch_boxes_overlap<RT_BOXES_STACK_DEEP, true>(c, bs.blocks, ba);
    else launch_boxes_overlap<RT_BOXES_STACK, false>(c, bs.blocks, ba);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): lo, hi, out, counts
int boxes_host(rt_ctx* c, const char* fn, const RtBoxBatch* boxes, uint32_t k, RtOverlap* out, uint32_t* counts) {
    if (!c) return -1;
    const std::string refusal = check_boxes_query(fn, c->sc.nodes != nullptr, boxes, k, out, counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = boxes->n;
    if (n == 0) return 0;
    const BoxesShape bs = boxes_shape(n, k, RT_BLOCK);
    const StagePart parts[] = {{boxes->lo, nullptr, bs.cornerBytes}, {boxes->hi, nullptr, bs.cornerBytes}, {nullptr, out, bs.outBytes}, {nullptr, counts, bs.countBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtBoxBatch dev{(const float*)d[0], (const float*)d[1], n};
        return boxes_device(c, fn, &dev, k, (RtOverlap*)d[2], (uint32_t*)d[3]);
    });
}
}  // namespace

extern "C" {
int rt_query_boxes(rt_ctx* c, const RtBoxBatch* d_boxes, uint32_t k, RtOverlap* d_out, uint32_t* d_counts) {
    return boxes_device(c, "rt_query_boxes", d_boxes, k, d_out, d_counts);
}
int rt_query_boxes_host(rt_ctx* c, const RtBoxBatch* boxes, uint32_t k, RtOverlap* out, uint32_t* counts) {
    return boxes_host(c, "rt_query_boxes_host", boxes, k, out, counts);
}
}  // extern "C"

// ---- oriented box queries (obb_queries.h has the checks, the arithmetic and the stack choice; DESIGN.md, "Oriented box queries")
namespace {
template <int STACK, bool GLIST>
void launch_obbs_overlap(rt_ctx* c, uint32_t blocks, const ObbsArgs& ba) {
    hipLaunchKernelGGL((k_obbs_overlap<STACK, GLIST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, ba);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_obbs_overlap<%d, %s>", STACK, tf(GLIST));
}

// the search; it writes the records itself. The deep search's lists share boxesListBuf: the passes run one behind the other on
// the ctx stream, and neither keeps anything in it between launches
int obbs_device(rt_ctx* c, const char* fn, const RtObbBatch* batch, uint32_t k, RtOverlap* d_out, uint32_t* d_counts) {
    if (!c) return -1;
    const std::string refusal = check_obbs_query(fn, c->sc.nodes != nullptr, batch, k, d_out, d_counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = batch->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = obbs_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const ObbShape os = obbs_shape(n, k, batch->sharedFrame != 0u, RT_BLOCK);
    const bool glist = stack != (uint32_t)RT_BOXES_STACK;
    if (glist && k) {
        if (c->boxesListBuf.bytes < os.listBytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees lists a search in flight may be using
        int rc = dev_alloc(c, c->boxesListBuf, os.listBytes);
        if (rc) return rc;
    }
    const ObbsArgs ba{batch->frames, batch->lo, batch->hi, n, k, batch->sharedFrame, (const float4*)c->objNearBuf.p, (uint4*)d_out, d_counts, (uint32_t*)c->boxesListBuf.p, (DevCounters*)c->aovCounterBuf.p};
    if (glist) launch_obbs_overlap<RT_BOXES_STACK_DEEP, true>(c, os.blocks, ba);
    else launch_obbs_overlap<RT_BOXES_STACK, false>(c, os.blocks, ba);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): frames, lo, hi, out, counts
int obbs_host(rt_ctx* c, const char* fn, const RtObbBatch* batch, uint32_t k, RtOverlap* out, uint32_t* counts) {
    if (!c) return -1;
    const std::string refusal = check_obbs_query(fn, c->sc.nodes != nullptr, batch, k, out, counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = batch->n;
    if (n == 0) return 0;
    const uint32_t shared = batch->sharedFrame;
    const ObbShape os = obbs_shape(n, k, shared != 0u, RT_BLOCK);
    const StagePart parts[] = {{batch->frames, nullptr, os.frameBytes}, {batch->lo, nullptr, os.cornerBytes}, {batch->hi, nullptr, os.cornerBytes}, {nullptr, out, os.outBytes}, {nullptr, counts, os.countBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtObbBatch dev{(const float*)d[0], (const float*)d[1], (const float*)d[2], n, shared};
        return obbs_device(c, fn, &dev, k, (RtOverlap*)d[3], (uint32_t*)d[4]);
    });
}
}  // namespace

extern "C" {
int rt_query_oriented_boxes(rt_ctx* c, const RtObbBatch* d_batch, uint32_t k, RtOverlap* d_out, uint32_t* d_counts) {
    return obbs_device(c, "rt_query_oriented_boxes", d_batch, k, d_out, d_counts);
}
int rt_query_oriented_boxes_host(rt_ctx* c, const RtObbBatch* batch, uint32_t k, RtOverlap* out, uint32_t* counts) {
    return obbs_host(c, "rt_query_oriented_boxes_host", batch, k, out, counts);
}
}  // extern "C"

// ---- triangle queries (tri_queries.h has the checks, the arithmetic and the stack choice; DESIGN.md, "Triangle queries")
namespace {
template <int STACK, bool GLIST>
void launch_tris_overlap(rt_ctx* c, uint32_t blocks, const TrisArgs& ta) {
    hipLaunchKernelGGL((k_tris_overlap<STACK, GLIST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, ta);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_tris_overlap<%d, %s>", STACK, tf(GLIST));
}

// the search; it writes the records itself. The deep search's lists share boxesListBuf with the box queries: the passes run one
// behind the other on the ctx stream, and none keeps anything in it between launches
int tris_device(rt_ctx* c, const char* fn, const RtTriangleBatch* tris, uint32_t k, RtOverlap* d_out, uint32_t* d_counts) {
    if (!c) return -1;
    const std::string refusal = check_tris_query(fn, c->sc.nodes != nullptr, tris, k, d_out, d_counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = tris->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = tris_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const TrisShape ts = tris_shape(n, k, RT_BLOCK);
    const bool glist = stack != (uint32_t)RT_BOXES_STACK;
    if (glist && k) {
        if (c->boxesListBuf.bytes < ts.listBytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees lists a search in flight may be using
        int rc = dev_alloc(c, c->boxesListBuf, ts.listBytes);
        if (rc) return rc;
    }
    const TrisArgs ta{tris->corners, n, k, c->tune.triPlane ? 1u : 0u, (const float4*)c->objNearBuf.p, (uint4*)d_out, d_counts, (uint32_t*)c->boxesListBuf.p, (DevCounters*)c->aovCounterBuf.p};
    if (glist) launch_tris_overlap<RT_BOXES_STACK_DEEP, true>(c, ts.blocks, ta);
    else launch_tris_overlap<RT_BOXES_STACK, false>(c, ts.blocks, ta);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): corners, out, counts
int tris_host(rt_ctx* c, const char* fn, const RtTriangleBatch* tris, uint32_t k, RtOverlap* out, uint32_t* counts) {
    if (!c) return -1;
    const std::string refusal = check_tris_query(fn, c->sc.nodes != nullptr, tris, k, out, counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = tris->n;
    if (n == 0) return 0;
    const TrisShape ts = tris_shape(n, k, RT_BLOCK);
    const StagePart parts[] = {{tris->corners, nullptr, ts.cornerBytes}, {nullptr, out, ts.outBytes}, {nullptr, counts, ts.countBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtTriangleBatch dev{(const float*)d[0], n};
        return tris_device(c, fn, &dev, k, (RtOverlap*)d[1], (uint32_t*)d[2]);
    });
}
}  // namespace

extern "C" {
int rt_query_triangles(rt_ctx* c, const RtTriangleBatch* d_tris, uint32_t k, RtOverlap* d_out, uint32_t* d_counts) {
    return tris_device(c, "rt_query_triangles", d_tris, k, d_out, d_counts);
}
int rt_query_triangles_host(rt_ctx* c, const RtTriangleBatch* tris, uint32_t k, RtOverlap* out, uint32_t* counts) {
    return tris_host(c, "rt_query_triangles_host", tris, k, out, counts);
}
}  // extern "C"

// ---- cut queries (cut_queries.h has the arithmetic and the stack choice, tri_queries.h the checks; DESIGN.md, "Triangle cuts")
namespace {
template <int STACK, bool GLIST>
void launch_tris_cut(rt_ctx* c, uint32_t blocks, const CutsArgs& ca) {
    hipLaunchKernelGGL((k_tris_cut<STACK, GLIST>), dim3(blocks), dim3(RT_BLOCK), 0, c->stream, c->sc, ca);
    snprintf(c->rep.lastKernel, sizeof c->rep.lastKernel, "k_tris_cut<%d, %s>", STACK, tf(GLIST));
}

// the search; it writes the records itself. The deep search's key lists share boxesListBuf with the box and triangle queries
int cuts_device(rt_ctx* c, const char* fn, const RtTriangleBatch* tris, uint32_t k, RtCut* d_out, uint32_t* d_counts) {
    if (!c) return -1;
    const std::string refusal = check_tris_query(fn, c->sc.nodes != nullptr, tris, k, d_out, d_counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = tris->n;
    if (n == 0) return 0;
    std::string deep;
    const uint32_t stack = cuts_stack(fn, c->maxLeafDepth, &deep);
    if (!stack) return c->fail(deep);
    RT_HIP(c, hipSetDevice(c->device));
    const CutsShape cs = cuts_shape(n, k, RT_BLOCK);
    const bool glist = stack != (uint32_t)RT_BOXES_STACK;
    if (glist && k) {
        if (c->boxesListBuf.bytes < cs.listBytes) RT_HIP(c, hipStreamSynchronize(c->stream));   // growing frees lists a search in flight may be using
        int rc = dev_alloc(c, c->boxesListBuf, cs.listBytes);
        if (rc) return rc;
    }
    const CutsArgs ca{tris->corners, n, k, c->tune.triPlane ? 1u : 0u, (const float4*)c->objNearBuf.p, (uint4*)d_out, d_counts, (uint32_t*)c->boxesListBuf.p, (DevCounters*)c->aovCounterBuf.p};
    if (glist) launch_tris_cut<RT_BOXES_STACK_DEEP, true>(c, cs.blocks, ca);
    else launch_tris_cut<RT_BOXES_STACK, false>(c, cs.blocks, ca);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The host-memory form (staged): corners, out, counts
int cuts_host(rt_ctx* c, const char* fn, const RtTriangleBatch* tris, uint32_t k, RtCut* out, uint32_t* counts) {
    if (!c) return -1;
    const std::string refusal = check_tris_query(fn, c->sc.nodes != nullptr, tris, k, out, counts);
    if (!refusal.empty()) return c->fail(refusal);
    const uint32_t n = tris->n;
    if (n == 0) return 0;
    const CutsShape cs = cuts_shape(n, k, RT_BLOCK);
    const StagePart parts[] = {{tris->corners, nullptr, cs.cornerBytes}, {nullptr, out, cs.outBytes}, {nullptr, counts, cs.countBytes}};
    return staged(c, parts, [&](void* const* d) {
        const RtTriangleBatch dev{(const float*)d[0], n};
        return cuts_device(c, fn, &dev, k, (RtCut*)d[1], (uint32_t*)d[2]);
    });
}
}  // namespace

extern "C" {
int rt_query_cuts(rt_ctx* c, const RtTriangleBatch* d_tris, uint32_t k, RtCut* d_out, uint32_t* d_counts) {
    return cuts_device(c, "rt_query_cuts", d_tris, k, d_out, d_counts);
}
int rt_query_cuts_host(rt_ctx* c, const RtTriangleBatch* tris, uint32_t k, RtCut* out, uint32_t* counts) {
    return cuts_host(c, "rt_query_cuts_host", tris, k, out, counts);
}
}  // extern "C"
