// The body of both fused kernels (rt_kernels.hip.h: k_render_fused, k_render_fused_maps), included inside each of them.
// The kernel declares the template parameters STACK, OVF, PIX and CULL (as template parameters or constants), ALPHA (the
// traversal looks triangle hits up in their object's alpha map: alpha_cut) and MAPS (shading reads the metalness and bump
// maps: shade_path<true>), and names its argument `ka`.
// (Text rather than a device function: the early passes of the optimizer run on a device function before it is inlined, and
// with the body in one the k_render_fused instantiations came out different from what they were with it in the kernel —
// other spills, other scratch sizes. These kernels spill heavily and have produced wrong binaries; their code stays put.)

    const DevScene& sc = ka.sc;
    const PathState& ps = ka.ps;
    const FrameParams& fp = ka.fp;
    const FusedArgs& fa = ka.fa;
    __shared__ uint32_t s_stack[(RT_BLOCK / RT_WAVE) * (STACK + 1) * RT_WAVE];
    __shared__ uint32_t s_list[RT_BLOCK / RT_WAVE][3 * RT_WAVE];
    __shared__ float4 s_box[64];  // DevScene::maskBox (the objects of the mask's window that can be ruled out): the rays' object masks are computed from here (reach_mask_from)
    __shared__ uint2 s_meta[RT_META_LDS];
    const uint32_t nBox = CULL ? sc.reachCount : 0u;
    if (CULL && threadIdx.x < 2u * nBox) s_box[threadIdx.x] = sc.maskBox[threadIdx.x];
    fill_meta_lds(sc, s_meta);
    const uint32_t wv = threadIdx.x / RT_WAVE;
    uint32_t* stack = s_stack + wv * (STACK + 1) * RT_WAVE + (threadIdx.x & (RT_WAVE - 1));
    uint32_t* list = s_list[wv];
    uint32_t* ovf = OVF ? fa.overflow + (size_t)blockIdx.x * RT_BLOCK + threadIdx.x : nullptr;
    const size_t ovfStride = (size_t)gridDim.x * RT_BLOCK;
    const TracePwArgs ta{nullptr, nullptr, nullptr, fa.refill, 0u, fa.wSetup, fa.wLeaf, fa.fastLanes, fa.fastShare, nullptr, nullptr, fa.counters, nullptr, nullptr, fa.overflow};
    WaveTotals wt;
    uint32_t refTot = 0, pathTot = 0, segTot = 0, emitTot = 0;
    const unsigned long long tKernelStart = fa.waveTimes ? wall_clock64() : 0ull;
    // scatter = g > 0: batchPixels is a multiple of g and a block is batchPixels / g chunks of g slots, nBatches apart
    const uint32_t nBatches = fa.scatter ? ((fp.nPixels + fa.scatter - 1) / fa.scatter + fa.batchPixels / fa.scatter - 1) / (fa.batchPixels / fa.scatter)
                                         : ((fp.nFrames > 1u ? ((fp.nPixels + 63u) >> 6) * 64u * fp.nFrames : fp.nPixels) + fa.batchPixels - 1) / fa.batchPixels;

    // A lane keeps a pixel until all its samples are done, then resolves it and takes the next one: when `pixelRefill`
    // of the wave's lanes are free (or all of them), the wave reserves that many slots with one atomic. The wave stays
    // populated until the tile runs out, instead of draining to its slowest pixel once per block.
    const uint32_t nSlots = fp.nFrames > 1u ? ((fp.nPixels + 63u) >> 6) * 64u * fp.nFrames : fp.nPixels;  // nFrames > 1 comes with scatter = 0
    const uint32_t total = fa.scatter ? nBatches * fa.batchPixels : nSlots;
    const uint32_t refillAt = min(max(fa.pixelRefill, 1u), fa.batchPixels);
    uint32_t slot = 0;
    bool valid = false, alive = false, exhausted = false;
    uint32_t auxMask = 0;  // bit 0: the pixel's path has a NEE ray in flight, bit 1: a cosine probe
    for (;;) {
        const bool mine = lane_id() < fa.batchPixels && !alive;
        const unsigned long long mF = __ballot(mine);
        const uint32_t take = __popcll(mF);
        if (!exhausted && take >= refillAt) {
            uint32_t base = 0;
            if (lane_id() == 0) base = atomicAdd(fa.batchHead, take);
            base = __shfl(base, 0, RT_WAVE);
            if (base >= total) exhausted = true;
            else if (mine) {
                // Frame constants and the shading tables are re-read from the kernel-argument segment where they are used
                // (the asm makes the pointers opaque, so the loads cannot be hoisted): held across the traversal loop they
                // cost ~60 scalar registers of a kernel that has none to spare.
                const FusedKernArgs* kq = opaque_kernarg<FusedKernArgs>();
                const FrameParams* fq = &kq->fp;
                const DevScene* sq = &kq->sc;
                if (valid && fq->nFrames == 1u) resolve_pixel(ps, *fq, fa.rgba, slot);  // several frames: k_blend_frames, afterwards
                const uint32_t a = base + lanes_below(mF);
                uint32_t ns = a;
                if (fa.scatter) {
                    // a block's pixels are spread over the whole tile (chunks of `scatter` consecutive slots, nBatches chunks
                    // apart), so that all blocks cost about the same when every wave gets just one of them
                    const uint32_t ch = a / fa.scatter, perBlock = fa.batchPixels / fa.scatter;
                    ns = ((ch % perBlock) * nBatches + ch / perBlock) * fa.scatter + a % fa.scatter;
                }
                valid = a < total && ns < nSlots && (fq->nFrames == 1u || slot_in_tile(*fq, ns) < fq->nPixels);
                slot = ns;
                auxMask = 0;
                if (valid) alive = init_path(*sq, ps, *fq, slot) > 0u;  // (0: rt_render_sampled gives the pixel no sample; resolve_pixel leaves it alone)
            }
        }
        const unsigned long long mA = __ballot(alive);
        if (mA == 0) {
            if (exhausted) break;
            continue;
        }
        const unsigned long long mM = __ballot(alive && !(auxMask & 4u));  // bit 2: the kept camera hit stands in for the main ray
        const unsigned long long mL = __ballot(alive && (auxMask & 1u)), mC = __ballot(alive && (auxMask & 2u));
        const uint32_t nM = __popcll(mM), nL = __popcll(mL), nC = __popcll(mC);
        if (alive) {
            if (!(auxMask & 4u)) list[lanes_below(mM)] = (slot << 2) | RAY_MAIN;
            if (auxMask & 1u) list[nM + lanes_below(mL)] = (slot << 2) | RAY_NEE;
            if (auxMask & 2u) list[nM + nL + lanes_below(mC)] = (slot << 2) | RAY_PROBE;
        }
        const uint32_t nRays = nM + nL + nC;
        __threadfence_block();  // the rays written by shade_path / init_path are read by other lanes of this wave
        trace_wave<STACK, OVF, PIX, false, true, CULL, 0, false, ALPHA>(sc, ps, ta, stack, ovf, ovfStride, list, nRays, wt, s_meta);
        __threadfence_block();  // ... and so are the hit records
        if (alive) {
            bool nowAlive = false;
            uint32_t refRays = 0, nPaths = 0;
            const FusedKernArgs* kq = opaque_kernarg<FusedKernArgs>();
            const FrameParams* fq = &kq->fp;
            const DevScene* sq = &kq->sc;
            shade_path<MAPS>(*sq, ps, *fq, slot, nowAlive, auxMask, refRays, nPaths, emitTot, false);
            segTot++;
            if (CULL && nowAlive && nBox) {
                // the new rays' object masks (sphere_seed), here rather than inside shade_path: its registers are spilling already
                float4 sd;
                if (!(auxMask & 4u)) {
                    sd = ps.hit(RAY_MAIN)[slot];
                    sd.z = __uint_as_float(reach_mask_from(s_box, nBox, f4xyz(ps.rayO()[slot]), f4xyz(ps.rayD()[slot]), sc.cullOriginLimit));
                    ps.hit(RAY_MAIN)[slot] = sd;
                }
                if (auxMask & 1u) {
                    sd = ps.hit(RAY_NEE)[slot];
                    sd.z = __uint_as_float(reach_mask_from(s_box, nBox, f4xyz(ps.auxO()[slot]), f4xyz(ps.auxDL()[slot]), sc.cullOriginLimit));
                    ps.hit(RAY_NEE)[slot] = sd;
                }
                if (auxMask & 2u) {
                    sd = ps.hit(RAY_PROBE)[slot];
                    sd.z = __uint_as_float(reach_mask_from(s_box, nBox, f4xyz(ps.auxO()[slot]), f4xyz(ps.auxDC()[slot]), sc.cullOriginLimit));
                    ps.hit(RAY_PROBE)[slot] = sd;
                }
            }
            alive = nowAlive;
            auxMask = nowAlive ? auxMask : 0u;
            refTot += refRays;
            pathTot += nPaths;
        }
    }
    if (valid) {  // the pixels that finished after the tile ran out
        const FusedKernArgs* kq = opaque_kernarg<FusedKernArgs>();
        if (kq->fp.nFrames == 1u) resolve_pixel(ps, kq->fp, fa.rgba, slot);
    }

    if (fa.waveTimes && lane_id() == 0) {  // phase_stats: when did this wave run out of blocks?
        const size_t w = (size_t)blockIdx.x * (RT_BLOCK / RT_WAVE) + threadIdx.x / RT_WAVE;
        fa.waveTimes[2 * w] = tKernelStart;
        fa.waveTimes[2 * w + 1] = wall_clock64();
    }
    unsigned long long wb = wave_sum_u64(wt.totBox), wtri = wave_sum_u64(wt.totTri);
    uint32_t wr = wave_sum_u32(wt.totRays), wh = wave_sum_u32(wt.totHits);
    uint32_t wRef = wave_sum_u32(refTot), wP = wave_sum_u32(pathTot), wS = wave_sum_u32(segTot), wE = wave_sum_u32(emitTot);
    const unsigned long long wskip = CULL ? wave_sum_u64(wt.totSkipBox) : 0ull;
    if (lane_id() == 0 && (wr | wP | wS)) {
        if (CULL && wskip) atomicAdd(&fa.counters->skippedBoxTests, wskip);
        if (wE) atomicAdd(&fa.counters->emitterTests, (unsigned long long)wE);
        atomicAdd(&fa.counters->boxTests, wb);
        atomicAdd(&fa.counters->triTests, wtri);
        atomicAdd(&fa.counters->raysTraced, (unsigned long long)wr);
        atomicAdd(&fa.counters->raysHit, (unsigned long long)wh);
        atomicAdd(&fa.counters->raysReference, (unsigned long long)wRef);
        atomicAdd(&fa.counters->paths, (unsigned long long)wP);
        atomicAdd(&fa.counters->segments, (unsigned long long)wS);
    }
