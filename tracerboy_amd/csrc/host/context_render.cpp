/* context_render.cpp -- TracerBoy::Render x n frames (the reference's TracerBoy.cpp:2677-2946) as launches of the path-tracing
 * kernels: renderImpl, at the end of the file, is the list of a call's steps.  They execute the plan launch_plan.h makes (pipeline, copy of
 * the feature set, split stack, pre-pass, batches and frame groups), ask the two trials no rule could replace (launch_trials.h) and dispatch to
 * the pipelines; frame-group mode and the split-role pipeline share one executor (FrameGroupExec). */
#include "context_internal.h"
#include "tb_vec.h"

namespace tbctx {

bool historyRelevantChange(const tb_output_settings& a, const tb_output_settings& b) /* TracerBoy.cpp:2163-2185 */
{
    return a.OutputType != b.OutputType || a.EnableNormalMaps != b.EnableNormalMaps || a.RenderModeRealTime != b.RenderModeRealTime ||
           a.DOFFocalDistance != b.DOFFocalDistance || a.ApertureWidth != b.ApertureWidth || a.FilterType != b.FilterType || a.FilterWidth != b.FilterWidth ||
           a.FireflyClampValue != b.FireflyClampValue || a.EnableNextEventEstimation != b.EnableNextEventEstimation ||
           a.EnableSamplingImportanceResampling != b.EnableSamplingImportanceResampling || a.EnableBlueNoise != b.EnableBlueNoise ||
               a.MaxBounces != b.MaxBounces ||
           a.DebugValue != b.DebugValue || a.DebugValue2 != b.DebugValue2;
}

/* Wavefront pipeline (option "pipeline" = 2): frames are processed in batches of as many frames as fit the path
 * budget; per batch: generate+extend, then MaxBounces x (shade, connect, extend), then the ordered accumulation.
 * Every launch is a fixed-size grid-stride kernel reading its queue length from device memory: no host sync inside. */
void renderWavefront(tb_context* c, int variant, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t n, TbPerFrameConstants pf)
{
    const uint64_t pixels = (uint64_t)W * H;
    const uint64_t perFrame = (uint64_t)((W + 7) / 8) * ((H + 7) / 8) * 64; /* sample ids walk whole 8x8 tiles (wf_sample_pixel) */
    const uint64_t budget = (uint64_t)opt<OPT_wavefront_paths>(c);
    const uint32_t segCap = (uint32_t)std::max<int64_t>(256, opt<OPT_wavefront_segment>(c));
    uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, budget / perFrame));
    const uint64_t maxSegments = (perFrame * batch + segCap - 1) / segCap;
    const uint64_t capacity = maxSegments * segCap;
    if (capacity > 0xffffff00ull) throw std::runtime_error("wavefront batch exceeds 2^32 paths");
    {   /* the LDS a stage asks for, checked here so that a large segment fails with a sentence instead of a launch error */
        const size_t blobBytes = c->sceneInLds ? c->ds.ldsBlobBytes : 0, ldsLimit = 160 * 1024;
        if (opt<OPT_wavefront_sort>(c)) {
            if (segCap > 65536u)
                throw std::runtime_error("wavefront_sort: wavefront_segment must not exceed 65536 (the index permutation is 16-bit); unsupported");
            const size_t sortBytes = 64 * 4 + ((size_t)segCap * 3 + 15) / 16 * 16;
            if (16 + blobBytes + sortBytes > ldsLimit) throw std::runtime_error("wavefront_sort: a segment of " + std::to_string(segCap) + " entries needs " +
                std::to_string(16 + blobBytes + sortBytes) + " B of LDS (limit 163840): lower wavefront_segment; unsupported");
        }
        if (16 + (size_t)c->ds.stackDepth * 1024 + blobBytes > ldsLimit) throw std::runtime_error("wavefront pipeline: traversal stack of depth " +
            std::to_string(c->ds.stackDepth) + " does not fit LDS; unsupported");
    }
    const bool sss = (kVariants[variant].features() & PT_FEAT_SSS) != 0; /* entries may be steps of the interior walk: two more columns per queue */
    {
        for (int q = 0; q < 2; q++) for (int k = 0; k < (sss ? 6 : 4); k++) ensure(c->wfCols[q][k], capacity * 16);
        for (int k = 0; k < (sss ? 12 : 11); k++) if (sss || k != 8) ensure(c->wfShadowCols[k], capacity * 16); /* column i (8) and l (11): FEAT_SSS only */
        ensure(c->wfHitA, capacity * 16); ensure(c->wfHitG, capacity * 4);
        ensure(c->wfSamples, pixels * batch * 16);
        ensure(c->wfCounts, maxSegments * 3 * 4);
        c->wfCapacity = capacity;
    }
    WfQueue E[2], S; memset(E, 0, sizeof E); memset(&S, 0, sizeof S);
    for (int q = 0; q < 2; q++) {
        E[q].a = (float4*)c->wfCols[q][0].p; E[q].b = (float4*)c->wfCols[q][1].p; E[q].c = (float4*)c->wfCols[q][2].p; E[q].d = (float4*)c->wfCols[q][3].p;
        E[q].e = (float4*)c->wfCols[q][4].p; E[q].f = (float4*)c->wfCols[q][5].p;
    }
    float4** sc[12] = {&S.a, &S.b, &S.c, &S.d, &S.e, &S.f, &S.g, &S.h, &S.i, &S.j, &S.k, &S.l};
    for (int k = 0; k < 12; k++) *sc[k] = (float4*)c->wfShadowCols[k].p;
    /* per-segment fill counts; every stage writes the counts of all segments of its output queues, so no clearing */
    E[0].segCount = (uint32_t*)c->wfCounts.p; E[1].segCount = E[0].segCount + maxSegments; S.segCount = E[1].segCount + maxSegments;
    WfHits hits; hits.tuv_prim = (float4*)c->wfHitA.p; hits.geom = (uint32_t*)c->wfHitG.p;
    const wf_variant_fn fn = kVariants[variant].wf;
    const uint32_t gridOpt = (uint32_t)opt<OPT_wavefront_grid>(c);
    const uint32_t depth = pf.MaxBounces;
    std::vector<uint32_t> counts;
    for (uint32_t f0 = 0; f0 < n; f0 += batch) {
        const uint32_t nf = std::min(batch, n - f0);
        WfParams wp; memset(&wp, 0, sizeof wp);
        wp.W = W; wp.H = H; wp.firstFrame = firstFrame + f0; wp.numFrames = nf; wp.tiles = c->tiles;
        wp.samples = (float4*)c->wfSamples.p;
        wp.segCapacity = segCap; wp.numSegments = (uint32_t)((perFrame * nf + segCap - 1) / segCap);
        wp.sortByMaterial = opt<OPT_wavefront_sort>(c) ? 1u : 0u;
        wp.refillBelow = (uint32_t)std::min<int64_t>(64, std::max<int64_t>(0, opt<OPT_wavefront_refill>(c)));
        const uint32_t grid = std::min(gridOpt, wp.numSegments);
        const int lds = c->sceneInLds ? 1 : 0;
        HIP_TRY(fn(c->stream, WF_STAGE_GENERATE_EXTEND, &c->ds, &pf, &wp, nullptr, nullptr, &E[0], &hits, lds, nullptr, nullptr, grid));
        /* One round = one ray per live path.  Without SSS a path casts one extension ray per bounce, so MaxBounces rounds empty the
         * queues.  With SSS every step of an interior walk is a round of its own (up to 100 per bounce, kernel.glsl:1565): past the
         * first MaxBounces rounds the host reads the segment counts back before each round and stops when nothing is left. */
        for (uint32_t b = 0; depth > 0; b++) {
            const WfQueue& in = E[b & 1]; const WfQueue& next = E[(b + 1) & 1];
            HIP_TRY(fn(c->stream, WF_STAGE_SHADE, &c->ds, &pf, &wp, &in, &S, &next, &hits, lds, nullptr, nullptr, grid));
            HIP_TRY(fn(c->stream, WF_STAGE_CONNECT, &c->ds, &pf, &wp, nullptr, &S, &next, &hits, lds, nullptr, nullptr, grid));
            if (!sss && b + 1 >= depth) break;
            /* SSS: past the first MaxBounces rounds the queues are looked at every FOURTH round only (a round over empty queues is a
             * few no-op launches; a look is a copy + a wait of the host, which used to serialise host and device once per round) */
            if (sss && b + 1 >= depth && ((b + 1 - depth) & 3u) == 0u) {
                counts.resize(wp.numSegments);
                HIP_TRY(hipMemcpyAsync(counts.data(), next.segCount, (size_t)wp.numSegments * 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                uint64_t live = 0; for (uint32_t v : counts) live += v;
                if (live == 0) break;
                if (b > depth * 101u + 8u) throw std::runtime_error("wavefront pipeline: paths still alive after MaxBounces x 101 rounds");
            }
            HIP_TRY(fn(c->stream, WF_STAGE_EXTEND, &c->ds, &pf, &wp, nullptr, nullptr, &next, &hits, lds, nullptr, nullptr, grid));
        }
        HIP_TRY(fn(c->stream, WF_STAGE_ACCUMULATE, &c->ds, &pf, &wp, nullptr, nullptr, nullptr, &hits, lds, (TbFloat4*)c->output.p, (TbFloat4*)c->jittered.p,
            gridOpt));
    }
}

/* Pooled pipeline (option "pipeline" = 3, pt_pooled.inc): one persistent launch per batch of frames, then the ordered
 * accumulation of the batch's sample buffer. */
void renderPooled(tb_context* c, int variant, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t n, TbPerFrameConstants pf)
{
    const uint64_t pixels = (uint64_t)W * H;
    const uint64_t budget = (uint64_t)opt<OPT_pooled_samples>(c); /* sample buffer entries (16 B each) */
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, budget / pixels));
    if (pixels * batch > 0xffffff00ull) throw std::runtime_error("pooled batch exceeds 2^32 samples");
    ensure(c->wfSamples, pixels * batch * 16);
    const wf_variant_fn fn = kVariants[variant].wf;
    const uint32_t blocks = tb_persistent_grid(W, H, c->tiles);
    if (blocks == 0) return; /* this rank owns no tile */
    for (uint32_t f0 = 0; f0 < n; f0 += batch) {
        WfParams wp; memset(&wp, 0, sizeof wp);
        wp.W = W; wp.H = H; wp.firstFrame = firstFrame + f0; wp.numFrames = std::min(batch, n - f0); wp.tiles = c->tiles;
        wp.samples = (float4*)c->wfSamples.p;
        wp.pathsPerLane = (uint32_t)opt<OPT_pooled_paths>(c);
        if (opt<OPT_pooled_profile>(c)) { /* counting variant: wave-occupancy slots, read back with tb_read_wave_profile */
            ensure(c->rayStats, 21 * 8);
            if (firstFrame + f0 == 0) HIP_TRY(hipMemsetAsync(c->rayStats.p, 0, 21 * 8, c->stream));
            wp.prof = (unsigned long long*)c->rayStats.p + 7;
        }
        const int lds = c->sceneInLds ? 1 : 0;
        HIP_TRY(fn(c->stream, WF_STAGE_POOLED, &c->ds, &pf, &wp, nullptr, nullptr, nullptr, nullptr, lds, nullptr, nullptr, blocks));
        HIP_TRY(fn(c->stream, WF_STAGE_ACCUMULATE, &c->ds, &pf, &wp, nullptr, nullptr, nullptr, nullptr, lds, (TbFloat4*)c->output.p, (TbFloat4*)c->jittered.p,
            2048));
    }
}

/* compute units of the context's device, asked once */
int deviceCUs(tb_context* c)
{
    if (!c->numCUs && hipDeviceGetAttribute(&c->numCUs, hipDeviceAttributeMultiprocessorCount,
        c->device) != hipSuccess) throw std::runtime_error("hipDeviceGetAttribute(multiprocessor count) failed");
    return c->numCUs;
}

/* the split-role kernel's abort word and the state the wave that raised it left behind (pt_split.inc give_up); clears the word */
std::string splitAbortMessage(tb_context* c, bool clear)
{
    volatile uint32_t* w = c->splitAbort;
    char buf[512];
    static const char* why[] = {"?", "a traversal wave found nothing to walk", "a shading wave waited for hits", "a queue position stayed full"};
    snprintf(buf, sizeof buf,
        "the split-role kernel gave up (%s for spin_limit sleeps; workgroup %u wave %u; state %u %u 0x%x 0x%x; tickets %u, positions %u, shading waves done %u); the frame is incomplete",
             why[w[0] < 4 ? w[0] : 0], w[1] >> 8, w[1] & 255u, w[2], w[3], w[4], w[5], w[6], w[7], w[8]);
    if (clear) for (int i = 0; i < 9; i++) w[i] = 0; /* a query that is not the end of a render (tb_accum_device_ptr) reports and leaves the report for tb_sync */
    return buf;
}

/* the split-role kernel's workgroup shape and thresholds from the options (everything but the abort word and the profile pointer) */
static void splitParamsFromOptions(tb_context* c, TbSplitParams& sp)
{
    memset(&sp, 0, sizeof sp);
    sp.travWaves = (uint32_t)std::max<int64_t>(1, opt<OPT_split_trav>(c)); sp.shadeWaves = (uint32_t)opt<OPT_split_shade>(c);
    if (!sp.shadeWaves) sp.shadeWaves = c->sceneInLds ? 4 : 6; /* 0 = the default for the kind of scene */
    sp.readyMin = (uint32_t)opt<OPT_split_ready>(c); sp.refillMin = (uint32_t)std::max<int64_t>(1, opt<OPT_split_refill>(c));
    sp.innerWeight = (uint32_t)std::max<int64_t>(1, opt<OPT_split_wi>(c)); sp.leafWeight = (uint32_t)std::max<int64_t>(1, opt<OPT_split_wl>(c));
    sp.travLast = opt<OPT_split_trav_last>(c) ? 1u : 0u; sp.shadePrio = opt<OPT_split_shade_prio>(c) ? 1u : 0u;
    sp.ringCap = 256; while (sp.ringCap < 256u * sp.shadeWaves) sp.ringCap *= 2;
    sp.spinLimit = (uint32_t)opt<OPT_split_spin_limit>(c);
}

/* the pixels of the frame a context renders: all of them, or those of its tiles (tile t of a row-major grid belongs to rank t % world) */
static uint64_t ownedFramePixels(uint32_t W, uint32_t H, const TbTileMap& t)
{
    if (t.world <= 1) return (uint64_t)W * H;
    const uint32_t tilesX = (W + t.tileW - 1) / t.tileW, tilesY = (H + t.tileH - 1) / t.tileH;
    uint64_t n = 0;
    for (uint32_t i = t.rank; i < tilesX * tilesY; i += t.world)
        n += (uint64_t)std::min(t.tileW, W - (i % tilesX) * t.tileW) * std::min(t.tileH, H - (i / tilesX) * t.tileH);
    return n;
}

/* What the steps of one render call share (renderImpl, below, is the list of the steps). */
struct RenderCall {
    tb_context* c; uint32_t W, H, n; tb_output_settings s; float timeSeed; bool sync;
    bool aov, count, adaptive, perCall /* option adaptive_test = 1 */, clearStats; int64_t adaptiveMin, pipe;
    bool budgeted, skipTest; /* planned under a sample budget; ... whose list pass applies the adaptive skip test too */
    TbPerFrameConstants pf; TbDeviceTargets tg;
    const Variant* v; int variantIndex; bool twoLevel; tb_plan_input pin; tb_launch_plan plan;
    bool wavefront, pooled, split, groups; /* of the first plan (a plan made again for layout C changes none of them) */
    const Copy* copy; int mode; TbDeviceScene dsLaunch; size_t overflowHalf; /* the copy of the feature set and how it is asked to run (PtMode), the scene as it sees it, words per half of the split stack */
    bool prepass, firstBounce, compactHits, overlap; uint32_t hitPrimBits, stampBits; size_t hitRecordBytes;
    /* The stamp of compact hit records is cyclic: with s = 32 - hitIndexBits bits it repeats every 2^s - 1 launches (15 at the 4-bit minimum; a buffer
     * sees every second launch, so a record as a launch 30 launches ago left it on the same buffer would pass -- every launch in between has rewritten
     * every record of the buffer, and what was actually observed, a line of the launch before last, differs in its stamp at any width).  There is no
     * check word: a 16-B piece is written and read whole. */
    /* a key per (copy, mode) for the trials and the warm-ups: the launcher's address, and a bit for the adaptive launch, whose kernels are others */
    uintptr_t launchKey() const { return (uintptr_t)copy->launch ^ (mode == PT_MODE_ADAPTIVE ? ~(~(uintptr_t)0 >> 1) : 0); }
    uint32_t hitStampOf(uint32_t epoch) const { return compactHits ? 1u + epoch % ((1u << stampBits) - 1u) : 0u; }
};

/* the scene as the launch on side stream `par` sees it: its own half of the split stack (consecutive launches overlap on the two side streams) */
static TbDeviceScene sceneOfSide(TbDeviceScene ds, uint32_t par, size_t overflowHalf) { if (ds.stackOverflow) ds.stackOverflow += par * overflowHalf; return ds; }

/* Frame-group execution, the host side of the lock-step kernels' frame-group mode (renderFrameGroups) and of the split-role pipeline
 * (renderSplit): batches of frames go into one of two ordered sample buffers, launches alternate between the two side streams so that a
 * launch starts while the one before drains, and a fold takes each batch into the surfaces in frame order on the main stream.
 * overlap = false: everything on the main stream, no events.  Stream of every enqueue: launchStream(par) unless it says c->stream. */
struct FrameGroupExec {
    tb_context* c; TbDeviceTargets& tg; bool overlap;
    hipStream_t launchStream(uint32_t par) const { return overlap ? c->side[par] : c->stream; }
    TbDeviceTargets targetsOfSide(uint32_t par) const { TbDeviceTargets t = tg; t.samples = (TbFloat4*)c->fgSamples[par].p;
        t.workCounter = (uint32_t*)c->workCounter.p + par * 128u; return t; }
    /* a buffer of side `par` that only grows: before it is replaced nobody may read the old one any more; touch: a fresh allocation is mapped lazily */
    void grow(DevBuf& b, uint32_t par, size_t bytes, bool touch) const
    {
        if (b.bytes >= bytes) return;
        HIP_TRY(hipStreamSynchronize(c->side[par])); HIP_TRY(hipStreamSynchronize(c->stream));
        ensure(b, bytes);
        if (touch) HIP_TRY(hipMemsetAsync(b.p, 0, bytes, launchStream(par)));
    }
    /* the first overlapped launch after other work on the main stream orders the side streams behind it, once; both sample buffers are sized -- and
     * touched -- by the first call that needs them, not by the call that first reaches the second one */
    void begin(size_t sampleBytes) const
    {
        ensure(c->workCounter, 1024);
        if (!overlap) c->sideOrdered = false;
        else if (!c->sideOrdered) {
            HIP_TRY(hipEventRecord(c->evMain, c->stream));
            for (int i = 0; i < 2; i++) HIP_TRY(hipStreamWaitEvent(c->side[i], c->evMain, 0));
            c->sideOrdered = true;
        }
        for (uint32_t par = 0; par < 2u; par++) grow(c->fgSamples[par], par, sampleBytes, true);
    }
    /* the first render with a kernel (`key`) sends a launch without frames down BOTH side streams, so that whatever the runtime sets up at a queue's
     * first dispatch of it (scratch: milliseconds, once per stream) falls into this call and not into whichever later call reaches the second stream */
    template <class Warm> void warmOnce(const void* key, Warm warm) const
    {
        if (std::find(c->warmedLaunchers.begin(), c->warmedLaunchers.end(), key) != c->warmedLaunchers.end()) return;
        for (uint32_t par = 0; par < 2u; par++) warm(par);
        c->warmedLaunchers.push_back(key);
    }
    /* the batches of a call: prepare(nf, par, stream) what the launch needs (before the wait: it may enqueue), launch(f0, nf, par, stream) into
     * tg.samples, fold(f0, nf) on the main stream.  clearStats: the stats words, on the stream of the first launch */
    template <class Prepare, class Launch, class Fold> void run(uint32_t n, uint32_t batch, bool clearStats, Prepare prepare, Launch launch, Fold fold) const
    {
        for (uint32_t f0 = 0; f0 < n; f0 += batch) {
            const uint32_t nf = std::min(batch, n - f0), par = c->fgLaunch++ & 1u;
            hipStream_t ptStream = launchStream(par);
            tg.samples = (TbFloat4*)c->fgSamples[par].p; tg.workCounter = (uint32_t*)c->workCounter.p + par * 128u; c->lastFgPar = (int)par;
            prepare(nf, par, ptStream);
            if (overlap) HIP_TRY(hipStreamWaitEvent(ptStream, c->evFold[par], 0)); /* the fold that last read this sample buffer */
            if (f0 == 0) { if (clearStats && overlap) HIP_TRY(hipMemsetAsync(c->stats.p, 0, 16, ptStream));
                HIP_TRY(hipEventRecord(c->evKernelStart, ptStream)); }
            launch(f0, nf, par, ptStream); /* the launch before may still be draining on the other stream */
            if (f0 == 0) { HIP_TRY(hipEventRecord(c->evKernel, ptStream)); c->lastKernelFrames = nf; }
            if (overlap) { HIP_TRY(hipEventRecord(c->evPt[par], ptStream)); HIP_TRY(hipStreamWaitEvent(c->stream, c->evPt[par], 0)); }
            fold(f0, nf);
            if (overlap) HIP_TRY(hipEventRecord(c->evFold[par], c->stream));
        }
    }
};

/* the scene a split-role launch sees: layout B, and with option split_stack_cap below a deeper tree's depth only that many stack entries in LDS
 * (the rest in global memory, pt_scene.h; `overflow` stands for the buffer where only WHICH kernel is asked) */
static TbDeviceScene splitScene(tb_context* c, uint32_t* overflow, uint32_t lanes)
{
    TbDeviceScene ds = c->ds; ds.nodesC = nullptr; ds.stackOverflow = nullptr; ds.stackOverflowLanes = 0;
    const int64_t cap = opt<OPT_split_stack_cap>(c);
    if (cap > 0 && (uint32_t)cap < c->ds.stackDepth && !c->sceneInLds) { ds.stackDepth = (uint32_t)cap; ds.stackOverflow = overflow; ds.stackOverflowLanes = lanes; }
    return ds;
}

/* Would pt_launch_split_* take this call?  Asked of the launcher itself (its query form launches nothing): besides what PlanLaunch can
 * see -- LDS per workgroup, the number of 8x8 tiles -- it refuses a workgroup shape of which not one fits a CU by registers. */
static bool splitLaunchable(const RenderCall& r)
{
    tb_context* c = r.c;
    if (!r.v->split) return false;
    TbSplitParams sp; splitParamsFromOptions(c, sp);
    const TbDeviceScene dsProbe = splitScene(c, (uint32_t*)16, 0xffffffffu);
    TbDeviceTargets probe; memset(&probe, 0, sizeof probe); probe.samples = (TbFloat4*)16; probe.workCounter = (uint32_t*)16; probe.frameGroup = 1;
    int perCU = 0;
    return r.v->split(c->stream, &dsProbe, &r.pf, &probe, &sp, r.W, r.H, 0, 1, &c->tiles, c->sceneInLds ? 1 : 0, &perCU) == hipSuccess;
}

/* Split-role pipeline (option "pipeline" = 4, pt_split.inc): workgroups of traversal waves + shading waves over an LDS ray queue, executed as
 * frame groups (FrameGroupExec), accumulate_samples_kernel folding each batch.  Options: split_trav / split_shade (waves of either role per
 * workgroup), split_ready, split_refill, split_wi / split_wl (TbSplitParams), split_frame_group (frames of a wave's work item), split_stack_cap. */
static void renderSplit(const RenderCall& r)
{
    tb_context* c = r.c; const uint32_t W = r.W, H = r.H, n = r.n; const TbPerFrameConstants& pf = r.pf; TbDeviceTargets tg = r.tg;
    const uint64_t pixels = (uint64_t)W * H, budget = (uint64_t)opt<OPT_pooled_samples>(c);
    uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n, 32768), budget / pixels));
    batch = (n + (n + batch - 1) / batch - 1) / ((n + batch - 1) / batch); /* equal batches */
    const int lds = c->sceneInLds ? 1 : 0;
    TbSplitParams sp; splitParamsFromOptions(c, sp);
    HIP_TRY(hipHostGetDevicePointer((void**)&sp.abortFlag, c->splitAbort.create(64), 0));
    if (opt<OPT_split_profile>(c)) { /* counting copy: 16 counters, cleared with the history, read back with tb_read_split_profile */
        ensure(c->splitProf, 16 * 8);
        if (c->samplesRendered == 0) HIP_TRY(hipMemsetAsync(c->splitProf.p, 0, 16 * 8, c->stream));
        sp.prof = (unsigned long long*)c->splitProf.p;
    }
    const pt_split_fn fn = r.v->split;
    TbDeviceScene dsL = splitScene(c, (uint32_t*)16, 0xffffffffu);
    size_t overflowHalf = 0;
    if (dsL.stackOverflow) { /* how many workgroups per CU: the split-stack kernel's own answer */
        TbDeviceTargets probe = tg; probe.samples = (TbFloat4*)16; probe.workCounter = (uint32_t*)16; probe.frameGroup = 1;
        int perCU = 0;
        HIP_TRY(fn(c->stream, &dsL, &pf, &probe, &sp, W, H, 0, 1, &c->tiles, 0, &perCU));
        const uint32_t over = c->ds.stackDepth - dsL.stackDepth, lanes = (uint32_t)std::max(perCU, 1) * (uint32_t)deviceCUs(c) * sp.travWaves * 64u;
        ensure(c->stackOverflow, (size_t)over * lanes * 4 * 2); /* two halves, one per side stream */
        overflowHalf = (size_t)over * lanes;
        dsL = splitScene(c, (uint32_t*)c->stackOverflow.p, lanes);
    }
    tg.frameGroup = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(opt<OPT_split_frame_group>(c), std::min(batch, n)));
    while ((std::min(batch, n) + tg.frameGroup - 1) / tg.frameGroup > 4095u) tg.frameGroup *= 2; /* a claimed item is group << 20 | tile */
    tg.bandedItems = (uint32_t)opt<OPT_banded_items>(c);
    /* (the stats words were cleared on the main stream, if the plan does not overlap, which the side streams are ordered behind) */
    FrameGroupExec ex{c, tg, opt<OPT_overlap_launches>(c) != 0};
    ex.begin(pixels * batch * 16);
    const void* key = (const void*)((uintptr_t)fn ^ (dsL.stackOverflow ? 2u : 0u) ^ (lds ? 4u : 0u));
    if (ex.overlap) ex.warmOnce(key, [&](uint32_t par) {
        const TbDeviceTargets warm = ex.targetsOfSide(par); const TbDeviceScene dsPar = sceneOfSide(dsL, par, overflowHalf);
        HIP_TRY(fn(c->side[par], &dsPar, &pf, &warm, &sp, W, H, c->samplesRendered, 0, &c->tiles, lds, nullptr));
    });
    ex.run(n, batch, false, [](uint32_t, uint32_t, hipStream_t) {},
        [&](uint32_t f0, uint32_t nf, uint32_t par, hipStream_t st) { const TbDeviceScene dsPar = sceneOfSide(dsL, par, overflowHalf);
            HIP_TRY(fn(st, &dsPar, &pf, &tg, &sp, W, H, c->samplesRendered + f0, nf, &c->tiles, lds, nullptr)); },
        [&](uint32_t f0, uint32_t nf) {
            HIP_TRY(pt_launch_accumulate_samples(c->stream, tg.samples, W, H, c->samplesRendered + f0, nf, &c->tiles, tg.output, tg.jittered)); });
    c->lastSplitWaves = (int)(sp.travWaves * 100 + sp.shadeWaves);
}

/* Frame-group mode of the lock-step kernels (TbDeviceTargets::samples, pt_scene.h): the frames of a batch are cut into groups, workgroup
 * (group, region) renders its 256 pixels x G frames drawing (pixel, frame) pairs from a counter in LDS, every sample goes to an ordered sample
 * buffer and accumulate_samples_kernel folds them in frame order (bit-identical sums).  Keeps all lanes of a workgroup busy to its end and gives
 * a rank of a tile split enough workgroups; on whenever a call renders enough frames to form groups (launch_plan.h, with the batch and group
 * sizes and the measurements they come from).  Option "frame_group" = G > 0 forces the group size, < 0 forbids the mode. */
static void renderFrameGroups(RenderCall& r)
{
    tb_context* c = r.c; const uint32_t W = r.W, H = r.H; const TbPerFrameConstants& pf = r.pf; TbDeviceTargets& tg = r.tg;
    const tb_launch_plan& plan = r.plan; const pt_variant_fn launch = r.copy->launch; const int lds = c->sceneInLds ? 1 : 0, numCUs = deviceCUs(c);
    const uint64_t pixels = (uint64_t)W * H;
    const uint32_t batch = plan.batch_frames;
    const uint64_t regions = std::max<uint64_t>(1, tb_persistent_grid(W, H, c->tiles));
    if (regions > 0xfffffu) throw std::runtime_error("frame too large for the frame-group launch (more than 2^20 16x16 regions)");
    if (plan.costly_first) { /* the counts: cleared when the scene, the frame size or the tile split changes (they are hints: nobody waits for the memset) */
        const uint64_t key = ((uint64_t)c->sceneGeneration << 40) ^ ((uint64_t)W << 20) ^ (uint64_t)H ^ ((uint64_t)c->tiles.world << 60) ^ ((uint64_t)c->tiles.rank << 56);
        if (!c->regionCost.p) ensure(c->regionCost, 4u << 20);
        if (c->regionCostKey != key) { HIP_TRY(hipMemsetAsync(c->regionCost.p, 0, 4u << 20, c->stream)); c->regionCostKey = key; c->sideOrdered = false; }
    }
    tg.bandedItems = (uint32_t)opt<OPT_banded_items>(c);
    /* (an adaptive frame-group launch: frameGroup and workCounter take the storage of the one-pixel-per-lane form's threshold and count pointer,
     * pt_scene.h; the list pointer stays, in regionOrder's place) */
    const uint32_t* const liveList = r.adaptive ? tg.liveList : nullptr;
    tg.frameGroup = plan.frame_group; tg.fgGuided = plan.guided_groups;
    uint32_t lgGroup = 0; while ((2u << lgGroup) <= tg.frameGroup) lgGroup++;
    FrameGroupExec ex{c, tg, r.overlap};
    ex.begin(pixels * batch * 16);
    /* a zero-frame launch of the frame-group form of `launch` itself down one side stream (resident grid of workgroups that find the
     * list empty), with or without the hit records of the pre-pass; it waits for the launch */
    auto warmFrameGroupForm = [&](uint32_t par, bool withHits) {
        TbDeviceTargets warm = ex.targetsOfSide(par);
        if (c->fgSlotLog[par].bytes < 16ull * numCUs * 16 * 8) ensure(c->fgSlotLog[par], 16ull * numCUs * 16 * 8);
        warm.slotLog = (unsigned long long*)c->fgSlotLog[par].p; warm.slotLogCap = 16; warm.launchEpoch = ++c->launchEpoch;
        warm.primaryHits = withHits ? (unsigned long long*)c->fgHits[par].p : nullptr; warm.firstBounce = withHits && r.firstBounce ? 1u : 0u;
        warm.hitStamp = withHits ? r.hitStampOf(warm.launchEpoch) : 0u; warm.hitPrimBits = r.hitPrimBits; warm.hitGeomBits = c->hitGeomBits;
        const TbDeviceScene dsPar = sceneOfSide(r.dsLaunch, par, r.overflowHalf);
        HIP_TRY(launch(ex.launchStream(par), &dsPar, &pf, &warm, W, H, c->samplesRendered, 0, &c->tiles, withHits ? 0 : lds, 0, PT_MODE_LOCKSTEP));
        HIP_TRY(hipStreamSynchronize(ex.launchStream(par)));
    };
    /* The kernel copies held to an occupancy keep a few registers in scratch: the first render with a given kernel sends a zero-frame launch
     * of its one-pixel-per-lane form (same feature set, at least as much scratch, a full grid of workgroups that exit at once; nobody waits for
     * it) down both side streams.  Two-level scenes in the tuned copies have no one-pixel-per-lane form (pt_variant.inc refuses it: the first
     * render of an instanced scene in a fresh context used to fail here and then for good): they are warmed with the frame-group form
     * itself, and so is a copy for scenes in LDS, which has no other form. */
    if (ex.overlap) ex.warmOnce((const void*)r.launchKey(), [&](uint32_t par) {
        if (r.twoLevel || r.copy->row->role == PT_ROLE_LDS_GROUPS) return warmFrameGroupForm(par, false);
        TbDeviceTargets none = tg; none.samples = nullptr;
        TbDeviceScene dsWarm = c->ds; dsWarm.nodesC = nullptr; /* the one-pixel-per-lane twin fetches layout B */
        HIP_TRY(launch(c->side[par], &dsWarm, &pf, &none, W, H, c->samplesRendered, 0, &c->tiles, lds, 0, PT_MODE_LOCKSTEP));
    });
    if (r.prepass) {
        /* the hit records: sized and touched once like the sample buffers; and the kernels that take their first hits from them
         * keep more registers in scratch than the twin the warm-up above runs (sss: 464 against 416 B per lane), so they are
         * run once themselves, with no frames, down both side streams -- a queue whose scratch has to grow under a dispatch
         * that follows another kernel closely gave one wrong 16x16 region in the first render of 1 process in ~3 000 */
        for (uint32_t par = 0; par < 2u; par++) ex.grow(c->fgHits[par], par, pixels * batch * r.hitRecordBytes, true);
        /* one kernel per (split stack, node layout) */
        const void* key = (const void*)(r.launchKey() ^ (1u | (r.dsLaunch.stackOverflow ? 2u : 0u) | (r.dsLaunch.nodesC ? 4u : 0u) | (r.firstBounce ? 8u : 0u)));
        ex.warmOnce(key, [&](uint32_t par) { warmFrameGroupForm(par, true); });
    }
    ex.run(r.n, batch, r.clearStats,
        [&](uint32_t nf, uint32_t par, hipStream_t ptStream) {
            /* slot logs: 16 workgroups per CU at most (2 x residency of 8); a row has room for 8x a workgroup's fair share of the launch's
             * items at the SMALLEST resident grid the launcher may choose (2 per CU), so that the rows of any grid hold the whole list
             * several times over and a workgroup whose row is full (it retires) never strands work */
            const uint64_t numGroups = tb_fg_groups(nf, lgGroup, tg.fgGuided, 0xffffffffu, nullptr, nullptr), items = regions * numGroups,
                wgs = 16ull * (uint64_t)numCUs, fewest = 2ull * (uint64_t)numCUs;
            tg.slotLogCap = (uint32_t)std::min<uint64_t>(65534, 8 * ((items + fewest - 1) / fewest) + 16); /* 16 bits of an entry's tag */
            tg.launchEpoch = ++c->launchEpoch; c->lastSlotLogCap = (int)tg.slotLogCap;
            ex.grow(c->fgSlotLog[par], par, wgs * tg.slotLogCap * 8, false);
            tg.slotLog = (unsigned long long*)c->fgSlotLog[par].p;
            if (plan.costly_first) { /* this launch's order from the counts so far; the launch goes on counting */
                /* how much of the usual list counts as "late" (option costly_late_samples, in samples from the end of the list; default: all of it.
                 * Moving only the last 2^24 samples' worth -- 7 ms of a 4K glass scene, one long path -- was measured to gain half as much on a
                 * rank's 32-spp step and nothing on the whole frame) */
                const uint64_t lateSamples = (uint64_t)std::max<int64_t>(1, opt<OPT_costly_late_samples>(c)), perItem = 256ull * nf / std::max<uint64_t>(1, numGroups);
                const uint64_t lateItems = std::min<uint64_t>(items, (lateSamples + perItem - 1) / std::max<uint64_t>(1, perItem));
                ex.grow(c->regionOrder[par], par, (1 + items + regions) * 4, false);
                uint32_t* order = (uint32_t*)c->regionOrder[par].p;
                HIP_TRY(pt_launch_region_order(ptStream, (const uint32_t*)c->regionCost.p, &c->tiles, W, H, (uint32_t)regions, (uint32_t)numGroups,
                    (uint32_t)(items - lateItems), order, order + 1 + items));
                tg.regionCost = (uint32_t*)c->regionCost.p; tg.regionOrder = order;
            }
            if (r.prepass) { tg.primaryHits = (unsigned long long*)c->fgHits[par].p; tg.firstBounce = r.firstBounce ? 1u : 0u;
                tg.hitStamp = r.hitStampOf(tg.launchEpoch); tg.hitPrimBits = r.hitPrimBits; tg.hitGeomBits = c->hitGeomBits; }
        },
        /* (the adaptive launch tested per call: the same copy's kernel over the live list, and the fold over the list) */
        [&](uint32_t f0, uint32_t nf, uint32_t par, hipStream_t ptStream) { const TbDeviceScene dsPar = sceneOfSide(r.dsLaunch, par, r.overflowHalf);
            HIP_TRY(launch(ptStream, &dsPar, &pf, &tg, W, H, c->samplesRendered + f0, nf, &c->tiles, lds, 0, r.mode)); },
        [&](uint32_t f0, uint32_t nf) {
            if (r.adaptive) HIP_TRY(pt_launch_accumulate_live(c->stream, tg.samples, W, H, c->samplesRendered + f0, nf, liveList, c->lastOwnedPixels, tg.output,
                tg.jittered));
            else HIP_TRY(pt_launch_accumulate_samples(c->stream, tg.samples, W, H, c->samplesRendered + f0, nf, &c->tiles, tg.output, tg.jittered)); });
}

/* ---- the steps of a render call, in the order renderImpl takes them -------------------------------------------------------------------- */

/* validate, size the surfaces (main stream), forget the history on a change that matters to it */
static int beginCall(RenderCall& r, const tb_output_settings* settings)
{
    tb_context* c = r.c; const uint32_t W = r.W, H = r.H;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "tb_render: no scene loaded");
    if (W == 0 || H == 0) return fail(c, TB_E_INVALID, "tb_render: zero-sized target");
    if (W > 16384 || H > 16384) return fail(c, TB_E_INVALID,
        "tb_render: a target has at most 16384 pixels a side (D3D12_REQ_TEXTURE2D_U_OR_V_DIMENSION; pixel indices are 32-bit)");
    if (settings) r.s = *settings; else DefaultOutputSettings(r.s);
    if (W != c->width || H != c->height) {
        size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        ensure(c->output, bytes); ensure(c->jittered, bytes);
        HIP_TRY(hipMemsetAsync(c->output.p, 0, bytes, c->stream)); HIP_TRY(hipMemsetAsync(c->jittered.p, 0, bytes, c->stream));
        for (DevBuf& b : c->aov) b.release();
        c->width = W; c->height = H; resetHistory(c);
    }
    if (c->haveLastSettings && (historyRelevantChange(r.s, c->lastSettings) || r.timeSeed != c->lastTime)) resetHistory(c);
    c->lastSettings = r.s; c->haveLastSettings = true; c->lastTime = r.timeSeed;
    return TB_OK;
}

/* The adaptive launch (option "adaptive"): not in real time (the reference's !IsRealTime), and only for a call whose last frame
 * is past option adaptive_min_frames -- before that no pixel can skip, and every other call takes the plan and the kernels it always took.
 * Option adaptive_test = 1: one test per call, at its first frame -- the call is adaptive iff THAT frame is past the threshold (a call that starts
 * at or below it is a plain call even if it ends above), and the pixels live then get every frame of the call. */
static void decideAdaptive(RenderCall& r)
{
    tb_context* c = r.c;
    r.aov = opt<OPT_aov>(c) != 0; r.count = opt<OPT_count_rays>(c) != 0;
    r.adaptiveMin = std::min<int64_t>(opt<OPT_adaptive_min_frames>(c), 0xffffffffll);
    r.perCall = opt<OPT_adaptive_test>(c) == 1;
    r.adaptive = opt<OPT_adaptive>(c) != 0 && !r.count && !r.s.RenderModeRealTime &&
        (r.perCall ? (int64_t)c->samplesRendered : (int64_t)c->samplesRendered + (int64_t)r.n - 1) > r.adaptiveMin;
    /* A sample budget (tb_set_sample_budget) is the list pass's second source: every call under it, the one from frame 0
     * included, is a per-call adaptive call -- live at its first frame F0 iff F0 < budget, and, where options adaptive and adaptive_test are on and
     * F0 is past the threshold, iff the skip test does not hold either.  Real time ignores it, as it ignores option adaptive. */
    r.budgeted = c->budget.set && !r.s.RenderModeRealTime;
    if (r.budgeted) { r.skipTest = r.adaptive; r.adaptive = r.perCall = true; }
    c->budget.lastBudgeted = r.budgeted;
    c->lastAdaptive = r.adaptive; c->lastOwnedPixels = ownedFramePixels(r.W, r.H, c->tiles);
    /* 4 = the split-role kernel where it exists, the lock-step kernel (0) elsewhere */
    r.pipe = opt<OPT_pipeline>(c) == 4 ? 0 : opt<OPT_pipeline>(c);
}

/* TbDeviceTargets::camPre: path_begin's own expressions (pt_device.hpp), evaluated once */
void cameraConstants(const TbPerFrameConstants& pf, uint32_t W, uint32_t H, TbDeviceTargets& tg)
{
    const float resX = (float)W, resY = (float)H;
    const tb3 camPos = tb3_make(pf.CameraPosition.x, pf.CameraPosition.y, pf.CameraPosition.z);
    const tb3 lookAt = tb3_make(pf.CameraLookAt.x, pf.CameraLookAt.y, pf.CameraLookAt.z);
    const tb3 focal = camPos - pf.FocalDistance * tb3_normalize(lookAt - camPos);
    tg.camFocal[0] = focal.x; tg.camFocal[1] = focal.y; tg.camFocal[2] = focal.z;
    tg.camInvResX = 1.0f / resX; tg.camInvResY = 1.0f / resY; tg.camAspect = resX / resY; tg.camPre = 1u;
}

/* TbDeviceTargets: surfaces, AOVs, counters (sized and cleared on the main stream), the frame constants and the camera's */
static void fillTargets(RenderCall& r)
{
    tb_context* c = r.c; const uint32_t W = r.W, H = r.H; TbDeviceTargets& tg = r.tg;
    c->ds.alphaTest = opt<OPT_alpha_test>(c) ? 1u : 0u;
    ensure(c->stats, 16);
    r.clearStats = c->samplesRendered == 0; /* enqueued later, on the stream of the first path-tracing launch */
    memset(&tg, 0, sizeof tg);
    tg.output = (TbFloat4*)c->output.p; tg.jittered = (TbFloat4*)c->jittered.p; tg.stats = (uint32_t*)c->stats.p;
    if (!c->debugCounters.p) { ensure(c->debugCounters, 64); HIP_TRY(hipMemsetAsync(c->debugCounters.p, 0, 64, c->stream)); }
    tg.debugCounters = (uint32_t*)c->debugCounters.p;
    if (r.aov) {
        size_t px = (size_t)W * H;
        for (int i = 2; i <= 7; i++) { size_t bytes = px * (i == TB_AOV_DEPTH ? 4 : 16); if (c->aov[i].bytes != bytes) { ensure(c->aov[i], bytes);
            HIP_TRY(hipMemsetAsync(c->aov[i].p, 0, bytes, c->stream)); } }
        tg.aovNormals = (TbFloat4*)c->aov[2].p; tg.aovWorldPos0 = (TbFloat4*)c->aov[3].p; tg.aovWorldPos1 = (TbFloat4*)c->aov[4].p;
        tg.aovCustom = (TbFloat4*)c->aov[5].p; tg.aovDepth = (float*)c->aov[6].p; tg.aovEmissive = (TbFloat4*)c->aov[7].p;
        /* a real-time frame's positions go to the half tb_render_realtime reads as the current one (rt.active), whichever of the two the
         * kernels pick by the parity of the global frame number: the sample counter restarts with every camera move and tb_invalidate_history,
         * the chain's ping-pong does not -- left to the parity, a restart after an odd number of frames made the chain read the previous
         * frame's positions as the current ones and the current ones as the previous frame's */
        if (c->rt.chainFrame) tg.aovWorldPos0 = tg.aovWorldPos1 = (TbFloat4*)c->aov[TB_AOV_WORLD_POSITION0 + c->rt.active].p;
    }
    /* (debug_profile_groups: the counters' buffer handed to a frame-group launch -- only a library built with -DTB_EXP_PROFILE_GROUPS has a kernel
     * that writes them, scripts/c2_instruction_mix.py; the shipped frame-group kernels carry no counters and ignore the pointer) */
    if (r.count || opt<OPT_debug_profile_groups>(c)) { ensure(c->rayStats, 21 * 8); if (c->samplesRendered == 0) HIP_TRY(hipMemsetAsync(c->rayStats.p, 0, 21 * 8, c->stream));
        tg.rayStats = (unsigned long long*)c->rayStats.p; }
    MakeFrameConstants(c->scene, c->camera, r.s, c->samplesRendered, r.timeSeed, c->selX, c->selY, r.pf);
    if (const int64_t lights = opt<OPT_debug_light_count>(c)) r.pf.LightCount = (uint32_t)std::min<int64_t>(lights, 0xffffffffll);
    if (opt<OPT_camera_constants>(c) != 0) cameraConstants(r.pf, W, H, tg);
}

/* what PlanLaunch (launch_plan.h) is told about this context's scene, the call and the options */
static void fillPlanInput(const RenderCall& r, tb_plan_input& in)
{
    tb_context* c = r.c; const Variant* v = r.v;
    memset(&in, 0, sizeof in);
    in.variant_features = v->features(); in.variant_waves_hi = v->wavesHi(); in.variant_prepass_in_base = !v->hi && v->base->row->prepassInBase ? 1u : 0u;
    in.variant_stash_entries = v->stashHi();
    in.variant_has_wavefront = v->wf ? 1u : 0u; in.variant_has_pooled = v->pooled ? 1u : 0u; in.variant_has_split = v->split ? 1u : 0u;
    in.scene_in_lds = c->sceneInLds ? 1u : 0u; in.lds_blob_bytes = c->ds.ldsBlobBytes; in.stack_depth = c->ds.stackDepth;
    in.two_level = c->ds.numInstances ? 1u : 0u;
    in.has_lights = c->scene.lights.empty() ? 0u : 1u; in.has_compact_nodes = c->ds.nodesC ? 1u : 0u;
    in.interior_walk_triangle_share = c->interiorWalkTriangleShare;
    in.width = r.W; in.height = r.H; in.frames = r.n; in.max_bounces = r.s.MaxBounces; in.owned_regions = tb_persistent_grid(r.W, r.H, c->tiles);
    in.count_rays = r.count ? 1u : 0u; in.aov = r.aov ? 1u : 0u; in.realtime = r.s.RenderModeRealTime ? 1u : 0u; in.selected_pixel = c->selX != 0xffffffffu ? 1u : 0u;
    in.pipeline = opt<OPT_pipeline>(c); in.frame_group = opt<OPT_frame_group>(c); in.high_occupancy = opt<OPT_high_occupancy>(c);
    in.stack_lds_cap = opt<OPT_stack_lds_cap>(c); in.stack_overflow_max = opt<OPT_stack_overflow_max>(c); in.node_layout = opt<OPT_node_layout>(c);
    in.primary_prepass = opt<OPT_primary_prepass>(c); in.overlap_launches = opt<OPT_overlap_launches>(c); in.pooled_samples = opt<OPT_pooled_samples>(c);
    in.split_trav = opt<OPT_split_trav>(c); in.split_shade = opt<OPT_split_shade>(c); in.split_stack_cap = opt<OPT_split_stack_cap>(c);
    in.guided_groups = opt<OPT_guided_groups>(c); in.sync_call = r.sync ? 1u : 0u;
    in.costly_first = opt<OPT_banded_items>(c) == 0 ? (uint32_t)std::max<int64_t>(0, std::min<int64_t>(2, opt<OPT_costly_first>(c))) : 0u;
    in.adaptive = r.adaptive ? (r.perCall ? 2u : 1u) : 0u;
}

/* the feature set that covers what scene + settings need, and the plan for it.  WHAT to launch is decided by a pure function of scene statistics,
 * call size and options (launch_plan.h; tests/test_launch_plan.py walks its branches on the CPU); the steps after this one execute the plan. */
static int pickVariantAndPlan(RenderCall& r)
{
    tb_context* c = r.c;
    uint32_t need = c->sceneFeatures | settingsFeatureMask(c, r.s, r.aov);
    if (r.count || opt<OPT_force_full_variant>(c)) need = PT_FEAT_ALL;
    r.v = &kVariants[kNumVariants - 1];
    for (int i = 0; i < kNumVariants; i++) if ((need & ~kVariants[i].features()) == 0) { r.v = &kVariants[i]; break; }
    c->lastVariant = r.v->name;
    r.variantIndex = (int)(r.v - kVariants);
    r.twoLevel = c->ds.numInstances != 0; /* instanced scene (flatten_instances = 0): pipeline 0 only */
    if (r.twoLevel && r.pipe != 0 && !r.adaptive) return fail(c, TB_E_UNSUPPORTED,
        "tb_render: two-level (instanced) scenes are not supported by pipelines 1-3; use pipeline 0 or flatten_instances = 1");
    fillPlanInput(r, r.pin);
    PlanLaunch(r.pin, r.plan);
    if (r.plan.pipeline == 4 && !splitLaunchable(r)) { /* the launcher's own refusal: the lock-step kernel, by the plan's rules for it */
        r.pin.pipeline = 0; PlanLaunch(r.pin, r.plan); r.plan.rule_pipeline = TB_PLAN_RULE_SPLIT_NO_ROOM;
    }
    r.wavefront = r.plan.pipeline == 2; r.pooled = r.plan.pipeline == 3; r.split = r.plan.pipeline == 4; r.groups = r.plan.groups != 0;
    r.copy = r.plan.high_occupancy_copy ? r.v->hi : r.v->base;
    return TB_OK;
}

/* split stack: the deepest entries in global memory, one column per lane of the resident grid (at most 2 x 8 workgroups per CU) */
static void sizeSplitStack(RenderCall& r)
{
    tb_context* c = r.c;
    r.overflowHalf = 0;
    r.dsLaunch = c->ds; r.dsLaunch.stackOverflow = nullptr; r.dsLaunch.stackOverflowLanes = 0;
    if (!r.plan.stack_overflow_entries) return;
    const uint32_t lanes = 2u * 8u * (uint32_t)deviceCUs(c) * 256u;
    /* two halves: consecutive batches of a call overlap on the two side streams */
    ensure(c->stackOverflow, (size_t)r.plan.stack_overflow_entries * lanes * 4 * 2);
    r.overflowHalf = (size_t)r.plan.stack_overflow_entries * lanes;
    r.dsLaunch.stackDepth = r.plan.stack_lds_entries; r.dsLaunch.stackOverflow = (uint32_t*)c->stackOverflow.p; r.dsLaunch.stackOverflowLanes = lanes;
}

/* which copy of the feature set launches, and which node layout it walks (the plan is made again with what came of building layout C) */
static void pickCopy(RenderCall& r)
{
    tb_context* c = r.c; const Variant*& v = r.v; tb_launch_plan& plan = r.plan;
    if (plan.full_variant && v != &kVariants[kNumVariants - 1]) { v = &kVariants[kNumVariants - 1]; r.copy = v->base; c->lastVariant = v->name; }
    c->lastCopyWaves = r.copy == v->hi ? v->wavesHi() : 0u;
    r.mode = r.adaptive ? (r.groups ? PT_MODE_LIVE_GROUPS : PT_MODE_ADAPTIVE) : r.pipe == 1 ? PT_MODE_STREAM : PT_MODE_LOCKSTEP;
    /* the set's copy for scenes in LDS in place of the occupancy copy where its workgroups fit with the whole stack and it has a kernel for the call
     * as planned (pt_pick_form: the frame-group kernels of a one-level scene in LDS without counters; a pre-pass, even one left to the trial, keeps
     * the occupancy copy) */
    const PtShape planned{r.mode, r.groups, r.adaptive, r.count, c->sceneInLds, r.twoLevel, plan.compact_nodes != 0, plan.stack_overflow_entries != 0, true,
        plan.prepass != TB_PLAN_PREPASS_OFF, false, plan.guided_groups != 0};
    /* that copy fetches the shading tables without bounds checks (kernels/pt_variant_matte6.hip): only for a scene whose tables the host has checked
     * (lds_image.h SceneTablesInRange) and a call whose light indices stay inside the light table -- the index is (uint32_t)(rnd * LightCount) with
     * rnd < 1, and below 2^23 the fp32 product cannot round up to LightCount.  Any other keeps the occupancy copy with its guards */
    const bool tablesChecked = c->tablesInRange && r.pf.LightCount <= c->ds.numLights && r.pf.LightCount < (1u << 23);
    if (r.copy == v->hi && v->lds && pt_pick_form(*v->lds->row, planned).ok && LdsCopyFits(v->wavesLds(), c->ds.stackDepth, c->ds.ldsBlobBytes) &&
        tablesChecked) {
        r.copy = v->lds; c->lastCopyWaves = v->wavesLds(); }
    /* the adaptive launch, one pixel per lane, is the base copy's; the list-driven frame-group launch (rule TB_PLAN_RULE_ADAPTIVE_GROUPS) keeps the copy
     * chosen above */
    if (r.mode == PT_MODE_ADAPTIVE) r.copy = v->base;
    /* layout C on first demand */
    if (opt<OPT_node_layout>(c) == 1 && !r.twoLevel && !c->sceneInLds && !c->ds.nodesC && !c->compactTried) {
        ensureCompactNodes(c); r.dsLaunch.nodesC = c->ds.nodesC; r.dsLaunch.quant = c->ds.quant;
        r.pin.has_compact_nodes = c->ds.nodesC ? 1u : 0u; PlanLaunch(r.pin, plan);
    }
    if (!plan.compact_nodes) r.dsLaunch.nodesC = nullptr;
    c->lastNodeLayout = plan.compact_nodes ? 1 : 0;
}

static uint64_t kindOfCall(const RenderCall& r) /* same scene, frame, frames per call, depth and kernel: the key of a trial */
{
    return ((uint64_t)r.W << 48) ^ ((uint64_t)r.H << 32) ^ ((uint64_t)r.n << 12) ^ ((uint64_t)r.s.MaxBounces << 4) ^ ((uint64_t)r.c->sceneGeneration << 24) ^
        (uint64_t)r.launchKey();
}

/* the pre-pass where the plan leaves it to the trial (launch_trials.h): the sample is the first launch of the call before this one, if it has
 * finished -- tb_render_async enqueues, it never waits: no hipEventSynchronize here */
static void tryPrepass(RenderCall& r)
{
    tb_context* c = r.c;
    r.prepass = r.plan.prepass == TB_PLAN_PREPASS_ON;
    if (r.plan.prepass != TB_PLAN_PREPASS_TRIAL) return;
    const uint64_t key = kindOfCall(r);
    float ms = 0;
    if (!PrepassSampleWanted(c->prepassTrial, key, c->kernelEventStamp) || hipEventQuery(c->evKernel) != hipSuccess ||
        hipEventElapsedTime(&ms, c->evKernelStart, c->evKernel) != hipSuccess) ms = 0;
    r.prepass = PrepassTrialStep(c->prepassTrial, key, c->kernelEventStamp, ms);
}

/* what the pre-pass leaves behind for the lock-step kernel, per sample */
static void hitRecordFormat(RenderCall& r)
{
    tb_context* c = r.c;
    /* first-bounce pass (option first_bounce; pt_first, pt_persistent.inc): where the pre-pass runs, run a sample's whole first bounce there --
     * camera ray, shading, the first hit's feeler, scatter -- and hand the lock-step kernel the path's state (96-B records instead of 32-B hits) */
    r.firstBounce = r.prepass && opt<OPT_first_bounce>(c) != 0 && !r.plan.compact_nodes;
    /* compact hit records (pt_scene.h): 16 B where the scene's hit-group and primitive indices leave at least 4 bits of the fourth word for the stamp */
    /* (option compact_hits = 1 + k, a test hook: the primitive field k bits narrower than the scene needs -- hits that do not fit are stored as
     * nobody's and walked again by their lanes) */
    const int64_t compactOpt = opt<OPT_compact_hits>(c);
    r.hitPrimBits = compactOpt >= 2 ? (uint32_t)std::max<int64_t>(1, (int64_t)c->hitPrimBits - (compactOpt - 1)) : c->hitPrimBits;
    const uint32_t hitIndexBits = r.hitPrimBits + c->hitGeomBits;
    r.compactHits = r.prepass && !r.firstBounce && compactOpt != 0 && hitIndexBits >= 1 && hitIndexBits <= 28;
    /* Option compact_stamp_bits (a test hook) narrows the stamp (RenderCall::hitStampOf) to that many bits so that a small scene can be stressed at
     * the minimum width (tests/test_buffer_reuse_stress.py). */
    r.stampBits = (uint32_t)std::min<int64_t>(32 - (int64_t)hitIndexBits, std::max<int64_t>(2, opt<OPT_compact_stamp_bits>(c)));
    r.hitRecordBytes = r.firstBounce ? 96 : r.compactHits ? 16 : 32;
    c->lastCompactHits = r.compactHits ? 1 : 0;
    c->lastPrimaryPrepass = r.prepass ? 1 : 0; c->lastFirstBounce = r.firstBounce ? 1 : 0; c->lastPlan = r.plan;
}

/* Launches of the kernels without the EXT features (no selected pixel, no AOVs: nothing but the sample buffer is written) may overlap the drain
 * of the launch before them, which pays for the feature sets whose kernels fit their registers (matte / env: cornell-box +9 %, the 870 k scene
 * +4 ... +9 %, at every frame size measured) and is in doubt for the others: Teapot (surf) gains 9-17 % on calls below ~10 M samples and loses 6 %
 * above; the 4K glass scenes LOST 6-7 % with the round-3 kernels (whose leaf steps waited for scratch) and gain 4-5 % with the present ones, the
 * same scenes at 1080p gain 8-16 %, the reference's vw-van (vol) 18-39 % (scripts/overlap_ab.py, profiles/r4/overlap_ab*.json) -- no rule in
 * scene statistics fits that, and it moves with the kernels.  Like the pre-pass it is therefore TRIED where it is in doubt (option
 * overlap_launches = 1, the default; 2 = always, 0 = never; launch_trials.h), and every call leaves its record for the trial. */
static void tryOverlap(RenderCall& r)
{
    tb_context* c = r.c;
    r.overlap = r.plan.overlap_launches != 0;
    const uint64_t callKey = kindOfCall(r) ^ (r.prepass ? 1u : 0u);
    const bool trial = r.overlap && opt<OPT_overlap_launches>(c) == 1 && (r.v->features() & (PT_FEAT_SPECULAR | PT_FEAT_TEXTURES | PT_FEAT_SSS | PT_FEAT_MIX)) != 0;
    const DevEvent* ends = c->evCallEnd;
    if (trial) r.overlap = OverlapTrialStep(c->overlapTrial, c->callRec, c->callCount, callKey,
        [&](uint64_t i) { return ends[i & 7u] && ends[(i - 2) & 7u] && hipEventQuery(ends[i & 7u]) == hipSuccess; },
        [&](uint64_t i) { float ms = 0; return hipEventElapsedTime(&ms, ends[(i - 2) & 7u], ends[i & 7u]) == hipSuccess ? ms : 0.0f; });
    c->lastOverlap = r.overlap ? 1 : 0;
    hipEvent_t prevEnd = c->callCount ? ends[(c->callCount - 1) & 7u].e : nullptr;
    RecordCall(c->callRec, c->callCount, callKey, trial, r.overlap, prevEnd && hipEventQuery(prevEnd) == hipErrorNotReady);
}

/* The live list of an adaptive call's first frame (pt_kernels.hip live_list_*), on the main stream: scratch, the count in 16 bytes of its own, then
 * W x H entries at most -- the count directly before the list, where the list-driven frame-group kernels look for it (pt_scene.h
 * TB_LIVE_COUNT_WORDS; the one-pixel-per-lane kernel takes it by its own pointer).  Between ev0 and evKernelStart, so that option last_kernel_us
 * times the path-tracing launch alone. */
static void buildLiveList(RenderCall& r)
{
    tb_context* c = r.c; TbDeviceTargets& tg = r.tg;
    const uint32_t regions = tb_persistent_grid(r.W, r.H, c->tiles);
    const size_t scratch = (tb_live_list_scratch_bytes(regions) + 15u) / 16u * 16u;
    ensure(c->liveList, scratch + 4u * TB_LIVE_COUNT_WORDS + (size_t)r.W * r.H * 4u);
    uint8_t* base = (uint8_t*)c->liveList.p;
    c->liveCountOffset = scratch;
    /* (tested per call, the one-pixel-per-lane kernel's guard `frame > adaptiveMinFrames` before each later frame must never hold) */
    tg.liveCount = (const uint32_t*)(base + scratch); tg.liveList = tg.liveCount + TB_LIVE_COUNT_WORDS; tg.adaptiveMinFrames = r.perCall ? 0xffffffffu : (uint32_t)r.adaptiveMin;
    /* (under a budget without the skip test no frame is past the threshold) */
    const uint32_t minFrames = r.budgeted && !r.skipTest ? 0xffffffffu : (uint32_t)r.adaptiveMin;
    HIP_TRY(pt_launch_live_list(c->stream, tg.output, tg.jittered, r.budgeted ? (const uint32_t*)c->budget.values.p : nullptr, &c->tiles, r.W, r.H,
        c->samplesRendered, minFrames, r.pf.MinConvergence, tg.aovNormals, tg.aovCustom, r.s.OutputType == TB_OUTPUT_TYPE_LIVE_PIXELS ? 1 : 0, base, (uint32_t*)tg.liveList, (uint32_t*)tg.liveCount));
}

/* the path-tracing launches of the call: one of the other pipelines, one launch of the lock-step kernel on the main stream, or frame groups */
static void dispatch(RenderCall& r)
{
    tb_context* c = r.c;
    if (!r.groups) HIP_TRY(hipEventRecord(c->evKernelStart, c->stream));
    c->lastKernelFrames = 0;
    c->lastPipeline = r.split ? 4 : (r.wavefront ? 2 : (r.pooled ? 3 : (int)(r.pipe == 1 && !r.adaptive ? 1 : 0)));
    if (r.split) renderSplit(r);
    else if (r.wavefront) renderWavefront(c, r.variantIndex, r.W, r.H, c->samplesRendered, r.n, r.pf);
    else if (r.pooled) renderPooled(c, r.variantIndex, r.W, r.H, c->samplesRendered, r.n, r.pf);
    else if (r.groups) renderFrameGroups(r);
    else HIP_TRY(r.copy->launch(c->stream, &r.dsLaunch, &r.pf, &r.tg, r.W, r.H, c->samplesRendered, r.n, &c->tiles, c->sceneInLds ? 1 : 0, r.count ? 1 : 0,
        r.mode));
    /* one launch (or one pipeline) for the whole call */
    if (!c->lastKernelFrames) { HIP_TRY(hipEventRecord(c->evKernel, c->stream)); c->lastKernelFrames = r.n; }
}

/* the end of the call on the main stream: its events (evCallEnd: for the overlap trial of later calls), and the wait of a synchronous call */
static int closeCall(RenderCall& r)
{
    tb_context* c = r.c;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventRecord(c->evCallEnd[c->callCount & 7u].create(), c->stream)); c->callCount++;
    c->samplesRendered += r.n;
    if (r.sync) {
        HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipEventElapsedTime(&c->lastMs, c->ev0, c->ev1));
        HIP_TRY(hipEventElapsedTime(&c->lastKernelMs, c->evKernelStart, c->evKernel));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
    }
    return TB_OK;
}

int renderImpl(tb_context* c, uint32_t W, uint32_t H, uint32_t n, const tb_output_settings* settings, float timeSeed, bool sync)
{
    RenderCall r{}; r.c = c; r.W = W; r.H = H; r.n = n; r.timeSeed = timeSeed; r.sync = sync;
    if (c->budget.set && !(settings && settings->RenderModeRealTime)) { /* before anything is resized or forgotten */
        if (W != c->budget.width || H != c->budget.height) return fail(c, TB_E_INVALID, "tb_render: the sample budget is " + std::to_string(c->budget.width) +
            " x " + std::to_string(c->budget.height) + ", the render " + std::to_string(W) + " x " + std::to_string(H) +
            ": set a budget of the render's size or clear it (tb_set_sample_budget)");
        if (opt<OPT_count_rays>(c)) return fail(c, TB_E_INVALID,
            "tb_render: a sample budget and option \"count_rays\" exclude each other (the counting kernels have no list-driven copy)");
        if (opt<OPT_adaptive>(c) && opt<OPT_adaptive_test>(c) == 0) return fail(c, TB_E_INVALID,
            "tb_render: a sample budget with option \"adaptive\" needs \"adaptive_test\" = 1: the budget is applied once per call, the per-frame skip test "
            "would need a budget test inside the kernels");
    }
    if (const int rc = beginCall(r, settings)) return rc;
    if (n == 0) return TB_OK;
    decideAdaptive(r);
    fillTargets(r);
    if (const int rc = pickVariantAndPlan(r)) return rc;
    sizeSplitStack(r);
    pickCopy(r);
    tryPrepass(r);
    hitRecordFormat(r);
    tryOverlap(r);
    if (!r.overlap) c->sideOrdered = false;
    c->kernelEventStamp++; /* this render records evKernelStart / evKernel */
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    if (r.clearStats && !r.overlap) HIP_TRY(hipMemsetAsync(c->stats.p, 0, 16, c->stream)); /* (an overlapped call: on the stream of its first launch) */
    /* a plain call zeroes a pixel's sums through its frame-0 sample, the list-driven fold and the one-pixel-per-lane adaptive kernel write listed
     * pixels only: a budgeted call from frame 0 clears both surfaces first, so that a pixel that was never sampled reads (0, 0, 0, 0) */
    if (r.budgeted && c->samplesRendered == 0) {
        HIP_TRY(hipMemsetAsync(c->output.p, 0, c->output.bytes, c->stream)); HIP_TRY(hipMemsetAsync(c->jittered.p, 0, c->jittered.bytes, c->stream));
    }
    if (r.adaptive) buildLiveList(r);
    dispatch(r);
    return closeCall(r);
}

} // namespace tbctx
