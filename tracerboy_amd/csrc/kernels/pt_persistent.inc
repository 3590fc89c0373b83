/* pt_persistent.inc -- body of the persistent path-tracing kernel; included once per feature set
 * (pt_variant_*.hip define PT_FEATURES and PT_SUFFIX) so the variants compile in parallel. */
#ifndef PT_PERSISTENT_ATTR
#define PT_PERSISTENT_ATTR /* variants that are a register or two above a waves-per-SIMD step ask for it explicitly */
#endif
/* Primary-visibility pre-pass (TbDeviceTargets::primaryHits, pt_scene.h): a resident grid whose workgroups take (16x16 region, frame)
 * items in turn, one 8x8 pixel tile per wave; path_begin gives the camera ray exactly as the lock-step kernel will compute it again. */
template <uint32_t F, bool HYBRID, bool NODEC>
__global__ __launch_bounds__(BLOCK) void pt_primary(TbDeviceScene ds, TbPerFrameConstants pf, TbDeviceTargets tg, uint32_t W, uint32_t H,
                                                    uint32_t firstFrame, uint32_t numFrames, TbTileMap tiles)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SceneRefs sc;
    make_refs<false>(sc, ds, nullptr);
    uint32_t* stack = (uint32_t*)smem + threadIdx.x;
    uint32_t* const overflow = HYBRID ? ds.stackOverflow + (size_t)blockIdx.x * BLOCK + threadIdx.x : nullptr;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t regions = tb_persistent_grid(W, H, tiles), items = regions * numFrames;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t region = item % regions, f = item / regions;
        uint32_t bx, by;
        block_region(tiles, W, H, region, bx, by);
        const uint32_t x = bx * 16u + (wave & 1u) * 8u + (lane & 7u), y = by * 16u + (wave >> 1) * 8u + (lane >> 3);
        if (x >= W || y >= H) continue;
        Path p;
        path_begin<F>(p, ds, pf, firstFrame + f, W, H, x, y, &tg);
        const size_t i = (size_t)f * W * H + (size_t)y * W + x;
        if (p.state == ST_DONE) continue; /* MaxBounces == 0: nothing is traced (the host does not ask for the pre-pass then) */
        Hit h; uint32_t nb = 0, nt = 0;
        const bool isHit = traverse<false, false, HYBRID, NODEC>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, nullptr, overflow);
        /* (t or -1, u, v, primitive) and the hit-group index; a camera ray that leaves the scene is shaded like any other miss by the
         * lane that draws the sample.  (Finishing those samples here and letting the lanes skip them was measured: the pre-pass grew
         * by what the lock-step kernel saved.) */
        /* A record of its own per sample, stamped with the launch's epoch and closed by a check word: the per-XCD L2s are not coherent
         * with each other and a small frame's buffers stay L2-resident from launch to launch, so the lane that draws the sample may be
         * served a line as an earlier launch left it.  (A first version put the hit in the sample's own 16-B slot, unstamped: 3 % of
         * 200 x 120 x 9 renders shaded one 16x16 region x frame from stale slots.)  Plain 16-B stores and loads: system-scope ones
         * made the pre-pass 45 % slower, and a record that fails the check only costs its lane the walk (pt_persistent). */
        const unsigned long long w0 = (unsigned long long)(isHit ? __float_as_uint(h.t) : 0xbf800000u) | (unsigned long long)__float_as_uint(h.u) << 32,
                                 w1 = (unsigned long long)__float_as_uint(h.v) | (unsigned long long)h.prim << 32,
                                     w2 = (unsigned long long)h.geom | (unsigned long long)tg.launchEpoch << 32,
                                 w3 = w0 ^ w1 ^ w2;
        if (tg.hitStamp) { /* compact record (pt_scene.h) */
            const uint32_t pb = tg.hitPrimBits, gb = tg.hitGeomBits;
            const bool fits = !isHit || ((h.prim >> pb) == 0u && (h.geom >> gb) == 0u);
            const uint32_t packed = isHit ? (h.geom << pb | h.prim) : 0u;
            ((uint4*)tg.primaryHits)[i] = uint4{isHit ? __float_as_uint(h.t) : 0xbf800000u, __float_as_uint(h.u), __float_as_uint(h.v),
                                              fits ? (tg.hitStamp << (pb + gb) | packed) : 0u};
            continue;
        }
        uint4* rec = (uint4*)(tg.primaryHits + 4 * i);
        rec[0] = uint4{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
        rec[1] = uint4{(uint32_t)w2, (uint32_t)(w2 >> 32), (uint32_t)w3, (uint32_t)(w3 >> 32)};
    }
}

/* ---- first-bounce pass (TbDeviceTargets::firstBounce) ------------------------------------------------------------------------------
 * The state record of one sample: six 16-B pieces.
 *   [0] ro.xyz, seed   [1] rd.xyz, state | flags << 8 | bounce << 16   [2] T.xyz, launch epoch   [3] L.xyz, check = XOR of the other 15 words
 *   [4] absorption.xyz, maxTravel   [5] curIOR, newIOR, roughness, 0        (read and written only for a path that enters an interior walk)
 * Stamped and checked like the pre-pass's hit records: a record that is not this launch's, or not whole, sends its lane down the path from
 * the camera ray on (pt_persistent below) -- never a wrong state, only a slower sample. */
TBD void first_record_store(uint4* rec, const Path& p, uint32_t epoch)
{
    const uint32_t misc = p.state | (p.flags & 0xffu) << 8 | (uint32_t)p.bounce << 16;
    const uint32_t w[15] = {__float_as_uint(p.ro.x), __float_as_uint(p.ro.y), __float_as_uint(p.ro.z), __float_as_uint(p.seed),
                            __float_as_uint(p.rd.x), __float_as_uint(p.rd.y), __float_as_uint(p.rd.z), misc,
                            __float_as_uint(p.T.x), __float_as_uint(p.T.y), __float_as_uint(p.T.z), epoch,
                            __float_as_uint(p.L.x), __float_as_uint(p.L.y), __float_as_uint(p.L.z)};
    uint32_t check = 0;
    for (int k = 0; k < 15; k++) check ^= w[k];
    rec[0] = uint4{w[0], w[1], w[2], w[3]}; rec[1] = uint4{w[4], w[5], w[6], w[7]};
    rec[2] = uint4{w[8], w[9], w[10], w[11]}; rec[3] = uint4{w[12], w[13], w[14], check};
    if (p.state == ST_SSS) {
        rec[4] = uint4{__float_as_uint(p.absorption.x), __float_as_uint(p.absorption.y), __float_as_uint(p.absorption.z), __float_as_uint(p.maxTravel)};
        rec[5] = uint4{__float_as_uint(p.curIOR), __float_as_uint(p.newIOR), __float_as_uint(p.roughness), 0u};
    }
}

TBD bool first_record_load(const uint4* rec, Path& p, uint32_t epoch)
{
    const uint4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
    if (c.w != epoch || (a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z) != d.w) return false;
    p.ro = tb3_make(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)); p.seed = __uint_as_float(a.w);
    p.rd = tb3_make(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z));
    p.state = b.w & 0xffu; p.flags = (b.w >> 8) & 0xffu; p.bounce = (int)(b.w >> 16);
    p.T = tb3_make(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z));
    p.L = tb3_make(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    p.weight = 1.0f; p.sssStep = 0; p.lastBoxes = p.lastTris = 0; p.nMat = p.nLight = 0;
    if (p.state == ST_SSS) {
        const uint4 e = rec[4], f = rec[5];
        p.absorption = tb3_make(__uint_as_float(e.x), __uint_as_float(e.y), __uint_as_float(e.z)); p.maxTravel = __uint_as_float(e.w);
        p.curIOR = __uint_as_float(f.x); p.newIOR = __uint_as_float(f.y); p.roughness = __uint_as_float(f.z);
    }
    return true;
}

/* One sample's first bounce per lane, one 8x8 pixel tile of one frame per wave, a resident grid like pt_primary's.  The order of the step
 * functions is the lock-step kernel's for the feature set: without mix materials the bounce is finished before its feeler is walked. */
#ifndef PT_FIRST_ATTR
#define PT_FIRST_ATTR PT_PERSISTENT_ATTR
#endif
template <uint32_t F, bool HYBRID>
__global__ __launch_bounds__(BLOCK) PT_FIRST_ATTR void pt_first(TbDeviceScene ds, TbPerFrameConstants pf, TbDeviceTargets tg, uint32_t W, uint32_t H,
                                                                       uint32_t firstFrame, uint32_t numFrames, TbTileMap tiles)
{
    static_assert(!(F & FEAT_EXT), "the first-bounce pass writes no AOVs");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SceneRefs sc;
    make_refs<false>(sc, ds, nullptr);
    uint32_t* stack = (uint32_t*)smem + threadIdx.x;
    uint32_t* const overflow = HYBRID ? ds.stackOverflow + (size_t)blockIdx.x * BLOCK + threadIdx.x : nullptr;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t regions = tb_persistent_grid(W, H, tiles), items = regions * numFrames;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t region = item % regions, f = item / regions;
        uint32_t bx, by;
        block_region(tiles, W, H, region, bx, by);
        const uint32_t x = bx * 16u + (wave & 1u) * 8u + (lane & 7u), y = by * 16u + (wave >> 1) * 8u + (lane >> 3);
        if (x >= W || y >= H) continue;
        Path p;
        path_begin<F>(p, ds, pf, firstFrame + f, W, H, x, y, &tg);
        uint4* rec = (uint4*)tg.primaryHits + 6 * ((size_t)f * W * H + (size_t)y * W + x);
        if (p.state == ST_EXTEND) {
            Hit h; uint32_t nb = 0, nt = 0;
            const bool isHit = traverse<false, false, HYBRID, false, false, (F & FEAT_SSS) != 0>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, nullptr, overflow);
            path_on_closest<F>(p, sc, ds, pf, isHit, h);
            if constexpr (!(F & FEAT_MIX)) {
                const bool feeler = p.state == ST_SHADOW;
                const tb3 sro = p.ro, srd = p.rd, contrib = p.contrib;
                if (feeler) p.state = ST_SCATTER;
                if (p.state == ST_SCATTER) path_scatter<F>(p, pf);
                if (feeler) {
                    Hit hs;
                    const bool blocked = traverse<false, false, HYBRID, false, false, (F & FEAT_SSS) != 0>(sc, ds, sro, srd, hs, stack, BLOCK, nb, nt, nullptr, overflow);
                    path_apply_shadow<F>(p, sc, ds, pf, blocked, hs, srd, contrib);
                }
            } else {
                if (p.state == ST_SHADOW) {
                    Hit hs;
                    const bool blocked = traverse<false, false, HYBRID, false, false, (F & FEAT_SSS) != 0>(sc, ds, p.ro, p.rd, hs, stack, BLOCK, nb, nt, nullptr, overflow);
                    path_on_shadow<F>(p, sc, ds, pf, blocked, hs);
                }
                if (p.state == ST_SCATTER) path_scatter<F>(p, pf);
            }
        }
        first_record_store(rec, p, tg.launchEpoch);
    }
}

/* GUIDED: the launch's frame groups shrink over its end (TbDeviceTargets::fgGuided, pt_scene.h tb_fg_groups) -- a copy of its own, because the three
 * instructions per drawn sample that read a slot's size cost the VALU-bound cornell-box kernel 0.6 % of its asynchronous step (1.0 % behind a uniform
 * branch: same box, 7 140 / 7 105 against 7 185 Msamples/s) and only launches of calls that wait use it */
/* ADAPTIVE: the adaptive launch (TbDeviceTargets::liveList, pt_scene.h) -- the one-pixel-per-lane form over the packed live pixels, each lane testing
 * its pixel again before every later frame (DESIGN.md section 10) */
/* GROUPS + ADAPTIVE: the adaptive launch tested once per call -- the frame-group form over the live list.  A work item is one 256-entry block of
 * the list x G frames: the "regions" of the binding below are the list's blocks, a slot's entry carries the block's number where it carries a
 * region's coordinates, and a sample number finds its pixel on the list (resolve()).  Everything else -- claims, slots, the ordered sample buffer --
 * is the frame-group form's. */
template <uint32_t F, bool SCENE_LDS, bool COUNT, bool GROUPS, bool HYBRID = false, bool NODEC = false, bool TWOLEVEL = false, bool PRIMARY = false,
          bool FIRST = false, bool GUIDED = false, bool ADAPTIVE = false>
__global__ __launch_bounds__(BLOCK) PT_PERSISTENT_ATTR void pt_persistent(TbDeviceScene ds, TbPerFrameConstants pf, TbDeviceTargets tg, uint32_t W, uint32_t H,
                                                        uint32_t firstFrame, uint32_t numFrames, TbTileMap tiles)
{
    /* the adaptive launch: the grid is the owned region count, an upper bound; a workgroup whose first entry is past the live count has no pixel */
    uint32_t liveCount = 0;
    if constexpr (ADAPTIVE && !GROUPS) { liveCount = *tg.liveCount; if (blockIdx.x * BLOCK >= liveCount) return; }
    if constexpr (ADAPTIVE && GROUPS) { if (tg.liveList[-TB_LIVE_COUNT_WORDS] == 0u) return; } /* nothing is live: the whole grid leaves at once */
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    /* what the walks of this kernel carry besides the hit: per-ray box / triangle counters for the counting launch and for the full feature
     * set's heatmap (RayGenCommon.h:537-543), the IsValidHit filter in the full feature set only; the wave-occupancy profile rides on COUNT */
    constexpr bool RAY_COUNTERS = COUNT || (F & FEAT_EXT) != 0, ALPHA = (F & FEAT_EXT) != 0;
    /* frame-group mode: the workgroup's sample counter and its ring of bound slots (entry layout below) */
    __shared__ uint32_t drawn;
    __shared__ unsigned long long slotTable[8];
    /* regions, log2(frames per group), frame groups per region, "a claim has found nothing", tag base: read at every draw, kept out of the registers */
    __shared__ uint32_t groupConst[6];
    __shared__ uint32_t bindState[2];  /* binders under way, slots bound so far */
    /* A slot's entry: tag << 40 | first frame of the group (relative) << 24 | log2(frames of the group) << 20 | region y << 10 | region x.
     * The lane that binds a slot pays for the divisions that turn a work item into (region, frame group); the 256 x G samples
     * of the slot then need shifts and masks only (the frame-group size is a power of two, context.cpp). */
    /* the tag, the top 24 bits of an entry: the slot's number + 1 (16 bits; the host keeps the logs below 65 535 slots a workgroup) under
     * the low byte of the launch's epoch (groupConst[4]) -- a log row as an earlier launch left it (a stale cache line: the per-XCD L2s
     * are not coherent with each other, and a row is rewritten every launch) can then not be taken for this launch's */
    auto slot_tag = [&](uint32_t slot) -> uint32_t { return ((volatile uint32_t*)groupConst)[4] | ((slot + 1u) & 0xffffu); };
    /* Binding (fg_bind_next, pt_common.hpp).  A binder (the lane that draws a slot's trigger sample, draw() below) claims a work item and
     * gives it the NEXT FREE slot number -- in that order.  Slots are therefore bound 0, 1, 2 ... without a gap, and "nothing left" is
     * not an entry but a state of the workgroup: a claim has failed (final: no binder claims after that), no binder is under way, and
     * the slot asked for was never bound (fg_resolve_slow).  The first form bound slot s + 1 from slot s's trigger; two binders under
     * way at once -- a workgroup at the frame's edge draws its second slot's trigger while thread 0 is still claiming -- could then
     * leave slot 1 with "nothing left" and slot 2 with the last item of the launch, which no lane ever reached: 256 x G samples of the
     * final frame group unrendered, about once in 1 000 renders of a 200 x 120 frame (scripts/lost_item_stress.py; the slot log named
     * it).  Published in the LDS ring and, for good, in the workgroup's row of a log in global memory: the ring entry of slot s is
     * reused for slot s + 8, and a lane parked on a slot not yet bound (ST_WAIT) asks again only once per trip of its wave round the
     * path loop. */
#ifdef TB_WG_TIMELINE
    /* experiment builds only (scripts/wg_timeline.py): the last 8 entries of the workgroup's log row carry its timeline in 100-MHz ticks --
     * [cap-1] start, [cap-2] the first lane that found nothing left, [cap-3 .. cap-6] the exit of each wave, [cap-7] samples drawn */
    __shared__ unsigned long long tlDry;
    __shared__ uint32_t tlStat[4]; /* ticks inside bind_next, lane-trips parked in ST_WAIT, out-of-line resolves, binds */
    const uint32_t logCapUse = tg.slotLogCap - 12u;
    if (GROUPS && threadIdx.x == 0) { tlDry = 0; for (int i = 0; i < 4; i++) tlStat[i] = 0; tg.slotLog[(size_t)blockIdx.x * tg.slotLogCap + tg.slotLogCap - 1u] = wall_clock64(); }
    auto bind_next = [&]() { const unsigned long long t0 = wall_clock64();
        fg_bind_next(groupConst, bindState, slotTable, tg.workCounter, tg.slotLog + (size_t)blockIdx.x * tg.slotLogCap, logCapUse, tg.bandedItems, tiles, W, H, (F & FEAT_SSS) ? tg.regionOrder : nullptr);
        atomicAdd(&tlStat[0], (uint32_t)(wall_clock64() - t0)); atomicAdd(&tlStat[3], 1u); };
#else
    const uint32_t logCapUse = tg.slotLogCap;
    auto bind_next = [&]() {
        /* (the list form: block b of the list goes through block_region as region (b & 1023, b >> 10) of a frame 1024 regions wide, so the entry's 20
         * region bits are b itself; no order table -- its pointer is the list's) */
        if constexpr (ADAPTIVE) fg_bind_next(groupConst, bindState, slotTable, tg.workCounter, tg.slotLog + (size_t)blockIdx.x * tg.slotLogCap, logCapUse,
            tg.bandedItems, TbTileMap{0u, 1u, 16u, 16u}, 16384u, 16384u, nullptr);
        else fg_bind_next(groupConst, bindState, slotTable, tg.workCounter, tg.slotLog + (size_t)blockIdx.x * tg.slotLogCap, logCapUse,
        tg.bandedItems, tiles, W, H, (F & FEAT_SSS) ? tg.regionOrder : nullptr); };
#endif
    if (threadIdx.x == 0) {
        drawn = BLOCK; for (int i = 0; i < 8; i++) slotTable[i] = 0;
        if (GROUPS) {
            /* (the list form: the 256-entry blocks of the live list in place of the regions) */
            const uint32_t regions = ADAPTIVE ? (tg.liveList[-TB_LIVE_COUNT_WORDS] + 255u) >> 8 : tb_persistent_grid(W, H, tiles),
                lg = 31u - (uint32_t)__clz((int)tg.frameGroup);
            groupConst[3] = 0; groupConst[4] = (tg.launchEpoch & 0xffu) << 16; bindState[0] = 0; bindState[1] = 0;
            /* frame groups per region (< 4096: group << 20 | region) */
            groupConst[0] = regions; groupConst[1] = lg; groupConst[2] = tb_fg_groups(numFrames, lg, GUIDED ? 1u : 0u, 0xffffffffu, nullptr, nullptr);
            groupConst[5] = numFrames | (GUIDED ? 0x80000000u : 0u);
            bind_next();
        }
    }
    /* the copies that walk with the LDS steps (traverse(), pt_device.hpp): inner child refs become LDS addresses on their way in, and every lane's
     * stack column starts with the sentinel those steps pop last */
#ifdef PT_LDS_WALK
    constexpr bool LDS_STEPS = SCENE_LDS && !HYBRID && !NODEC && !TWOLEVEL && !(F & FEAT_EXT);
#else
    constexpr bool LDS_STEPS = false;
#endif
    uint32_t* stackBase = (uint32_t*)smem;
    const uint8_t* blob = smem + (size_t)ds.stackDepth * BLOCK * 4;
    if (SCENE_LDS) {
        const uint4* src = (const uint4*)ds.ldsBlob; uint4* dst = (uint4*)(smem + (size_t)ds.stackDepth * BLOCK * 4);
        for (uint32_t i = threadIdx.x; i < ds.ldsBlobBytes / 16; i += BLOCK) dst[i] = LDS_STEPS ? lds_steps_copy_in(src[i], i, ds, blob) : src[i];
        if (LDS_STEPS) stackBase[threadIdx.x] = 0xffffffffu;
    }
    if (SCENE_LDS || GROUPS) __syncthreads();
    SceneRefs sc;
    make_refs<SCENE_LDS>(sc, ds, blob);

    /* pixel mapping: lane -> 8x8 tile, wave -> one of 2x2 tiles of a 16x16 block region */
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t bx, by;
    block_region(tiles, W, H, blockIdx.x, bx, by);
    /* the lane's pixel, x | y << 16: one pixel for the whole launch, or in frame-group mode the pixel of the sample in flight */
    uint32_t xy = (bx * 16u + (wave & 1u) * 8u + (lane & 7u)) | (by * 16u + (wave >> 1) * 8u + (lane >> 3)) << 16;
    /* (the adaptive launch: entry 256 b + t of the live list; a lane past the count has no pixel -- 0xffff is beyond any frame) */
    if constexpr (ADAPTIVE && !GROUPS) { const uint32_t i = blockIdx.x * BLOCK + threadIdx.x; xy = i < liveCount ? tg.liveList[i] : 0xffffffffu; }
#define PX (xy & 0xffffu)
#define PY (xy >> 16)
#define PIX ((size_t)PY * W + PX)
    const bool mine = !GROUPS && PX < W && PY < H && numFrames > 0;
    bool alive = mine;
    /* OutputGlobalStats, SoftwareRayTraceCS.hlsl:15-24 */
    if (blockIdx.x == 0 && threadIdx.x == 0 && tg.stats) tg.stats[0] = ((W - 1) / 8 + 1) * ((H - 1) / 8 + 1);
    /* The lane's stack column in LDS and its overflow column in global memory (split stack, pt_scene.h) are made from the lane number at
     * every walk (walk_addr), and the number passes through an empty asm so that the sums cannot be hoisted to here: computed once they live
     * for the whole kernel, and the kernels held to an occupancy kept them in scratch -- reloaded at every push and pop (walk_owns, pt_device.hpp) */
    struct WalkAddr { uint32_t* stack; uint32_t* overflow; };
    auto walk_addr = [&]() __attribute__((always_inline)) -> WalkAddr {
        uint32_t t = threadIdx.x; asm volatile("" : "+v"(t));
        return WalkAddr{stackBase + t, HYBRID ? ds.stackOverflow + (size_t)blockIdx.x * BLOCK + t : nullptr};
    };
#ifdef PT_LDS_STASH
    /* PT_LDS_STASH entries of LDS per lane behind the stacks, [entry][lane] like them (a feature set's own choice, pt_variant_env5.hip).  What a path
     * carries ACROSS a walk and the walk never reads -- throughput, radiance, seed; across the feeler also the next ray -- is parked there by hand
     * before the walk and fetched after it: ds_write / ds_read instead of the scratch stores and loads the register allocator issues for them
     * through the vector-memory pipe, which is what bounds these kernels.  The launcher adds the bytes, the plan takes them off the stack's share. */
    constexpr bool STASH = !SCENE_LDS && !TWOLEVEL && !(F & FEAT_EXT) && GROUPS;
    uint32_t* const stashBase = (uint32_t*)smem + (size_t)ds.stackDepth * BLOCK;
    auto stash_at = [&]() __attribute__((always_inline)) -> uint32_t* { uint32_t t = threadIdx.x; asm volatile("" : "+v"(t)); return stashBase + t; };
#define STASH_PUT(st, k, v) (st)[(k) * BLOCK] = __float_as_uint(v)
#define STASH_GET(st, k) __uint_as_float((st)[(k) * BLOCK])
#endif
    uint32_t frame = firstFrame;
    const uint32_t endFrame = firstFrame + numFrames;

    /* Frame-group mode (TbDeviceTargets::samples).  A work item is one 16x16 region x frameGroup consecutive frames; a sample
     * depends on (x, y, frame) alone and lands in its own slot of the sample buffer, so any lane may render any of them.  The
     * launch is one resident grid: a workgroup numbers the samples it starts (LDS counter `drawn`), sample number K belongs to
     * the workgroup's slot K / (256 * frameGroup), and slots are bound to work items from the global lists about one slot ahead
     * of their use (bind_next above: one more slot whenever a slot's trigger sample is drawn).  Lanes therefore run from one item
     * into the next without waiting for the rest of the workgroup, and workgroups stay full until the lists are empty.  A lane
     * that finds its slot not bound yet (the start of a launch, when lanes whose first sample lies outside the frame draw again at
     * once) parks in ST_WAIT and asks again on the next trip round the loop -- no spinning inside divergent code. */
    /* (the trigger -- the first sample of a slot's last frame binds one more slot -- is pulled in resolve(), which knows how many frames the slot has) */
    auto resolve = [&](uint32_t K) -> int { /* 0: not published yet, 1: (xy, frame) set, 2: nothing left, 3: not a sample (outside the frame), draw again */
        const uint32_t lg = ((volatile uint32_t*)groupConst)[1];
        const uint32_t r = K >> 8, s = r >> lg, f = r & ((1u << lg) - 1u);
        unsigned long long e = ((volatile unsigned long long*)slotTable)[s & 7u];
        const uint32_t tag = slot_tag(s);
        if ((uint32_t)(e >> 40) != tag) { /* not bound yet, or the ring has gone round since: out of line */
#ifdef TB_WG_TIMELINE
            atomicAdd(&tlStat[2], 1u);
#endif
            e = fg_resolve_slow(s, tag, groupConst, bindState, tg.slotLog + (size_t)blockIdx.x * tg.slotLogCap);
            if (e < 2) return e ? 2 : 0;
        }
        /* A slot spans 256 << lg sample numbers whatever its group's size; a group of fewer frames (the launch's groups may shrink towards its end,
         * tb_fg_groups) uses the first of them, and a lane that draws a number beyond moves the counter on to the next slot's. */
        uint32_t lgS = lg;
        if constexpr (GUIDED) {
            lgS = ((uint32_t)e >> 20) & 15u;
            if (f >= (1u << lgS)) { atomicMax(&drawn, (s + 1u) << (8u + lg)); return 3; }
        }
        if ((K & 255u) == 0u && f == (1u << lgS) - 1u) bind_next(); /* the first sample of the slot's last frame: one more slot is bound */
        const uint32_t fr = firstFrame + ((uint32_t)(e >> 24) & 0x7fffu) + f;
        if constexpr (ADAPTIVE) {
            /* the list form: entry 256 x block + (K & 255) -- the list is in region / wave / lane order and K & 255 is the dense kernel's (wave, lane)
             * numbering, so a wholly live region's block is the slot above; an entry past the count is no sample, like a pixel outside the frame */
            const uint32_t i = ((uint32_t)e & 0xfffffu) << 8 | (K & 255u);
            if (fr >= endFrame || i >= tg.liveList[-TB_LIVE_COUNT_WORDS]) return 3;
            frame = fr; xy = tg.liveList[i];
            return 1;
        }
        const uint32_t x = ((uint32_t)e & 0x3ffu) * 16u + ((K >> 6) & 1u) * 8u + (K & 7u),
            y = (((uint32_t)e >> 10) & 0x3ffu) * 16u + ((K >> 7) & 1u) * 8u + ((K >> 3) & 7u);
        if (fr >= endFrame || x >= W || y >= H) return 3;
        frame = fr; xy = x | y << 16;
        return 1;
    };
    /* next sample for this lane: 1 = ready to begin, 0 = parked (frame holds the sample number), 2 = the lane is finished */
    auto next_sample = [&](uint32_t K, bool haveK) -> int {
        for (;;) {
            if (!haveK) K = atomicAdd(&drawn, 1u);
            const int r = resolve(K);
#ifdef TB_WG_TIMELINE
            if (r == 2 && ((volatile unsigned long long*)&tlDry)[0] == 0) ((volatile unsigned long long*)&tlDry)[0] = wall_clock64();
#endif
            if (r == 0) { frame = K; return 0; }
            if (r != 3) return r;
            haveK = false;
        }
    };
    int pending = 1;
    if (GROUPS) {
        pending = next_sample(threadIdx.x, true);
        alive = pending != 2;
    }
    TbFloat4 acc = {0, 0, 0, 0}, jacc = {0, 0, 0, 0};
    if (!GROUPS && alive && firstFrame > 0 && !((F & FEAT_EXT) && pf.IsRealTime)) { acc = tg.output[PIX]; if (tg.jittered) jacc = tg.jittered[PIX]; }
    unsigned long long cBoxes = 0, cTris = 0, cHits = 0, cMats = 0, cLights = 0, cSamples = 0, cRays = 0;
    WaveProf profStore; WaveProf* prof = nullptr;
    if (COUNT) { for (int i = 0; i < PROF_SLOTS; i++) profStore.v[i] = 0; prof = &profStore; }

    Path p;
    /* a path just begun: with the pre-pass its first hit is waiting (ST_PRIMARY), otherwise its camera ray is the pending ray */
    /* (with the first-bounce pass the path's state after its first bounce is waiting in the sample's record: nothing to compute here) */
    /* (the host's camera constants, TbDeviceTargets::camPre, where the scene is fetched from memory: +1.1 ... +1.6 % on the 870 k, van- and bistro-class
     * scenes; the LDS-resident cornell-box kernel measured -0.4 % with them and computes its own) */
    auto begin = [&]() __attribute__((always_inline)) {
        if (FIRST) { p.state = ST_PRIMARY; p.flags = 0; p.bounce = 0; return; }
        path_begin<F>(p, ds, pf, frame, W, H, PX, PY, SCENE_LDS ? nullptr : &tg);
#if TB_EXP_DOUBLE == 1
        { Path q; uint32_t f2 = frame, x2 = PX, y2 = PY; asm volatile("" : "+v"(f2), "+v"(x2), "+v"(y2));
          path_begin<F>(q, ds, pf, f2, W, H, x2, y2, SCENE_LDS ? nullptr : &tg);
          if (exp_never(q.rd.x + q.rd.y + q.rd.z, q.seed, q.ro.x + q.ro.y + q.ro.z, q.weight)) p.flags |= 0x40000000u; }
#endif
        if (PRIMARY && p.state == ST_EXTEND) p.state = ST_PRIMARY; };
    if (alive && pending == 1) begin();
    if (alive && pending == 0) p.state = ST_WAIT;
    while (alive) {
        if (COUNT) prof_hit(prof, PROF_ITER);
#ifdef TB_WG_TIMELINE
        if (GROUPS && p.state == ST_WAIT) atomicAdd(&tlStat[1], 1u);
#endif
        if (GROUPS && p.state == ST_WAIT) { /* frame-group mode: ask again for the work item of the sample number in `frame` */
            const int r = next_sample(frame, true);
            if (r == 2) { alive = false; break; }
            if (r == 0) continue;
            begin();
            if (p.state == ST_DONE) continue;
        }
        if (p.state == ST_DONE) {
            if (COUNT) prof_hit(prof, PROF_REGEN);
            /* kernel.glsl:1910-1920 + RayGenCommon.h:704-727 */
            tb3 color = p.L;
            if ((F & FEAT_EXT) && pf.FireflyClampValue >= EPSILON) color = tb3_min(color, tb3_splat(pf.FireflyClampValue));
            float s0 = color.x * p.weight, s1 = color.y * p.weight, s2 = color.z * p.weight, s3 = p.weight;
            bool ok = !(tb_isnan(s0) || tb_isnan(s1) || tb_isnan(s2) || tb_isnan(s3));
            float o0 = 0, o1 = 0, o2 = 0, o3 = 0;
            if (ok) { o0 += s0; o1 += s1; o2 += s2; o3 += s3; }
            float coin = rnd(p.seed, pf.Time);
            const size_t pix = PIX;
            TbFloat4 before{0, 0, 0, 0}; /* the adaptive launch: the sums before this sample (its LIVE_PIXELS AOV) */
            if constexpr (ADAPTIVE && !GROUPS && (F & FEAT_EXT) != 0) before = acc;
            if (GROUPS) tg.samples[(size_t)(frame - firstFrame) * W * H + pix] = TbFloat4{o0, o1, o2, coin < 0.5f ? -o3 : o3};
            else {
                if (((F & FEAT_EXT) && pf.IsRealTime) || frame == 0) acc = TbFloat4{0, 0, 0, 0};
                acc = TbFloat4{o0 + acc.x, o1 + acc.y, o2 + acc.z, o3 + acc.w};
                if (!((F & FEAT_EXT) && pf.IsRealTime) && (frame == 0 || coin < 0.5f)) {
                    if (frame == 0) jacc = TbFloat4{0, 0, 0, 0};
                    jacc = TbFloat4{o0 + jacc.x, o1 + jacc.y, o2 + jacc.z, o3 + jacc.w};
                }
            }
            if (F & FEAT_EXT) {
            if (tg.aovNormals) tg.aovNormals[pix] = TbFloat4{p.aovNormal.x, p.aovNormal.y, p.aovNormal.z, 1.0f};
            if (tg.aovWorldPos0 && (frame % 2) == 0) tg.aovWorldPos0[pix] = TbFloat4{p.aovWorldPos.x, p.aovWorldPos.y, p.aovWorldPos.z, p.aovNeighbor};
            if (tg.aovWorldPos1 && (frame % 2) == 1) tg.aovWorldPos1[pix] = TbFloat4{p.aovWorldPos.x, p.aovWorldPos.y, p.aovWorldPos.z, p.aovNeighbor};
            /* (the adaptive launch in LIVE_PIXELS mode: a sample that stored no primary albedo -- a camera ray that missed -- leaves the reference's
             * OutputLivePixels(false) tint of the sums before it, RayGenCommon.h:545-551) */
            if (ADAPTIVE && !GROUPS && tg.aovCustom && pf.OutputMode == TB_OUTPUT_TYPE_LIVE_PIXELS && !(p.flags & F_AOV_ALBEDO))
                tg.aovCustom[pix] = TbFloat4{before.x / before.w, 0.2f * (before.y / before.w), 0.2f * (before.z / before.w), before.w / before.w};
            else if (tg.aovCustom) tg.aovCustom[pix] = (p.flags & F_HEATMAP) ? TbFloat4{(float)p.lastTris, (float)p.lastBoxes, 0, 0} : TbFloat4{p.aovAlbedo.x,
                p.aovAlbedo.y, p.aovAlbedo.z, 1.0f};
            if (tg.aovDepth && (p.flags & F_AOV_DEPTH)) tg.aovDepth[pix] = p.aovDepth;
            if (tg.aovEmissive && (p.flags & F_AOV_EMISSIVE)) tg.aovEmissive[pix] = TbFloat4{p.aovEmissive.x, p.aovEmissive.y, p.aovEmissive.z, 1.0f};
            }
            if (COUNT) { cSamples++; cMats += p.nMat; cLights += p.nLight; }
            if (GROUPS) { const int r = next_sample(0, false); if (r == 2) { alive = false; break; } if (r == 0) { p.state = ST_WAIT; continue; } }
            else { frame++; if (frame >= endFrame) { alive = false; break; } }
            if constexpr (ADAPTIVE && !GROUPS) { /* (the list-driven frame-group form tests once per call: the list pass has) */
                /* the skip test before every later frame, on the sums in the lane's registers (behind the cheap frame guard: seven divisions and a
                 * square root).  A pixel that skips keeps skipping -- its sums and the threshold no longer change -- so the lane retires: its sums
                 * go back unchanged below, and an AOV call leaves the reference's ClearAOVs + OutputLivePixels(true) of a skipped pixel */
                if (frame > tg.adaptiveMinFrames && tb_adaptive_skip(acc, jacc, pf.MinConvergence)) {
                    if constexpr ((F & FEAT_EXT) != 0) {
                        if (tg.aovNormals) tg.aovNormals[pix] = TbFloat4{0, 0, 0, 1.0f};
                        if (tg.aovCustom) tg.aovCustom[pix] = pf.OutputMode == TB_OUTPUT_TYPE_LIVE_PIXELS ? TbFloat4{acc.x / acc.w, acc.y / acc.w, acc.z / acc.w,
                            acc.w / acc.w} : TbFloat4{0, 0, 0, 1.0f};
                    }
                    alive = false; break;
                }
            }
            begin();
            if (p.state == ST_DONE) continue; /* MaxBounces == 0 */
        }
        /* With the pre-pass the loop is turned by one slot: a path that has just begun takes its first hit from the sample's slot
         * and is shaded at once, then come the feelers (of these first hits and of the hits the previous trip ended with), then
         * the bounce rays -- every lane that walks in slot 1 walks a ray the pre-pass could not have walked for it. */
        if (PRIMARY && FIRST && p.state == ST_PRIMARY) {
            /* first-bounce pass: the state pt_first left (ST_EXTEND: the second bounce's ray is pending; ST_SSS: the first step of an interior
             * walk; ST_DONE: the path ended on its first hit).  A record that is not this launch's or not whole: the path from its camera ray on. */
            const uint4* rec = (const uint4*)tg.primaryHits + 6 * ((size_t)(frame - firstFrame) * W * H + PIX);
            if (!first_record_load(rec, p, tg.launchEpoch)) {
                path_begin<F>(p, ds, pf, frame, W, H, PX, PY, SCENE_LDS ? nullptr : &tg);
                if (tg.debugCounters) atomicAdd(&tg.debugCounters[0], 1u);
            }
        }
        if (PRIMARY && !FIRST && p.state == ST_PRIMARY) {
            const size_t i = (size_t)(frame - firstFrame) * W * H + PIX;
            Hit h; uint32_t tbits; bool mine;
            if (tg.hitStamp) { /* compact records (pt_scene.h): one 16-B piece, stamped */
                const uint4 r = ((const uint4*)tg.primaryHits)[i];
                const uint32_t pb = tg.hitPrimBits, gb = tg.hitGeomBits;
                tbits = r.x; h.u = __uint_as_float(r.y); h.v = __uint_as_float(r.z);
                h.prim = r.w & ((1u << pb) - 1u); h.geom = (r.w >> pb) & ((1u << gb) - 1u);
                mine = (r.w >> (pb + gb)) == tg.hitStamp;
            } else {
                const uint4* rec = (const uint4*)(tg.primaryHits + 4 * i);
                const uint4 ra = rec[0], rb = rec[1];
                tbits = ra.x; h.u = __uint_as_float(ra.y); h.v = __uint_as_float(ra.z); h.prim = ra.w; h.geom = rb.x;
                mine = rb.y == tg.launchEpoch && (ra.x ^ ra.z ^ rb.x) == rb.z && (ra.y ^ ra.w ^ rb.y) == rb.w;
            }
            h.t = __uint_as_float(tbits);
            p.state = ST_EXTEND;
            /* The record counts only if it is this launch's (epoch / stamp) and whole (check word).  Anything else -- measured: a line of the
             * launch before last still sitting in this XCD's L2, about one 16x16 region x frame in 300 renders of a 200 x 120 frame, seen
             * only where the buffer's previous content differed (a new scene) -- and the lane walks its camera ray itself in slot 1
             * below like any other pending ray: never a wrong hit, only a slower one. */
            if (mine) path_on_closest<F>(p, sc, ds, pf, tbits != 0xbf800000u, h);
            /* option debug_prepass_rejects: how often that happens (round 4: never in 10^4 renders; scripts/microbench/l2_stale.hip finds the kernel boundary
             * coherent) */
            else if (tg.debugCounters) atomicAdd(&tg.debugCounters[0], 1u);
        }
        /* ---- slot 1: the bounce ray (or one step of the SSS walk) ---- */
        auto slot1 = [&]() __attribute__((always_inline)) {
            float travel = 0.0f;
            if ((F & FEAT_SSS) && p.state == ST_SSS) travel = sss_travel(p, pf);
            Hit h; uint32_t nb = 0, nt = 0;
            bool isHit;
            const WalkAddr wa = walk_addr();
#ifdef PT_LDS_STASH
            if (STASH) { uint32_t* st = stash_at();
                STASH_PUT(st, 0, p.T.x); STASH_PUT(st, 1, p.T.y); STASH_PUT(st, 2, p.T.z); STASH_PUT(st, 3, p.L.x); STASH_PUT(st, 4, p.L.y); STASH_PUT(st, 5, p.L.z);
                STASH_PUT(st, 6, p.seed); }
#endif
            /* instanced scenes, tuned copies */
            if (TWOLEVEL) isHit = traverse_instanced<COUNT, ALPHA, HYBRID>(sc, ds, p.ro, p.rd, h, wa.stack, BLOCK, nb, nt, wa.overflow);
            /* two-level scenes */
            else if ((F & FEAT_EXT) && ds.numInstances) isHit = traverse_instanced<true, true>(sc, ds, p.ro, p.rd, h, wa.stack, BLOCK, nb, nt);
            else isHit = traverse<RAY_COUNTERS, ALPHA, HYBRID, NODEC, COUNT, (F & FEAT_SSS) != 0, LDS_STEPS>(sc, ds, p.ro, p.rd, h, wa.stack, BLOCK, nb, nt, prof,
                wa.overflow);
#ifdef PT_LDS_STASH
            if (STASH) { const uint32_t* st = stash_at();
                p.T = tb3_make(STASH_GET(st, 0), STASH_GET(st, 1), STASH_GET(st, 2)); p.L = tb3_make(STASH_GET(st, 3), STASH_GET(st, 4), STASH_GET(st, 5));
                p.seed = STASH_GET(st, 6); }
#endif
#if TB_EXP_DOUBLE == 2
            { Hit h2; uint32_t nb2 = 0, nt2 = 0; const tb3 o2 = tb3_make(exp_opaque(p.ro.x), exp_opaque(p.ro.y), exp_opaque(p.ro.z));
              const bool hit2 = traverse<RAY_COUNTERS, ALPHA, HYBRID, NODEC, false, (F & FEAT_SSS) != 0, LDS_STEPS>(sc, ds, o2, p.rd, h2, wa.stack, BLOCK, nb2, nt2, nullptr, wa.overflow);
              if (exp_never(h2.t, h2.u, h2.v, h2.t) && hit2 && h2.prim == 77u) p.flags |= 0x40000000u; }
#endif
#if TB_EXP_DOUBLE == 5
            if (!(F & FEAT_SSS) || p.state == ST_EXTEND) { Path q = p; q.seed = exp_opaque(p.seed); q.rd.x = exp_opaque(p.rd.x); q.ro.x = exp_opaque(p.ro.x); q.T.x = exp_opaque(p.T.x);
              Hit h2 = h; h2.u = exp_opaque(h.u); h2.t = exp_opaque(h.t); h2.prim = (uint32_t)__float_as_uint(exp_opaque(__uint_as_float(h.prim)));
              path_on_closest<F>(q, sc, ds, pf, isHit, h2);
              if (exp_never(q.L.x + q.L.y + q.L.z + q.contrib.x + q.contrib.y + q.contrib.z, q.seed + q.rd.x + q.rd.y + q.rd.z + q.ro.x + q.ro.y + q.ro.z,
                  q.N.x + q.N.y + q.N.z + q.Nd.x + q.Nd.y + q.Nd.z + q.nDotD + q.albedo.x + q.albedo.y + q.albedo.z + q.roughness + q.specCoef,
                  q.nextOrigin.x + q.nextOrigin.y + q.nextOrigin.z + (float)(q.state + q.flags + (uint32_t)q.matFlags))) p.flags |= 0x40000000u; }
#endif
            if (COUNT) { cBoxes += nb; cTris += nt; cRays++; if (isHit) cHits++; prof_hit(prof, PROF_CLOSEST); }
            p.lastBoxes = nb; p.lastTris = nt;
            /* OutputRayStats runs after every query, RayGenCommon.h:414,537-543 */
            if ((F & FEAT_EXT) && pf.OutputMode == TB_OUTPUT_TYPE_HEATMAP) p.flags |= F_HEATMAP;
            if (!(F & FEAT_SSS) || p.state == ST_EXTEND) {
                if ((F & FEAT_EXT) && tg.stats && p.bounce == 0 && PX == pf.SelectedPixelX && PY == pf.SelectedPixelY && isHit) output_selected_pixel(tg.stats,
                    sc, h);
                path_on_closest<F>(p, sc, ds, pf, isHit, h);
            } else {
                path_on_sss(p, sc, pf, isHit, h, travel);
                /* a walk that is still inside after TB_COSTLY_STEP steps: one count for its region of the frame (TbDeviceTargets::regionCost: the next launch starts there) */
                if constexpr (GROUPS && !COUNT) { if (tg.regionCost && p.state == ST_SSS && p.sssStep == TB_COSTLY_STEP)
                    atomicAdd(&tg.regionCost[((PY >> 4) & 1023u) << 10 | ((PX >> 4) & 1023u)], 1u); }
            }
        };
        if (!PRIMARY) slot1();
        /* ---- slot 2: the NEE shadow feeler, for the lanes that have one ---- */
        if constexpr (!(F & FEAT_MIX)) {
            /* Feature sets without mix materials: judging the feeler draws no random number and only adds to L, so the bounce is
             * finished FIRST (path_scatter: next direction, throughput, Russian roulette -- the same rand() calls in the same order)
             * and the feeler is traced afterwards.  What stays live across its walk is then the compact between-bounces state
             * (next ray, T, L, seed) plus the feeler and its contribution, instead of the whole shading state of the bounce
             * (normals, material, previous direction ...): fewer registers at the kernel's widest point. */
            const bool feeler = p.state == ST_SHADOW;
            const tb3 sro = p.ro, srd = p.rd, contrib = p.contrib;
            if (feeler) p.state = ST_SCATTER;
#if TB_EXP_DOUBLE == 6
            if (p.state == ST_SCATTER) { Path q = p; q.seed = exp_opaque(p.seed); q.N.x = exp_opaque(p.N.x); q.prevDir.x = exp_opaque(p.prevDir.x); q.T.x = exp_opaque(p.T.x);
              q.Nd.x = exp_opaque(p.Nd.x); q.albedo.x = exp_opaque(p.albedo.x); q.nextOrigin.x = exp_opaque(p.nextOrigin.x);
              path_scatter<F>(q, pf);
              if (exp_never(q.T.x + q.T.y + q.T.z, q.seed + q.rd.x + q.rd.y + q.rd.z, q.ro.x + q.ro.y + q.ro.z, (float)(q.state + q.flags + (uint32_t)q.bounce))) p.flags |= 0x40000000u; }
#endif
            if (p.state == ST_SCATTER) { if (COUNT) prof_hit(prof, PROF_SCATTER); path_scatter<F, ADAPTIVE>(p, pf); }
            if (feeler) {
                Hit h; uint32_t nb = 0, nt = 0;
                bool isHit;
                const WalkAddr wa = walk_addr();
#if TB_EXP_DOUBLE == 2
                { Hit h2; uint32_t nb2 = 0, nt2 = 0; const tb3 o2 = tb3_make(exp_opaque(sro.x), exp_opaque(sro.y), exp_opaque(sro.z));
                  const bool hit2 = traverse<RAY_COUNTERS, ALPHA, HYBRID, NODEC, false, (F & FEAT_SSS) != 0, LDS_STEPS>(sc, ds, o2, srd, h2, wa.stack, BLOCK, nb2, nt2, nullptr, wa.overflow);
                  if (exp_never(h2.t, h2.u, h2.v, h2.t) && hit2 && h2.prim == 77u) p.flags |= 0x40000000u; }
#endif
#ifdef PT_LDS_STASH
                if (STASH) { uint32_t* st = stash_at();
                    STASH_PUT(st, 0, p.T.x); STASH_PUT(st, 1, p.T.y); STASH_PUT(st, 2, p.T.z); STASH_PUT(st, 3, p.L.x); STASH_PUT(st, 4, p.L.y); STASH_PUT(st, 5, p.L.z);
                    STASH_PUT(st, 6, p.seed);
                    if (PT_LDS_STASH >= 13) { STASH_PUT(st, 7, p.ro.x); STASH_PUT(st, 8, p.ro.y); STASH_PUT(st, 9, p.ro.z);
                        STASH_PUT(st, 10, p.rd.x); STASH_PUT(st, 11, p.rd.y); STASH_PUT(st, 12, p.rd.z); } }
#endif
                /* instanced scenes, tuned copies */
                if (TWOLEVEL) isHit = traverse_instanced<COUNT, ALPHA, HYBRID>(sc, ds, sro, srd, h, wa.stack, BLOCK, nb, nt, wa.overflow);
            else if ((F & FEAT_EXT) && ds.numInstances) isHit = traverse_instanced<true, true>(sc, ds, sro, srd, h, wa.stack, BLOCK, nb, nt);
                else isHit = traverse<RAY_COUNTERS, ALPHA, HYBRID, NODEC, COUNT, (F & FEAT_SSS) != 0, LDS_STEPS>(sc, ds, sro, srd, h, wa.stack, BLOCK, nb, nt, prof,
                    wa.overflow);
#ifdef PT_LDS_STASH
                if (STASH) { const uint32_t* st = stash_at();
                    p.T = tb3_make(STASH_GET(st, 0), STASH_GET(st, 1), STASH_GET(st, 2)); p.L = tb3_make(STASH_GET(st, 3), STASH_GET(st, 4), STASH_GET(st, 5));
                    p.seed = STASH_GET(st, 6);
                    if (PT_LDS_STASH >= 13) { p.ro = tb3_make(STASH_GET(st, 7), STASH_GET(st, 8), STASH_GET(st, 9));
                        p.rd = tb3_make(STASH_GET(st, 10), STASH_GET(st, 11), STASH_GET(st, 12)); } }
#endif
                if (COUNT) { cBoxes += nb; cTris += nt; cRays++; if (isHit) cHits++; prof_hit(prof, PROF_SHADOW); }
                p.lastBoxes = nb; p.lastTris = nt;
                path_apply_shadow<F>(p, sc, ds, pf, isHit, h, srd, contrib);
            }
        } else {
        if (p.state == ST_SHADOW) {
            Hit h; uint32_t nb = 0, nt = 0;
            bool isHit;
            const WalkAddr wa = walk_addr();
#ifdef PT_LDS_STASH
            if (STASH) { uint32_t* st = stash_at();
                STASH_PUT(st, 0, p.T.x); STASH_PUT(st, 1, p.T.y); STASH_PUT(st, 2, p.T.z); STASH_PUT(st, 3, p.L.x); STASH_PUT(st, 4, p.L.y); STASH_PUT(st, 5, p.L.z);
                STASH_PUT(st, 6, p.seed); }
#endif
            /* instanced scenes, tuned copies */
            if (TWOLEVEL) isHit = traverse_instanced<COUNT, ALPHA, HYBRID>(sc, ds, p.ro, p.rd, h, wa.stack, BLOCK, nb, nt, wa.overflow);
            else if ((F & FEAT_EXT) && ds.numInstances) isHit = traverse_instanced<true, true>(sc, ds, p.ro, p.rd, h, wa.stack, BLOCK, nb, nt);
            else isHit = traverse<RAY_COUNTERS, ALPHA, HYBRID, NODEC, COUNT, (F & FEAT_SSS) != 0, LDS_STEPS>(sc, ds, p.ro, p.rd, h, wa.stack, BLOCK, nb, nt, prof,
                wa.overflow);
#ifdef PT_LDS_STASH
            if (STASH) { const uint32_t* st = stash_at();
                p.T = tb3_make(STASH_GET(st, 0), STASH_GET(st, 1), STASH_GET(st, 2)); p.L = tb3_make(STASH_GET(st, 3), STASH_GET(st, 4), STASH_GET(st, 5));
                p.seed = STASH_GET(st, 6); }
#endif
            if (COUNT) { cBoxes += nb; cTris += nt; cRays++; if (isHit) cHits++; prof_hit(prof, PROF_SHADOW); }
            p.lastBoxes = nb; p.lastTris = nt;
            path_on_shadow<F>(p, sc, ds, pf, isHit, h);
        }
        if (p.state == ST_SCATTER) { if (COUNT) prof_hit(prof, PROF_SCATTER); path_scatter<F, ADAPTIVE>(p, pf); }
        }
        if (PRIMARY && (p.state == ST_EXTEND || p.state == ST_SSS)) slot1();
    }
#ifdef TB_WG_TIMELINE
    if (GROUPS) {
        unsigned long long* row = tg.slotLog + (size_t)blockIdx.x * tg.slotLogCap + tg.slotLogCap;
        if (lane == 0) row[-3 - (int)wave] = wall_clock64();
        if (threadIdx.x == 0) { row[-2] = ((volatile unsigned long long*)&tlDry)[0]; row[-7] = ((volatile uint32_t*)&drawn)[0];
            for (int i = 0; i < 4; i++) row[-8 - i] = ((volatile uint32_t*)tlStat)[i]; }
    }
#endif
    if (mine) { tg.output[PIX] = acc; if (tg.jittered) tg.jittered[PIX] = jacc; }
    if (COUNT && tg.rayStats) {
        unsigned long long v[7] = {cBoxes, cTris, cHits, cMats, cLights, cSamples, cRays};
        for (int i = 0; i < 7; i++) { unsigned long long s = wave_sum(v[i]); if (lane == 0 && s) atomicAdd(&tg.rayStats[i], s); }
        for (int i = 0; i < PROF_SLOTS; i++) { unsigned long long s = wave_sum(profStore.v[i]); if (lane == 0 && s) atomicAdd(&tg.rayStats[7 + i], s); }
    }
}
#undef PX
#undef PY
#undef PIX
#ifdef PT_LDS_STASH
#undef STASH_PUT
#undef STASH_GET
#endif
