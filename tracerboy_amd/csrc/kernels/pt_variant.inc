/* pt_variant.inc -- one translation unit per feature set.  The including file defines
 *   PT_FEATURES  (bit mask of PT_FEAT_*)   PT_NAME (identifier suffix)   PT_COUNT (0/1: also build the counting kernels)
 * Two kernels per feature set: pt_stream (pipeline 1, resumable BVH walk) and pt_persistent (pipeline 0, lock-step bounce). */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"

/* PT_ONLY_PERSISTENT: a second copy of a feature set at a higher occupancy (fewer VGPRs, more scratch), pipeline 0 only */
namespace {
#include "pt_persistent.inc"
#ifndef PT_ONLY_PERSISTENT
#include "pt_stream.inc"
#endif
}

#define PT_CAT2(a, b) a##b
#define PT_CAT(a, b) PT_CAT2(a, b)

extern "C" hipError_t PT_CAT(pt_launch_persistent_, PT_NAME)(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf,
    const TbDeviceTargets* tg,
                                                            uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles,
                                                            int sceneInLds, int countRays, int pipeline)
{
    uint32_t blocks = tb_persistent_grid(W, H, *tiles);
    if (blocks == 0) return hipSuccess; /* this rank owns no tile */
    size_t lds = (size_t)ds->stackDepth * BLOCK * 4 + (sceneInLds ? ds->ldsBlobBytes : 0);
#ifdef PT_LDS_STASH
    if (!sceneInLds && tg->samples && !ds->numInstances) lds += (size_t)PT_LDS_STASH * BLOCK * 4; /* the feature set's stash behind the stacks (pt_persistent.inc) */
#endif
    /* groups that shrink over the end of the launch (TbDeviceTargets::fgGuided): compiled into the frame-group kernels of scenes in LDS only (a copy of
     * its own, pt_persistent.inc GUIDED); every other launch has equal groups whatever the host asked for -- the host asks for it there only */
    const bool guidedLaunch = tg->samples && tg->fgGuided && sceneInLds && !ds->stackOverflow && !ds->numInstances && !ds->nodesC && !tg->primaryHits;
    dim3 grid(blocks), block(BLOCK);
    int numCUs = 0; /* of the CURRENT device (a process may drive several: tb_create_multi), cached per device ordinal */
    {
        static int cuCache[64] = {0};
        int dev = 0; hipError_t e = hipGetDevice(&dev); if (e != hipSuccess) return e;
        if (dev < 0 || dev >= 64 || !cuCache[dev]) { e = hipDeviceGetAttribute(&numCUs, hipDeviceAttributeMultiprocessorCount, dev);
            if (e != hipSuccess) return e; if (dev >= 0 && dev < 64) cuCache[dev] = numCUs; }
        else numCUs = cuCache[dev];
    }
#define PT_LAUNCH(...) do { \
        hipError_t e = hipFuncSetAttribute((const void*)__VA_ARGS__, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e; \
        if (tg->samples) { /* frame-group mode (pt_scene.h): a resident grid that draws its work items from *workCounter */ \
            int perCU = 0; e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, __VA_ARGS__, BLOCK, lds); if (e != hipSuccess) return e; \
            uint32_t lgG = 0; while ((2u << lgG) <= tg->frameGroup) lgG++; \
            const uint64_t items = (uint64_t)blocks * tb_fg_groups(numFrames, lgG, guidedLaunch ? 1u : 0u, 0xffffffffu, nullptr, nullptr), \
                resident = (uint64_t)(perCU > 0 ? perCU : 1) * numCUs; \
            grid.x = (uint32_t)(items < 2 * resident ? items : 2 * resident); /* workgroups past residency find the list empty */ \
            if (grid.x == 0) grid.x = 1; /* a zero-frame launch (the host warming a stream up for this kernel): one workgroup that finds nothing */ \
            if (!tg->slotLog || !tg->slotLogCap || grid.x > 16u * (uint32_t)numCUs) return hipErrorInvalidValue; \
            e = hipMemsetAsync(tg->slotLog, 0, (size_t)grid.x * tg->slotLogCap * 8, stream); if (e != hipSuccess) return e; \
            e = hipMemsetAsync(tg->workCounter, 0, 512, stream); if (e != hipSuccess) return e; } \
        hipLaunchKernelGGL((__VA_ARGS__), grid, block, lds, stream, *ds, *pf, *tg, W, H, firstFrame, numFrames, *tiles); } while (0)
#ifndef PT_ONLY_PERSISTENT
#define PT_PICK(L, C) do { if (pipeline == 1) PT_LAUNCH(pt_stream<PT_FEATURES, L, C>); else PT_LAUNCH(pt_persistent<PT_FEATURES, L, C, false>); } while (0)
#else
#define PT_PICK(L, C) do { if (pipeline != 0) return hipErrorInvalidValue; PT_LAUNCH(pt_persistent<PT_FEATURES, L, C, false>); } while (0)
#endif
    /* The list-driven frame-group launch (pt_launch.h PT_LAUNCH_LIVE_GROUPS in place of a pipeline number; TbDeviceTargets::liveList): this copy's
     * frame-group kernel over the live list -- whole or split stack, scene in LDS or from memory, one or two levels; no counters, no hit records,
     * layout B, equal groups.  The grid, the slot logs and the stash are the frame-group launch's, with the owned regions as the upper bound of
     * the list's blocks (PT_LAUNCH). */
    if (pipeline == PT_LAUNCH_LIVE_GROUPS) {
        if (!tg->samples || !tg->liveList || countRays || tg->primaryHits || ds->nodesC || tg->fgGuided) return hipErrorInvalidValue;
#define PT_LIVE(L, HY, TL) PT_LAUNCH(pt_persistent<PT_FEATURES, L, false, true, HY, false, TL, false, false, false, true>)
#ifdef PT_ONLY_LDS_GROUPS
        if (!sceneInLds || ds->numInstances || ds->stackOverflow) return hipErrorInvalidValue;
        PT_LIVE(true, false, false);
#elif defined(PT_ONLY_PERSISTENT)
        if (ds->stackOverflow && ds->stackOverflowLanes < 2u * 8u * (uint32_t)numCUs * BLOCK) return hipErrorInvalidValue;
        if (ds->numInstances) { if (sceneInLds) return hipErrorInvalidValue; if (ds->stackOverflow) PT_LIVE(false, true, true); else PT_LIVE(false, false, true); }
        else if (ds->stackOverflow) { if (sceneInLds) PT_LIVE(true, true, false); else PT_LIVE(false, true, false); }
        else if (sceneInLds) PT_LIVE(true, false, false); else PT_LIVE(false, false, false);
#else
        if (ds->stackOverflow) return hipErrorInvalidValue; /* a base copy: whole stack in LDS */
#if !(PT_FEATURES & PT_FEAT_EXT)
        if (ds->numInstances) return hipErrorInvalidValue; /* of the base copies only the full feature set walks two levels */
#endif
        if (sceneInLds) PT_LIVE(true, false, false); else PT_LIVE(false, false, false);
#endif
#undef PT_LIVE
        return hipGetLastError();
    }
    if (tg->samples && (countRays || pipeline != 0)) return hipErrorInvalidValue; /* frame groups: pt_persistent without counters only */
#ifdef PT_ONLY_LDS_GROUPS
    /* a copy for scenes in LDS (pt_variant_matte6.hip): the frame-group kernels with the whole stack in LDS, nothing else */
    if (!tg->samples || !sceneInLds || countRays || ds->numInstances || tg->primaryHits || ds->nodesC || ds->stackOverflow) return hipErrorInvalidValue;
    if (guidedLaunch) PT_LAUNCH(pt_persistent<PT_FEATURES, true, false, true, false, false, false, false, false, true>);
    else PT_LAUNCH(pt_persistent<PT_FEATURES, true, false, true>);
#else
#if PT_COUNT
    if (countRays) { if (sceneInLds) PT_PICK(true, true); else PT_PICK(false, true); return hipGetLastError(); }
#else
    if (countRays) return hipErrorInvalidValue;
#endif
#ifdef PT_ONLY_PERSISTENT
    /* two-level (instanced) scenes: the tuned walk lives in the frame-group kernels of this copy */
    if (ds->numInstances) {
        if (!tg->samples || sceneInLds || ds->nodesC) return hipErrorInvalidValue;
        if (ds->stackOverflow) {
            if (ds->stackOverflowLanes < 2u * 8u * (uint32_t)numCUs * BLOCK) return hipErrorInvalidValue;
            PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, true, false, true>);
        } else PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, false, false, true>);
        return hipGetLastError();
    }
#elif !(PT_FEATURES & PT_FEAT_EXT)
    if (ds->numInstances) return hipErrorInvalidValue; /* of the base copies only the full feature set walks two levels */
#endif
#if (defined(PT_ONLY_PERSISTENT) || defined(PT_PRIMARY_IN_BASE)) && !(PT_FEATURES & PT_FEAT_EXT)
    /* primary-visibility pre-pass (TbDeviceTargets::primaryHits): frame-group kernels of the higher-occupancy copies, scenes fetched
     * from memory, one level; the pre-pass is a resident grid with the stack layout of the kernel it feeds */
    if (tg->primaryHits) {
        if (!tg->samples || sceneInLds || ds->numInstances) return hipErrorInvalidValue;
        if (ds->stackOverflow && ds->stackOverflowLanes < 2u * 8u * (uint32_t)numCUs * BLOCK) return hipErrorInvalidValue;
#ifndef PT_ONLY_PERSISTENT
        if (ds->stackOverflow || ds->nodesC) return hipErrorInvalidValue; /* a base copy: whole stack in LDS, layout B */
#endif
#define PT_PRIMARY(HY, NC) do { \
        hipError_t e = hipFuncSetAttribute((const void*)pt_primary<PT_FEATURES, HY, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e; \
        int perCU = 0; e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, pt_primary<PT_FEATURES, HY, NC>, BLOCK, lds); if (e != hipSuccess) return e; \
        const uint64_t items = (uint64_t)blocks * numFrames, resident = (uint64_t)(perCU > 0 ? (perCU > 8 ? 8 : perCU) : 1) * numCUs; \
        if (items) hipLaunchKernelGGL((pt_primary<PT_FEATURES, HY, NC>), dim3((uint32_t)(items < 2 * resident ? items : 2 * resident)), block, lds, stream, \
            *ds, *pf, *tg, W, H, firstFrame, numFrames, *tiles); \
        PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, HY, NC, false, true>); } while (0)
        /* first-bounce pass (TbDeviceTargets::firstBounce): pt_first in place of pt_primary, the lock-step kernel's FIRST form; layout B only */
#define PT_FIRST(HY) do { \
        if (ds->nodesC) return hipErrorInvalidValue; \
        hipError_t e = hipFuncSetAttribute((const void*)pt_first<PT_FEATURES, HY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e; \
        int perCU = 0; e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, pt_first<PT_FEATURES, HY>, BLOCK, lds); if (e != hipSuccess) return e; \
        const uint64_t items = (uint64_t)blocks * numFrames, resident = (uint64_t)(perCU > 0 ? (perCU > 8 ? 8 : perCU) : 1) * numCUs; \
        if (items) hipLaunchKernelGGL((pt_first<PT_FEATURES, HY>), dim3((uint32_t)(items < 2 * resident ? items : 2 * resident)), block, lds, stream, \
            *ds, *pf, *tg, W, H, firstFrame, numFrames, *tiles); \
        PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, HY, false, false, true, true>); } while (0)
        if (tg->firstBounce) {
#ifdef PT_ONLY_PERSISTENT
            if (ds->stackOverflow) PT_FIRST(true); else PT_FIRST(false);
#else
            PT_FIRST(false);
#endif
            return hipGetLastError();
        }
#ifdef PT_ONLY_PERSISTENT
        if (ds->stackOverflow) { if (ds->nodesC) PT_PRIMARY(true, true); else PT_PRIMARY(true, false); }
        else { if (ds->nodesC) PT_PRIMARY(false, true); else PT_PRIMARY(false, false); }
#else
        PT_PRIMARY(false, false);
#endif
#undef PT_FIRST
#undef PT_PRIMARY
        return hipGetLastError();
    }
#else
    if (tg->primaryHits) return hipErrorInvalidValue; /* the host asks for the pre-pass only where it is compiled in */
#endif
#ifdef PT_ONLY_PERSISTENT
    /* compact nodes (layout C, tb_abi.h): compiled into the frame-group kernels of the higher-occupancy copies, scenes fetched from memory */
    if (ds->nodesC) {
        if (!tg->samples || sceneInLds) return hipErrorInvalidValue;
        if (ds->stackOverflow) {
            if (ds->stackOverflowLanes < 2u * 8u * (uint32_t)numCUs * BLOCK) return hipErrorInvalidValue;
            PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, true, true>);
        } else PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, false, true>);
        return hipGetLastError();
    }
#else
    if (ds->nodesC) return hipErrorInvalidValue; /* the host hands layout C only to the copies that have it */
#endif
#ifdef PT_ONLY_PERSISTENT
    /* split traversal stack (pt_scene.h): the tree is deeper than this copy's share of LDS; the host sized the overflow for a resident grid */
    if (tg->samples && ds->stackOverflow) {
        /* the grid is at most 2 x residency, residency at most 8 workgroups per CU */
        if (ds->stackOverflowLanes < 2u * 8u * (uint32_t)numCUs * BLOCK) return hipErrorInvalidValue;
        if (sceneInLds) PT_LAUNCH(pt_persistent<PT_FEATURES, true, false, true, true>); else PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true, true>);
        return hipGetLastError();
    }
#endif
    if (ds->stackOverflow) return hipErrorInvalidValue;
#ifdef TB_EXP_PROFILE_GROUPS
    /* experiment builds only (scripts/c2_instruction_mix.py): the frame-group kernel with the wave-occupancy profile of the counting copies
     * compiled in -- trips per phase of the very launch shape bench.py times (host option debug_profile_groups hands it tg->rayStats) */
    if (tg->samples) { if (sceneInLds) PT_LAUNCH(pt_persistent<PT_FEATURES, true, true, true>);
        else PT_LAUNCH(pt_persistent<PT_FEATURES, false, true, true>); }
#else
    if (tg->samples) { if (guidedLaunch) PT_LAUNCH(pt_persistent<PT_FEATURES, true, false, true, false, false, false, false, false, true>);
        else if (sceneInLds) PT_LAUNCH(pt_persistent<PT_FEATURES, true, false, true>);
        else PT_LAUNCH(pt_persistent<PT_FEATURES, false, false, true>); }
#endif
    else if (sceneInLds) PT_PICK(true, false); else PT_PICK(false, false);
#endif /* PT_ONLY_LDS_GROUPS */
#undef PT_PICK
#undef PT_LAUNCH
    return hipGetLastError();
}

#ifndef PT_ONLY_PERSISTENT
/* The adaptive launch (TbDeviceTargets::liveList, pt_scene.h; the host has run pt_launch_live_list on the same stream): the one-pixel-per-lane form of
 * the base copy over the packed live pixels.  The grid is the owned region count, an upper bound, so that the host reads nothing back; a workgroup
 * past the live count exits at once.  The full feature set's copy walks two-level scenes too, like its dense copy. */
extern "C" hipError_t PT_CAT(pt_launch_adaptive_, PT_NAME)(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg,
                                                          uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles,
                                                          int sceneInLds, int countRays, int pipeline)
{
    if (!tg->liveList || !tg->liveCount || tg->samples || tg->primaryHits || countRays || pipeline != 0 || ds->stackOverflow || ds->nodesC)
        return hipErrorInvalidValue;
#if !(PT_FEATURES & PT_FEAT_EXT)
    if (ds->numInstances) return hipErrorInvalidValue;
#endif
    const uint32_t blocks = tb_persistent_grid(W, H, *tiles);
    if (blocks == 0 || numFrames == 0) return hipSuccess;
    const size_t lds = (size_t)ds->stackDepth * BLOCK * 4 + (sceneInLds ? ds->ldsBlobBytes : 0);
#define PT_ADAPTIVE(L) do { \
        hipError_t e = hipFuncSetAttribute((const void*)pt_persistent<PT_FEATURES, L, false, false, false, false, false, false, false, false, true>, \
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e; \
        hipLaunchKernelGGL((pt_persistent<PT_FEATURES, L, false, false, false, false, false, false, false, false, true>), dim3(blocks), dim3(BLOCK), lds, \
            stream, *ds, *pf, *tg, W, H, firstFrame, numFrames, *tiles); } while (0)
    if (sceneInLds) PT_ADAPTIVE(true); else PT_ADAPTIVE(false);
#undef PT_ADAPTIVE
    return hipGetLastError();
}
#endif

/* ---- wavefront pipeline (pipeline 2): one launcher per feature set, one stage per call ---------------------- */
#if !(PT_FEATURES & PT_FEAT_EXT) && !defined(PT_ONLY_PERSISTENT)
#include "wf_types.h"
#define PT_HAS_POOLED (!(PT_FEATURES & (PT_FEAT_SSS | PT_FEAT_MIX)))   /* pipeline 3 carries no interior-walk state */
namespace {
#include "wf_kernels.inc"
#if PT_HAS_POOLED
#include "pt_pooled.inc"
#endif
}
extern "C" hipError_t PT_CAT(wf_launch_, PT_NAME)(hipStream_t stream, int stage, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const WfParams* wp,
                                                  const WfQueue* in, const WfQueue* shadow, const WfQueue* next, const WfHits* hits,
                                                  int sceneInLds,
                                                  TbFloat4* output, TbFloat4* jittered, uint32_t gridBlocks)
{
    const size_t stackBytes = 16 + (size_t)ds->stackDepth * BLOCK * 4, blobBytes = sceneInLds ? ds->ldsBlobBytes : 0;
    dim3 grid(gridBlocks), block(BLOCK);
#define WF_LAUNCH(K, LDSBYTES, ...) do { \
        hipError_t e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDSBYTES)); \
        if (e != hipSuccess) return e; \
        hipLaunchKernelGGL(K, grid, block, (LDSBYTES), stream, __VA_ARGS__); } while (0)
    switch (stage) {
    case WF_STAGE_GENERATE_EXTEND:
        if (sceneInLds) WF_LAUNCH((wf_generate_extend<PT_FEATURES, true>), stackBytes + blobBytes, *ds, *pf, *wp, *next, *hits);
        else WF_LAUNCH((wf_generate_extend<PT_FEATURES, false>), stackBytes, *ds, *pf, *wp, *next, *hits);
        break;
    case WF_STAGE_SHADE: {
        if (wp->sortByMaterial && wp->segCapacity > 65536u) return hipErrorInvalidValue; /* the index permutation is 16-bit */
        const size_t sortBytes = wp->sortByMaterial ? wf_sort_lds_bytes(wp->segCapacity) : 0;
        if (sceneInLds) WF_LAUNCH((wf_shade<PT_FEATURES, true>), 16 + blobBytes + sortBytes, *ds, *pf, *wp, *in, *hits, *shadow, *next);
        else WF_LAUNCH((wf_shade<PT_FEATURES, false>), 16 + sortBytes, *ds, *pf, *wp, *in, *hits, *shadow, *next);
        break;
    }
    case WF_STAGE_CONNECT:
        if (wp->refillBelow) {
            if (sceneInLds) WF_LAUNCH((wf_connect<PT_FEATURES, true, true>), stackBytes + blobBytes, *ds, *pf, *wp, *shadow, *next, *hits);
            else WF_LAUNCH((wf_connect<PT_FEATURES, false, true>), stackBytes, *ds, *pf, *wp, *shadow, *next, *hits);
            break;
        }
        if (sceneInLds) WF_LAUNCH((wf_connect<PT_FEATURES, true>), stackBytes + blobBytes, *ds, *pf, *wp, *shadow, *next, *hits);
        else WF_LAUNCH((wf_connect<PT_FEATURES, false>), stackBytes, *ds, *pf, *wp, *shadow, *next, *hits);
        break;
    case WF_STAGE_EXTEND:
        if (wp->refillBelow) {
            if (sceneInLds) WF_LAUNCH((wf_extend_refill<PT_FEATURES, true>), stackBytes + blobBytes, *ds, *wp, *next, *hits);
            else WF_LAUNCH((wf_extend_refill<PT_FEATURES, false>), stackBytes, *ds, *wp, *next, *hits);
            break;
        }
        if (sceneInLds) WF_LAUNCH((wf_extend<PT_FEATURES, true>), stackBytes + blobBytes, *ds, *wp, *next, *hits);
        else WF_LAUNCH((wf_extend<PT_FEATURES, false>), stackBytes, *ds, *wp, *next, *hits);
        break;
#if PT_HAS_POOLED
    case WF_STAGE_POOLED: {
        const uint32_t R = wp->pathsPerLane == 2 ? 2u : 1u;
        const size_t poolBytes = (size_t)(2u * R * BLOCK) * 28 + 16; /* 6 ray rows + the queue, + 2 counter pairs */
        const size_t bytes = (stackBytes - 16) + poolBytes + blobBytes;
#define POOLED_PICK(C) do { \
        if (R == 2) { if (sceneInLds) WF_LAUNCH((pt_pooled<PT_FEATURES, true, 2, C>), bytes, *ds, *pf, *wp); \
            else WF_LAUNCH((pt_pooled<PT_FEATURES, false, 2, C>), bytes, *ds, *pf, *wp); } \
        else { if (sceneInLds) WF_LAUNCH((pt_pooled<PT_FEATURES, true, 1, C>), bytes, *ds, *pf, *wp); \
            else WF_LAUNCH((pt_pooled<PT_FEATURES, false, 1, C>), bytes, *ds, *pf, *wp); } } while (0)
        if (wp->prof) POOLED_PICK(true); else POOLED_PICK(false);
#undef POOLED_PICK
        break;
    }
#endif
    case WF_STAGE_ACCUMULATE:
        hipLaunchKernelGGL(wf_accumulate, grid, block, 0, stream, *wp, *pf, output, jittered);
        break;
    default: return hipErrorInvalidValue;
    }
#undef WF_LAUNCH
    return hipGetLastError();
}
#endif
