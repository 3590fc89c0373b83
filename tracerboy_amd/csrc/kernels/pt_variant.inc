/* pt_variant.inc -- one translation unit per copy of the lock-step kernel.  The including file defines PT_COPY, the name of its row in pt_copies.h:
 * the row says what is compiled here (pt_persistent always, pt_stream, the wavefront and pooled kernels of a base copy) and, through pt_pick_form,
 * which kernel a launch runs.  One launcher per copy, pt_launch_persistent_<copy>(..., mode) (pt_launch.h). */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"

/* the row, as the kernel sources read it */
#define PT_FEATURES PT_FIELD(PT_F_FEATURES, PT_COPY)
#define PT_NAME PT_COPY
#define PT_PERSISTENT_ATTR __attribute__((amdgpu_waves_per_eu(PT_FIELD(PT_F_BOUND, PT_COPY))))
#if PT_FIELD(PT_F_ROLE, PT_COPY) == PT_ROLE_LDS_GROUPS
#define PT_LDS_WALK 1 /* this copy's kernels -- scenes in LDS, whole stack in LDS, nothing else -- walk with the LDS steps (pt_device.hpp traverse) */
#endif
#if PT_FIELD(PT_F_STASH, PT_COPY) > 0
#define PT_LDS_STASH PT_FIELD(PT_F_STASH, PT_COPY) /* LDS entries per lane behind the stacks (pt_persistent.inc) */
#endif

namespace {
#include "pt_persistent.inc"
#if PT_FIELD(PT_F_STREAMING, PT_COPY)
#include "pt_stream.inc"
#endif

constexpr PtCopy kCopy = PT_FIELD(PT_F_INIT, PT_COPY);
constexpr PtFormSet kForms = pt_forms_of(kCopy); /* what this unit instantiates */

struct PtLaunch { /* a launcher's arguments, and what it derived from them */
    hipStream_t stream; const TbDeviceScene* ds; const TbPerFrameConstants* pf; const TbDeviceTargets* tg; uint32_t W, H, firstFrame, numFrames;
    const TbTileMap* tiles; uint32_t blocks; size_t lds; int numCUs; bool guided;
};

/* One kernel launch: the LDS attribute, and for a resident grid -- one that draws its work items from a list -- the occupancy query and
 * min(items, 2 x residency) workgroups (those past residency find the list empty).  prepass: the grid of pt_primary / pt_first, one item per region
 * and frame, residency capped at 8 workgroups per CU.  Otherwise the lock-step kernel: in frame-group mode (pt_scene.h) a resident grid over
 * regions x groups with its slot logs and work counter cleared, else one workgroup per owned region. */
template <class K> hipError_t launchKernel(K kernel, const PtLaunch& a, bool prepass)
{
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds); if (e != hipSuccess) return e;
    const TbDeviceTargets* tg = a.tg;
    dim3 grid(a.blocks);
    if (prepass || tg->samples) {
        int perCU = 0; e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, BLOCK, a.lds); if (e != hipSuccess) return e;
        uint32_t lgG = 0; while ((2u << lgG) <= tg->frameGroup) lgG++;
        const uint64_t items = (uint64_t)a.blocks * (prepass ? a.numFrames : tb_fg_groups(a.numFrames, lgG, a.guided ? 1u : 0u, 0xffffffffu, nullptr, nullptr)),
            resident = (uint64_t)(perCU > 0 ? (prepass && perCU > 8 ? 8 : perCU) : 1) * a.numCUs;
        grid.x = (uint32_t)(items < 2 * resident ? items : 2 * resident);
        if (prepass) { if (!items) return hipSuccess; }
        else {
            if (grid.x == 0) grid.x = 1; /* a zero-frame launch (the host warming a stream up for this kernel): one workgroup that finds nothing */
            if (!tg->slotLog || !tg->slotLogCap || grid.x > 16u * (uint32_t)a.numCUs) return hipErrorInvalidValue;
            e = hipMemsetAsync(tg->slotLog, 0, (size_t)grid.x * tg->slotLogCap * 8, a.stream); if (e != hipSuccess) return e;
            e = hipMemsetAsync(tg->workCounter, 0, 512, a.stream); if (e != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), a.lds, a.stream, *a.ds, *a.pf, *tg, a.W, a.H, a.firstFrame, a.numFrames, *a.tiles);
    return hipSuccess;
}

/* from a form to its kernels: the I-th of this copy's forms and on; the one place that spells template arguments */
template <int I = 0> hipError_t launchForm(const PtForm& f, const PtLaunch& a)
{
    if constexpr (I < kForms.n) {
        constexpr PtForm k = pt_form_of(kForms.code[I]);
        if (f.code() != kForms.code[I]) return launchForm<I + 1>(f, a);
        if constexpr (k.pre == PT_PRE_PRIMARY) { const hipError_t e = launchKernel(pt_primary<PT_FEATURES, k.hybrid, k.nodeC>, a, true); if (e != hipSuccess) return e; }
        if constexpr (k.pre == PT_PRE_FIRST) { const hipError_t e = launchKernel(pt_first<PT_FEATURES, k.hybrid>, a, true); if (e != hipSuccess) return e; }
#if PT_FIELD(PT_F_STREAMING, PT_COPY)
        if constexpr (k.stream) return launchKernel(pt_stream<PT_FEATURES, k.sceneLds, k.count>, a, false);
        else
#endif
        return launchKernel(pt_persistent<PT_FEATURES, k.sceneLds, k.count, k.groups, k.hybrid, k.nodeC, k.twoLevel, k.primary, k.first, k.guided, k.adaptive>, a,
            false);
    } else return hipErrorInvalidValue;
}
}

extern "C" hipError_t PT_CAT(pt_launch_persistent_, PT_COPY)(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg,
                                                            uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles,
                                                            int sceneInLds, int countRays, int mode)
{
    /* (the adaptive launch's grid is the owned region count, an upper bound, so that the host reads nothing back; a workgroup past the live count
     * exits at once) */
    const bool adaptive = mode == PT_MODE_ADAPTIVE;
    PtLaunch a{stream, ds, pf, tg, W, H, firstFrame, numFrames, tiles, tb_persistent_grid(W, H, *tiles), 0, 0, false};
    if (!adaptive) {
        if (a.blocks == 0) return hipSuccess; /* this rank owns no tile */
        const hipError_t e = pt_device_cus(&a.numCUs); if (e != hipSuccess) return e;
    }
    /* the grid of a split stack is at most 2 x residency, residency at most 8 workgroups per CU */
    const PtShape shape{mode, tg->samples != nullptr, tg->liveList && (!adaptive || tg->liveCount), countRays != 0, sceneInLds != 0, ds->numInstances != 0,
        ds->nodesC != nullptr, ds->stackOverflow != nullptr, ds->stackOverflowLanes >= 2u * 8u * (uint32_t)a.numCUs * BLOCK, tg->primaryHits != nullptr,
        tg->firstBounce != 0, tg->fgGuided != 0};
    const PtPick pick = pt_pick_form(kCopy, shape);
    if (!pick.ok) return hipErrorInvalidValue;
    if (adaptive && (a.blocks == 0 || numFrames == 0)) return hipSuccess;
    a.lds = (size_t)ds->stackDepth * BLOCK * 4 + (sceneInLds ? ds->ldsBlobBytes : 0);
    if (kCopy.stash && !sceneInLds && tg->samples && !ds->numInstances) a.lds += (size_t)kCopy.stash * BLOCK * 4; /* the stash behind the stacks */
    a.guided = pt_shrinking_groups(shape);
    const hipError_t e = launchForm(pick.form, a);
    return e != hipSuccess ? e : hipGetLastError();
}

/* ---- wavefront pipeline (pipeline 2): one launcher per feature set, one stage per call ---------------------- */
#if !(PT_FEATURES & PT_FEAT_EXT) && PT_FIELD(PT_F_ROLE, PT_COPY) == PT_ROLE_BASE
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
