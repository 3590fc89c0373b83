/* pt_split_variant.inc -- one translation unit per feature set of the split-role kernel (pipeline 4, pt_split.inc).
 * The including file defines PT_FEATURES, PT_NAME and (optionally) PT_SPLIT_ATTR. */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"

namespace {
#include "pt_split.inc"
}

/* LDS of one workgroup: traversal stacks + scene image + 48-B ray slots (two per shading lane) + the queue + control words */
static size_t split_lds_bytes(const TbDeviceScene* ds, const TbSplitParams* sp, int sceneInLds)
{
    return (size_t)ds->stackDepth * sp->travWaves * 64 * 4 + (sceneInLds ? ((size_t)ds->ldsBlobBytes + 15) / 16 * 16 : 0) + (size_t)sp->shadeWaves * 128 * 48 +
        (size_t)sp->ringCap * 4 + 16;
}

/* query != null: no launch, *query = workgroups per CU the launch would have (the host sizes the split stack's overflow from it) */
extern "C" hipError_t PT_CAT(pt_launch_split_, PT_NAME)(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg,
    const TbSplitParams* sp,
                                                       uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles, int sceneInLds,
                                                           int* query)
{
    if (!tg->samples || !tg->workCounter || !tg->frameGroup || !sp->travWaves || !sp->shadeWaves || (sp->travWaves + sp->shadeWaves) * 64 > 1024)
        return hipErrorInvalidValue;
    if ((sp->ringCap & (sp->ringCap - 1)) || sp->ringCap < 256u * sp->shadeWaves || ds->numInstances || ds->nodesC) return hipErrorInvalidValue;
    const uint32_t regions = tb_persistent_grid(W, H, *tiles);
    if (regions == 0) { if (query) *query = 0; return hipSuccess; } /* this rank owns no tile */
    /* a claimed item is group << 20 | 8x8 tile */
    if (4ull * regions > 0xfffffull || (numFrames + tg->frameGroup - 1) / tg->frameGroup > 4095u) return hipErrorInvalidValue;
    const size_t lds = split_lds_bytes(ds, sp, sceneInLds);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const uint32_t threads = (sp->travWaves + sp->shadeWaves) * 64;
    int numCUs = 0;
    { const hipError_t e = pt_device_cus(&numCUs); if (e != hipSuccess) return e; }
#define SPLIT_LAUNCH(...) do { \
        hipError_t e = hipFuncSetAttribute((const void*)__VA_ARGS__, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; \
        int perCU = 0; e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, __VA_ARGS__, (int)threads, lds); if (e != hipSuccess) return e; \
        if (perCU < 1) return hipErrorInvalidValue; \
        if (query) { *query = perCU; return hipSuccess; } \
        if (ds->stackOverflow && ds->stackOverflowLanes < (uint32_t)perCU * (uint32_t)numCUs * sp->travWaves * 64u) return hipErrorInvalidValue; \
        const uint64_t items = 4ull * regions * ((numFrames + tg->frameGroup - 1) / tg->frameGroup), resident = (uint64_t)perCU * numCUs; \
        uint32_t grid = (uint32_t)((items + sp->shadeWaves - 1) / sp->shadeWaves < resident ? (items + sp->shadeWaves - 1) / sp->shadeWaves : resident); \
        if (grid == 0) grid = 1; /* a zero-frame launch (the host warming a stream up): one workgroup that finds nothing */ \
        e = hipMemsetAsync(tg->workCounter, 0, 512, stream); if (e != hipSuccess) return e; \
        hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(threads), lds, stream, *ds, *pf, *tg, *sp, W, H, firstFrame, numFrames, *tiles); } while (0)
    if (sp->prof) { /* the counting copy (option split_profile) */
        if (ds->stackOverflow) { if (sceneInLds) return hipErrorInvalidValue; SPLIT_LAUNCH(pt_split<PT_FEATURES, false, true, true>); }
        else if (sceneInLds) SPLIT_LAUNCH(pt_split<PT_FEATURES, true, false, true>);
        else SPLIT_LAUNCH(pt_split<PT_FEATURES, false, false, true>);
    } else if (ds->stackOverflow) { if (sceneInLds) return hipErrorInvalidValue; SPLIT_LAUNCH(pt_split<PT_FEATURES, false, true>); }
    else if (sceneInLds) SPLIT_LAUNCH(pt_split<PT_FEATURES, true, false>);
    else SPLIT_LAUNCH(pt_split<PT_FEATURES, false, false>);
#undef SPLIT_LAUNCH
    return hipGetLastError();
}
