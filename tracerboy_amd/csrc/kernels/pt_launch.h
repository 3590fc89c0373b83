/* pt_launch.h -- C launch interface between the host context and the kernel translation units. */
#pragma once
#include <hip/hip_runtime_api.h>
#include "pt_scene.h"
#include "pt_copies.h"

/* compute units of the CURRENT device (a process may drive several: tb_create_multi), cached per device ordinal */
static inline hipError_t pt_device_cus(int* numCUs)
{
    static int cuCache[64] = {0};
    int dev = 0; hipError_t e = hipGetDevice(&dev); if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && cuCache[dev]) { *numCUs = cuCache[dev]; return hipSuccess; }
    e = hipDeviceGetAttribute(numCUs, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess && dev >= 0 && dev < 64) cuCache[dev] = *numCUs;
    return e;
}

extern "C" {
/* the lock-step kernels: one launcher per copy (pt_copies.h PT_COPY_LIST, pt_variant.inc); mode: PtMode -- what it launches, or that it refuses
 * (hipErrorInvalidValue), is pt_pick_form's answer */
#define PT_LOCKSTEP_ARGS hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W, uint32_t H, \
    uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles, int sceneInLds, int countRays, int mode
typedef hipError_t (*pt_variant_fn)(PT_LOCKSTEP_ARGS);
#define PT_LAUNCHER(copy) hipError_t pt_launch_persistent_##copy(PT_LOCKSTEP_ARGS);
PT_COPY_LIST(PT_LAUNCHER)
hipError_t pt_launch_trace_closest(hipStream_t stream, const TbDeviceScene* ds, uint32_t n, const float* origins, const float* dirs, float* outT, int* outMat,
                                   float* outBary, uint32_t* outPrim, uint32_t* outGeom, float* outNormal, float* outUV, uint32_t* outBoxes, uint32_t* outTris);
/* TbDeviceTargets::regionOrder (1 + regions x numGroups words) from TbDeviceTargets::regionCost; keys: regions words of scratch; lateFrom: the first
 * position of the usual list from which a counted region's items move to the front (pt_kernels.hip region_order_kernel) */
hipError_t pt_launch_region_order(hipStream_t stream, const uint32_t* cost, const TbTileMap* tiles, uint32_t W, uint32_t H, uint32_t regions,
                                  uint32_t numGroups, uint32_t lateFrom, uint32_t* order, uint32_t* keys);
/* the adaptive launch's live list (pt_kernels.hip live_list_*): list = W x H words at most, *count; scratch = tb_live_list_scratch_bytes(regions) */
static inline size_t tb_live_list_scratch_bytes(uint32_t regions) { return (size_t)regions * 36u; }
/* budget: null, or the W x H frame indices of tb_set_sample_budget -- a pixel is live iff frame < budget[pixel] and, where frame > minFrames, the
 * skip test does not hold (live_list_count_budget; minFrames = 0xffffffff: the budget alone) */
hipError_t pt_launch_live_list(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, const uint32_t* budget, const TbTileMap* tiles, uint32_t W,
                               uint32_t H, uint32_t frame, uint32_t minFrames, float minConvergence, TbFloat4* aovNormals, TbFloat4* aovCustom,
                               int livePixelsMode, void* scratch, uint32_t* list, uint32_t* count);
hipError_t pt_launch_accumulate_samples(hipStream_t stream, const TbFloat4* samples, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames,
    const TbTileMap* tiles,
                                        TbFloat4* output, TbFloat4* jittered);
/* The fold of the list-driven frame-group launch (PT_MODE_LIVE_GROUPS; pt_scene.h TB_LIVE_COUNT_WORDS: tg->samples and tg->liveList set, the count in
 * the 16 bytes before the list): accumulate_samples_kernel's sums for the listed pixels only (the other pixels' samples were never written).
 * maxEntries: an upper bound of the count, the owned pixels; the count itself stays on the device. */
hipError_t pt_launch_accumulate_live(hipStream_t stream, const TbFloat4* samples, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames,
                                     const uint32_t* list, uint64_t maxEntries, TbFloat4* output, TbFloat4* jittered);
hipError_t pt_launch_device_math(hipStream_t stream, int fn, uint32_t n, const float* a, const float* b, float* out);
hipError_t pt_launch_unpack_gathered(hipStream_t stream, const TbFloat4* gathered, size_t capacity, TbFloat4* full, uint32_t W, uint32_t H, uint32_t world,
    uint32_t tileW, uint32_t tileH);
hipError_t pt_launch_pack_owned(hipStream_t stream, const TbFloat4* full, TbFloat4* packed, uint32_t W, uint32_t H, const TbTileMap* tiles,
    uint32_t numOwnedTiles);
/* GPU LBVH build (bvh_kernels.hip); every pointer is a device pointer */
size_t bvh_gpu_scratch_bytes(uint32_t N);
hipError_t bvh_gpu_build(hipStream_t stream, const float* positions, const uint32_t* triVertexIndex, const uint32_t* triGeometry, const uint32_t* triPrimitive,
                         const uint32_t* triFlags, uint32_t N, uint32_t treeletPasses, uint8_t* scratch, size_t scratchBytes, uint8_t* bvhA, TbNodeB* nodesB,
                             TbTriB* trisB,
                         uint32_t* rootHeight);
/* top level over instances on the GPU (two-level scenes); rootRef / rootHeight are device words */
size_t bvh_gpu_tlas_scratch_bytes(uint32_t M);
hipError_t bvh_gpu_build_tlas(hipStream_t stream, uint32_t M, const float* objectToWorld, const float* worldToObject, const uint32_t* blasIndex,
    const uint32_t* hitGroupBase,
                              const float* blasBoxes, uint8_t* scratch, size_t scratchBytes, uint8_t* tlasA, TbNodeB* topNodes, uint32_t* rootRef,
                                  uint32_t* rootHeight);
/* real-time chain (rt_kernels.hip): temporal accumulation, one a-trous denoiser iteration, albedo composite */
hipError_t rt_launch_temporal(hipStream_t stream, const TbTemporalConstants* k, const TbFloat4* history, const TbFloat4* current, const TbFloat4* worldPos,
                              const TbFloat4* prevWorldPos, const TbFloat4* momentHistory, const TbFloat4* normals, TbFloat4* out, TbFloat4* outMoment);
hipError_t rt_launch_denoise(hipStream_t stream, const TbDenoiserConstants* k, const TbFloat4* input, const TbFloat4* normals, const TbFloat4* positions,
                             const TbFloat4* undenoised, TbFloat4* out);
hipError_t rt_launch_composite(hipStream_t stream, uint32_t W, uint32_t H, const TbFloat4* albedo, const TbFloat4* lighting, const TbFloat4* emissive,
    TbFloat4* out);
/* output stage (post_kernels.hip): optional histogram + average (auto exposure), then PostProcessCS */
hipError_t post_launch(hipStream_t stream, const TbPostConstants* pc, const TbFloat4* in, const float* inR32, const TbFloat4* aux,
                       uint32_t* histogram, float* averaged, TbFloat4* out, uint32_t* outRgba8);
}
