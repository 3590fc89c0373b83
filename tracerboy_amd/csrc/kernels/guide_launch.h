/* guide_launch.h -- the launchers of guide_kernels.hip: the guide pass of a still's denoise.  First hits of the frames
 * [firstFrame, firstFrame + numFrames) traced again by a kernel of its own and summed per pixel, in frame order, into three RGBA32F surfaces:
 *   albedo    (sum of the effective albedo e_f, number of frames)            e_f = the frame's albedo AOV, or (1, 1, 1) where that is all zero
 *   normal    (sum of the normal AOV over the frames that hit, their number)  a frame hits where its normal AOV is not all zero
 *   position  (sum of the world position over the frames that hit, sum of the distance to the neighbour's hit over them)
 * Every sum is fp32 acc = acc + v from 0.  The launcher knows neither contexts nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "pt_scene.h"

/* How a launch holds its traversal stacks, decided like the launch plan decides it for a copy held to four workgroups per CU (launch_plan.h): the
 * whole stack in LDS where a quarter of 160 KB has room for it (1 KB per entry + 128 B), else that many entries in LDS and the deepest ones
 * -- at most overflowMax -- in global memory (the HYBRID form), else the whole stack in LDS again at a lower residency; ok = 0: deeper than LDS.
 * forcedCap > 0 (option stack_lds_cap, a test hook as in the launch plan): no more entries than that in LDS although the stack would fit. */
struct GuidePlan { uint32_t ok, ldsEntries, overflowEntries, grid, lanes; };
static inline GuidePlan guide_stack_plan(uint32_t stackDepth, uint32_t overflowMax, uint32_t forcedCap)
{
    GuidePlan p{1u, stackDepth ? stackDepth : 1u, 0u, 0u, 0u};
    const uint32_t share = (160u * 1024u / 4u) / 512u * 512u, room = (share - 512u) / 1024u, cap = forcedCap > 0u && forcedCap < room ? forcedCap : room;
    if (p.ldsEntries <= cap) return p;
    if (p.ldsEntries - cap <= overflowMax) { p.overflowEntries = p.ldsEntries - cap; p.ldsEntries = cap; return p; }
    if ((uint64_t)p.ldsEntries * 1024u + 512u > 160u * 1024u) p.ok = 0u;
    return p;
}

extern "C" {
/* fills grid (workgroups: min(regions, 2 x residency), the grid strides over the 16 x 16 regions) and lanes (grid x 256: the columns of the overflow
 * buffer, overflowEntries x lanes words) of a plan made by guide_stack_plan */
hipError_t guide_plan_grid(GuidePlan* plan, uint32_t regions);
/* tg: read for the camera constants alone (TbDeviceTargets::camPre); overflow: null unless plan->overflowEntries.  Surfaces 16-B aligned, W x H. */
hipError_t guide_launch(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W, uint32_t H,
                        uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles, const GuidePlan* plan, uint32_t* overflow,
                        TbFloat4* albedo, TbFloat4* normal, TbFloat4* position);
}
