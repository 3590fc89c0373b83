/* vis_launch.h -- the launchers of vis_kernels.hip: the path inspector.
 *   vis_launch_paths    the complete paths of ONE pixel traced again, one lane per frame of [firstFrame, firstFrame + numFrames): a counting pass
 *                       (frames[f] = the sample's sum, flags and number of rays), a prefix sum over the frames (where each frame's rays go in the ray
 *                       buffer, what fits under the cap, the new count) and a storing pass -- so the buffer's order is frame, then bounce, whatever
 *                       the scheduling
 *   vis_launch_overlay  the reference's VisualizeRaysCS: the stored rays drawn as cylinders with arrow heads over a float picture
 * The launchers know neither contexts nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "pt_scene.h"
#include "guide_launch.h"

#define VIS_MAX_PATH_FRAMES 4096u

extern "C" {
/* plan: made by guide_stack_plan; this fills grid (workgroups of 256 lanes, one lane per frame) and lanes (the columns of the overflow buffer) */
hipError_t vis_plan_grid(GuidePlan* plan, uint32_t numFrames);
/* tg: read for the camera constants alone.  rayBuffer: the count word, then at once TB_MAX_VISUALIZER_RAYS records (the records 16-B aligned, so the word is not); base: the rays it holds
 * (the host's count; the count word is rewritten).  frames: numFrames records.  totals: two words -- [0] the buffer's new count, [1] the rays this
 * call would have stored without the cap.  x < W, y < H, 1 <= numFrames <= VIS_MAX_PATH_FRAMES. */
hipError_t vis_launch_paths(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W, uint32_t H,
                            uint32_t x, uint32_t y, uint32_t firstFrame, uint32_t numFrames, const GuidePlan* plan, uint32_t* overflow,
                            uint32_t* rayBuffer, uint32_t base, TbPathFrame* frames, uint32_t* totals);
/* rays: numRays records (no count word; at most TB_MAX_VISUALIZER_RAYS are read, and no more than k->RayCount).  scene, out: W x H RGBA32F, W and H
 * from k.  worldPos: null = no occluder; hits: null = worldPos.xyz is the position, else the position is worldPos.xyz / hits.w where hits.w > 0 and
 * none elsewhere (the guide pass's sums).  out8: null, or the R8G8B8A8_UNORM store of out. */
hipError_t vis_launch_overlay(hipStream_t stream, const TbVisualizeConstants* k, const TbVisualizerRay* rays, uint32_t numRays, const TbFloat4* scene,
                              const TbFloat4* worldPos, const TbFloat4* hits, TbFloat4* out, uint32_t* out8);
}
