/* rad_launch.h -- the launchers of rad_kernels.hip: radiance queries (include/tracerboy_hip.h tb_trace_radiance /
 * tb_make_camera_rays).
 *   rad_plan_grid            fills a plan's grid for n rays: the kernel of that feature set and form, its LDS, the device's residency
 *   rad_launch               the paths of a call's samples, per ray summed in sample order; splits the call into launches of at most maxPaths paths
 *                            over sample ranges of the same rays (the later launches accumulate: by the contract of the sum no bit changes)
 *   rad_launch_camera_rays   path_begin of every pixel of a window, as ray records
 * Every pointer is a device pointer, rays and out 16-B aligned.  n <= 2^31.  The launchers know neither contexts nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "pt_scene.h"
#include "pt_copies.h"
#include "guide_launch.h"
#include "rq_launch.h"

/* The refilling form is section 20's (rq_launch.h), for the reason found there: idle lanes draw consecutive indices from a per-wave pool of
 * RAD_CHUNK rays that lane 0 claims with ONE atomic add -- one add per refill saturated the counter's one address.  A pool of a radiance query is
 * smaller than RQ_CHUNK = 256: a ray is num_samples whole paths, hundreds to thousands of walk steps, so a wave claims far less often than the
 * any-hit walk does, and a large pool leaves the last waves of a launch with more work than their neighbours -- measured (DESIGN.md section 22,
 * scripts/radiance_rate.py): pools of 64 beat pools of 128 by 2 to 28 % and pools of 256 by 6 to 64 % on every ray set of both scenes.
 * RAD_REFILL_MIN: idle lanes at which a wave draws new rays.  Both are defaults of the plan; the script varies them through the environment
 * (TB_RAD_CHUNK, TB_RAD_REFILL). */
#define RAD_CHUNK 64u
#define RAD_REFILL_MIN 16u
/* Paths of one launch.  A launch's duration must not grow with n x num_samples without bound: a query of 2^31 rays x 2^24 samples is legal.  2^26
 * paths are 32 full-HD frames' worth; a call below it is one launch, and what the split costs a larger one -- a launch and one read and write of
 * out per 2^26 paths -- is nothing beside the paths.  Where n alone exceeds it a launch is one sample of every ray. */
#define RAD_MAX_PATHS (1u << 26)
/* A sample's seed is hash13(SeedX, SeedY, s) moved by seed_advance the way rand() moves it: floor(seed_advance) additions of 1, each rounded, then
 * one addition of the rest -- so that an advance of 16 lands where path_begin's sixteen draws land, bit for bit, and an advance of A + 2 where two
 * draws after an advance of A do.  At most this many steps; a larger advance adds what is left in one addition (as does a negative one, all of it). */
#define RAD_SEED_STEPS 1024u

/* which kernel and how: features, a feature set that rad_kernels.hip instantiates (kRadFeatureSets); form 0 one ray per lane -- a wave
 * takes 64 consecutive rays and the next 64 when all are done --, 1 the refilling persistent grid */
struct RadPlan { GuidePlan stack; uint32_t features, form, refillMin, chunk, maxPaths; };
struct RadCall { uint32_t firstSample, numSamples, hemisphere, accumulate; float seedAdvance; };

/* the feature sets the kernel is compiled for, smallest first (the order the picker searches) */
/* (those of pt_copies.h: matte, env, surf, sss, vol, full) */
static const uint32_t kRadFeatureSets[] = {0u, PT_FEAT_ENV, PT_FEATS_SURF, PT_FEATS_SSS, PT_FEATS_VOL, PT_FEAT_ALL};

extern "C" {
/* gridOverride: 0, or the workgroups of the persistent grid (a diagnostic) */
hipError_t rad_plan_grid(RadPlan* plan, uint64_t n, uint32_t gridOverride);
/* overflow: null unless plan->stack.overflowEntries (then overflowEntries x plan->stack.lanes words); counter: one word, zeroed here on the stream
 * before every launch of the refilling form; launches: how many launches the call became (may be null) */
hipError_t rad_launch(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const RadCall* call, const RadPlan* plan, uint32_t* overflow,
                      uint32_t* counter, uint64_t n, const TbRadianceRay* rays, TbFloat4* out, uint32_t* launches);
/* advance: one float, how far path_begin moved the seed of the window's first pixel */
hipError_t rad_launch_camera_rays(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W, uint32_t H,
                                  uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t frame, TbRadianceRay* out, float* advance);
}
