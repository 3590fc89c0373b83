/* dn_launch.h -- the launchers of dn_kernels.hip: the passes a still's denoise adds around the a-trous filter of rt_kernels.hip
 * (DESIGN.md section 12).  Each streams RGBA32F surfaces of nPixels = W x H pixels once; none knows about frames, options or contexts.
 * Every surface 16-B aligned; a launcher refuses (hipErrorInvalidValue) a null or misaligned surface and a zero-sized frame. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tb_abi.h"

extern "C" {
/* prepared[i] = (mean colour of output[i], variance of the luminance of that mean estimated from the two halves output / jittered hold) */
hipError_t dn_launch_prepare(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, TbFloat4* prepared, uint32_t W, uint32_t H);
/* filtered[i] = (prepared[i].xyz, 3x3 Gaussian of prepared.w, coordinates clamped to the frame) */
hipError_t dn_launch_prefilter(hipStream_t stream, const TbFloat4* prepared, TbFloat4* filtered, uint32_t W, uint32_t H);
/* final[i] = (in[i].xyz, 1) */
hipError_t dn_launch_finish(hipStream_t stream, const TbFloat4* in, TbFloat4* final, uint32_t W, uint32_t H);
/* The chain on the guide pass's sums (guide_launch.h).  gNormal = (sum of normals, frames that hit), gPosition = (sum of
 * positions, sum of neighbour distances), gAlbedo = (sum of the effective albedo, frames).
 * normals[i] = hits > 0 ? (gNormal.xyz / hits, 1) : (0, 0, 0, 1), with hits > 1 brought back to length 1 (zero where the sum cancels);
 * positions[i] = hits > 0 ? gPosition / hits : 0 */
hipError_t dn_launch_resolve_guides(hipStream_t stream, const TbFloat4* gNormal, const TbFloat4* gPosition, TbFloat4* normals, TbFloat4* positions,
                                    uint32_t W, uint32_t H);
/* dn_launch_prepare with d = max(gAlbedo.xyz / gAlbedo.w, 0.01) per channel: the mean colour and both halves' means are divided by d */
hipError_t dn_launch_prepare_demod(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, const TbFloat4* gAlbedo, TbFloat4* prepared,
                                   uint32_t W, uint32_t H);
/* final[i] = (in[i].xyz * d, 1) */
hipError_t dn_launch_finish_remod(hipStream_t stream, const TbFloat4* in, const TbFloat4* gAlbedo, TbFloat4* final, uint32_t W, uint32_t H);
/* The noise target of a sample budget.  filtered: dn_launch_prepare + dn_launch_prefilter of output / jittered; budget: W x H
 * frame indices.  A pixel with budget > frame gets budget = frame iff frame >= minFrames, it holds samples and its mean is black or filtered.w <
 * relError^2 (luma(mean)^2 + 0.01).  counts[0] += pixels stopped, counts[1] += pixels still live (budget > frame) afterwards: zero them first. */
hipError_t dn_launch_budget_stop(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, const TbFloat4* filtered, uint32_t* budget,
                                 uint32_t W, uint32_t H, uint32_t frame, uint32_t minFrames, float relError, unsigned long long* counts);
}
