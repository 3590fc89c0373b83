/* nn_launch.h -- the launchers of nn_kernels.hip: the layers of the still denoiser's U-Net.  None knows about contexts,
 * weight files or the network's graph.
 * An activation tensor is NHWC binary16 with its channel count padded to a multiple of 32 (nn_padded_channels); the padded channels hold zeros --
 * every kernel here writes them so.  Tensors are 16-byte aligned.  A launcher refuses (hipErrorInvalidValue) a null or misaligned pointer, a zero
 * dimension, more than 2^24 pixels, more than 512 channels in a tensor, and an odd size where a size is halved. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tb_abi.h"

static inline uint32_t nn_padded_channels(uint32_t c) { return (c + 31u) / 32u * 32u; }

extern "C" {
/* out[y][x][o] = half(relu?(bias[o] + sum over the 3 x 3 taps and the input channels of in * weight)), fp32 accumulation, zero padding, for a
 * width x height output.  The input is source A's channels followed by source B's (inB null and cB 0: A alone); both are width x height, except
 * that with upsampleA source A is (width / 2) x (height / 2) and read nearest-upsampled x 2.  weight and bias: tbnn::packLayer's
 * (nn_weights.h) for (cA, cB, cOut).  out has nn_padded_channels(cOut) channels and may alias neither input. */
hipError_t nn_launch_conv3x3(hipStream_t stream, uint32_t width, uint32_t height, const uint16_t* inA, uint32_t cA, uint32_t upsampleA, const uint16_t* inB,
                             uint32_t cB, const uint16_t* weight, const float* bias, uint32_t cOut, uint32_t relu, uint16_t* out);
/* out[y][x][c] = the largest of in[2y .. 2y + 1][2x .. 2x + 1][c] (a NaN among them gives NaN); in is width x height, both even, `channels`
 * counts the padded channels */
hipError_t nn_launch_maxpool2x2(hipStream_t stream, uint32_t width, uint32_t height, uint32_t channels, const uint16_t* in, uint16_t* out);
/* The network's input: paddedW x paddedH x 32 channels.  Channels 0-2 are color.xyz, with albedo and normal (both or neither) 3-5 albedo.xyz and
 * 6-8 normal.xyz, rounded to binary16 (nearest even); everything else, and every pixel outside width x height, is zero.  The surfaces are
 * width x height RGBA32F, row 0 = top.  unormColor: each colour channel first goes through the output stage's R8G8B8A8_UNORM store and back --
 * k = (uint32)(saturate(x) * 255 + 0.5) with NaN -> 0, then (float)k / 255 in fp32 -- which is what the reference's network loads from its
 * 8-bit post-process surface; albedo and normal are never clamped. */
hipError_t nn_launch_pack_input(hipStream_t stream, uint32_t width, uint32_t height, uint32_t paddedW, uint32_t paddedH, const TbFloat4* color,
                                const TbFloat4* albedo, const TbFloat4* normal, uint32_t unormColor, uint16_t* out);
/* (r, g, b, 1) of channels 0-2 of a paddedW x paddedH x 32-channel tensor, cropped to width x height */
hipError_t nn_launch_unpack_output(hipStream_t stream, uint32_t width, uint32_t height, uint32_t paddedW, const uint16_t* in, TbFloat4* out);
/* the guide sums (tb_render_guides) as the network reads them: albedo = sum.xyz / sum.w; normals as dn_launch_resolve_guides gives them
 * (sum / frames that hit, the mean of several brought to length 1, zero where nothing was hit) */
hipError_t nn_launch_resolve_aux(hipStream_t stream, uint32_t width, uint32_t height, const TbFloat4* gAlbedo, const TbFloat4* gNormal, TbFloat4* albedo,
                                 TbFloat4* normal);
/* (x, y, z, w) -> R8G8B8A8_UNORM as the output stage stores it: clamp, scale, + 0.5, truncate; alpha 255 */
hipError_t nn_launch_to_rgba8(hipStream_t stream, uint32_t width, uint32_t height, const TbFloat4* in, uint32_t* out);
}
