/* nn_launch.h -- the launchers of the two neural networks' kernels.  None knows about contexts, weight files or a network's graph.
 *   nn_convk_kernels.hip  the convolution of both, the still denoiser's U-Net and the 2 x super-resolution (section 16),
 *                         and the latter's residual add
 *   nn_kernels.hip        the U-Net's max-pool and the element-wise helpers: pack and 8-bit store (both networks), unpack and the guide
 *                         resolve (the U-Net)
 * An activation tensor is NHWC binary16 with its channel count padded to a multiple of 32 (nn_padded_channels); the padded channels hold zeros --
 * every kernel here writes them so.  Tensors are 16-byte aligned.  A launcher refuses (hipErrorInvalidValue) a null or misaligned pointer, a zero
 * dimension, more than 2^24 pixels, more than 512 channels in a tensor, and an odd size where a size is halved. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tb_abi.h"

static inline uint32_t nn_padded_channels(uint32_t c) { return (c + 31u) / 32u * 32u; }
/* what every launcher checks of a picture's size, a tensor's pointer and a tensor's channel count */
static inline bool nn_frame(uint32_t W, uint32_t H) { return W && H && (uint64_t)W * H <= (1ull << 24); }
static inline bool nn_tensor(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }
static inline bool nn_channels(uint32_t c) { return c >= 1u && c <= 512u; }

extern "C" {
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

/* nn_convk_kernels.hip.
 * out[y][x][o] = half(relu?(bias[o] + sum over the kernel x kernel taps and the input channels of in * weight)), fp32 accumulation, for a
 * width x height output; kernel 3 or 5, zero padding (kernel - 1) / 2 on every side, bias null: none.  The input is source A's channels followed
 * by source B's (inB null and cB 0: A alone); both are width x height, except that with upsampleA source A is (width / 2) x (height / 2) and read
 * nearest-upsampled x 2.  weight and bias: tbnn::packLayer's (nn_weights.h) for (cA, cB, cOut, kernel * kernel taps).  out has
 * nn_padded_channels(cOut) channels and may alias neither input.  form: 0, the plain form -- a wave per 16 pixels of a row, every fragment from
 * memory; 1, the staged form -- a workgroup per 32 x 8 pixels, its input tile and halo in LDS, four rows per weight fragment; the same bits either
 * way.  The staged form holds at most two k-blocks (nn_convk_staged_fits); more are refused like every other bad argument (hipErrorInvalidValue). */
static inline bool nn_convk_staged_fits(uint32_t cA, uint32_t cB) { return nn_padded_channels(cA) + (cB ? nn_padded_channels(cB) : 0u) <= 64u; }
hipError_t nn_launch_convk(hipStream_t stream, uint32_t width, uint32_t height, uint32_t kernel, uint32_t form, const uint16_t* inA, uint32_t cA,
                           uint32_t upsampleA, const uint16_t* inB, uint32_t cB, const uint16_t* weight, const float* bias, uint32_t cOut, uint32_t relu,
                           uint16_t* out);
/* out[y][x] = (|half(residual[y][x][c] + input[y >> 1][x >> 1][c])| for c = 0, 1, 2; 1) at (2 inW) x (2 inH): the exact sum of the two binary16
 * values rounded once, then its sign cleared (a NaN stays a NaN).  Both tensors have 32 channels; at most 2^24 output pixels. */
hipError_t nn_launch_sr_finish(hipStream_t stream, uint32_t inW, uint32_t inH, const uint16_t* residual, const uint16_t* input, TbFloat4* out);
}
