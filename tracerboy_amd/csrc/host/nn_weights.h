/* nn_weights.h -- the weights of the still denoiser's U-Net as nn_weights.cpp reads them from a TZA container, and the
 * repack of one layer for nn_convk (nn_convk_kernels.hip).  No HIP header: the reader is tested without a device. */
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace tbnn {

const uint32_t kLayers = 16;
extern const char* const kLayerNames[kLayers]; /* in the order the network runs them */
const uint32_t kMaxFileChannels = 256; /* per layer of a file; the layer seam (tb_run_conv3x3) takes up to 512 per tensor */

/* binary16 bits throughout; weight is o x i x 3 x 3 as in the file */
struct Layer { uint32_t in = 0, out = 0; std::vector<uint16_t> weight, bias; };
struct Weights { Layer layer[kLayers]; uint64_t weightBytes() const; };

/* a failure: code is TB_E_IO or TB_E_PARSE */
struct Error { int code; std::string message; };

/* throws Error */
Weights parseTza(const uint8_t* data, size_t size);
Weights readTza(const char* path);

uint16_t halfFromFloat(float f);   /* round to nearest even, overflow to infinity, NaN stays NaN */
float floatFromHalf(uint16_t h);

inline uint32_t roundUp(uint32_t v, uint32_t to) { return (v + to - 1u) / to * to; }

/* One layer as nn_convk (nn_convk_kernels.hip) reads it.  The kernel's K axis is source A's channels padded to a multiple of 32, then
 * source B's padded likewise; its output channels are padded to a multiple of 32.  taps: 9 for a 3 x 3 filter, 25 for a 5 x 5 one.
 * weight: [tap = ky * 3 + kx (ky * 5 + kx)][K / 32][padded out / 16][lane 0..63][8] binary16, where lane l's
 * eight values are output channel 16 * block + (l & 15) at k = 32 * kblock + 8 * (l >> 4) + j -- the A fragment of
 * v_mfma_f32_16x16x32_f16 as one 16-byte load; zero wherever a padded channel is involved.  bias: fp32, zero past the count (all zero for a null
 * bias). */
struct PackedLayer { uint32_t cA = 0, cB = 0, cOut = 0, kBlocks = 0, outPadded = 0; std::vector<uint16_t> weight; std::vector<float> bias; };
PackedLayer packLayer(uint32_t cA, uint32_t cB, uint32_t cOut, const uint16_t* weightOihw, const uint16_t* bias, uint32_t taps = 9u);

} // namespace tbnn
