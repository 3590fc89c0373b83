/* sr_weights.h -- the weights of the 2 x super-resolution network as sr_weights.cpp reads them from the reference's
 * weights.bin container and folds them.  No HIP header: the reader is tested without a device. */
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "nn_weights.h"

namespace tbsr {

const uint32_t kLayers = 7;
extern const char* const kLayerNames[kLayers]; /* in the order the network runs them */
extern const uint32_t kKernel[kLayers];        /* 5, 3, 3, 5, 3, 3, 3: the graph's, the file holds no shapes */
const uint32_t kMaxFileChannels = 256;

/* folded binary16 bits; weight is o x i x K x K as in the file; bias is empty for the last layer, which has neither bias nor ReLU */
struct Layer { uint32_t in = 0, out = 0, kernel = 0; std::vector<uint16_t> weight, bias; };
struct Weights { Layer layer[kLayers]; uint64_t weightBytes() const; };

/* throw tbnn::Error (TB_E_IO / TB_E_PARSE) */
Weights parse(const uint8_t* data, size_t size);
Weights read(const char* path);

/* binary32 -> binary16 as the reference converts its weights (DirectMLSuperResolution.cpp:47-63, Float16Compressor::compress), bit for bit: the
 * mantissa is truncated, not rounded; everything above 65504 becomes infinity; a NaN stays a NaN */
uint16_t compress(float value);

} // namespace tbsr
