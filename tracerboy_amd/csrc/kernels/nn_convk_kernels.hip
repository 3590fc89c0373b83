/* nn_convk_kernels.hip -- the convolution of both networks, the still denoiser's U-Net (K = 3, the plain form) and the 2 x
 * super-resolution (section 16: K = 3 and 5, either form), and the latter's residual add; launchers in nn_launch.h:
 *   nn_convk_kernel      K x K convolution, K = 3 or 5, + optional bias (+ ReLU) as an implicit GEMM on v_mfma_f32_16x16x32_f16; reads up to two
 *                        source tensors in channel order, the first optionally nearest-upsampled x 2 as it is gathered (upsample and concat cost
 *                        no pass)
 *   nn_convk_staged_kernel  the same convolution, bit for bit, with the input tile of a workgroup staged in LDS once and four output rows
 *                        register-blocked against every weight fragment
 *   nn_sr_finish_kernel  the residual add: |half(conv6 + the input nearest-upsampled x 2)| -> RGBA32F
 *
 * The layer arithmetic: binary16 activations and weights, fp32 accumulation (in the matrix core's order), + bias where there is one, max(., 0)
 * where the layer has ReLU, then one rounding to binary16 (nearest even; overflow gives infinity, NaN stays NaN).  Padding is zero, (K - 1) / 2 on
 * every side.  Accumulation order: tap-major (ky, then kx), then the k-blocks of 32 channels, one accumulator per block of 16 output channels.
 * Both forms keep that order and feed the matrix core the same fragments, so their results are the same bits.
 *
 * The GEMM of one wave: D[output channel][pixel] += W[output channel][k] * X[k][pixel] over k = 32 channels of one tap, for 16 consecutive x of one
 * output row and NB x 16 output channels.  Lane l holds, as the instruction wants them (cdna_hip_programming section 3: the f16 form uses the bf16 map),
 *   A (weights)      output channel l & 15, k = 8 (l >> 4) + j, j = 0..7: one 16-byte load of the host's repack (nn_weights.h packLayer)
 *   B (activations)  k = 8 (l >> 4) + j at pixel l & 15: eight consecutive channels of one pixel, one 16-byte load of an NHWC tensor whose
 *                    channel count is a multiple of 32 (nn_gather)
 *   D                pixel l & 15, output channels 4 (l >> 4) + r, r = 0..3: one 8-byte store (nn_store).
 * A k-block lies in source A or in source B, never across (both are padded to 32 channels, and the repack puts zero weights on the padding).
 * Every activation load is predicated on its tap lying inside the picture; a lane whose pixel is past the row end loads whatever taps are inside and
 * stores nothing; no lane reads or writes outside a tensor's padded extent. */
#include "nn_launch.h"

#define NNK_THREADS 256u
#define NNK_WAVES (NNK_THREADS / 64u)

namespace {

typedef _Float16 nn_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 nn_half4 __attribute__((ext_vector_type(4)));
typedef float nn_float4 __attribute__((ext_vector_type(4)));

struct NnConvK {
    const uint16_t* inA; const uint16_t* inB; const uint16_t* weight; const float* bias /* null: none */; uint16_t* out;
    uint32_t width, height, padA, padB /* padded channels of the sources; padB 0 = no source B */, upsampleA, cOut, outPadded, relu;
    uint32_t tilesX, units /* tilesX * height * (outPadded / (16 NB)) */;
};

/* eight channels of k-block kb (those of `quarter`) at pixel (sx, sy) of the layer's input: source A's k-blocks, read at (sy >> 1, sx >> 1)
 * with upsampleA, then source B's; zeros outside the picture -- the padding, and all a lane past the row end may ask for out of bounds */
__device__ __forceinline__ nn_half8 nn_gather(const NnConvK& p, int32_t sx, int32_t sy, uint32_t kb, uint32_t quarter)
{
    nn_half8 act = {0, 0, 0, 0, 0, 0, 0, 0};
    if (sx >= 0 && sy >= 0 && sx < (int32_t)p.width && sy < (int32_t)p.height) {
        const uint32_t kBlocksA = p.padA / 32u, widthA = p.upsampleA ? p.width / 2u : p.width;
        const size_t pixelA = p.upsampleA ? (size_t)((uint32_t)sy >> 1) * widthA + ((uint32_t)sx >> 1) : (size_t)(uint32_t)sy * p.width + (uint32_t)sx;
        const size_t pixelB = (size_t)(uint32_t)sy * p.width + (uint32_t)sx;
        const uint16_t* src = kb < kBlocksA ? p.inA + pixelA * p.padA + kb * 32u : p.inB + pixelB * p.padB + (kb - kBlocksA) * 32u;
        act = *(const nn_half8*)(src + quarter * 8u);
    }
    return act;
}

/* a lane's four sums of output block `block` (16 channels; the lane's are c0 ...) to pixel (x, y): + bias where there is one, ReLU where the layer
 * has it, one rounding */
__device__ __forceinline__ void nn_store(const NnConvK& p, uint32_t x, uint32_t y, uint32_t block, uint32_t quarter, nn_float4 acc)
{
    const uint32_t c0 = block * 16u + quarter * 4u;
    nn_float4 bias = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.bias) bias = *(const nn_float4*)(p.bias + c0);
    nn_half4 h;
    for (int r = 0; r < 4; r++) {
        float v = acc[r];
        if (p.bias) v = v + bias[r];
        if (p.relu) v = v < 0.0f ? 0.0f : v;      /* a NaN stays */
        h[r] = c0 + (uint32_t)r < p.cOut ? (_Float16)v : (_Float16)0.0f; /* the padded channels hold zeros whatever the sums were */
    }
    *(nn_half4*)(p.out + ((size_t)y * p.width + x) * p.outPadded + c0) = h;
}

template <int NB, int K> __global__ __launch_bounds__(NNK_THREADS) void nn_convk_kernel(const NnConvK p)
{
    const uint32_t lane = threadIdx.x & 63u, unit = blockIdx.x * NNK_WAVES + (threadIdx.x >> 6); /* a wave's unit: one tile of one row, one group of output channels */
    if (unit >= p.units) return; /* the whole wave */
    const uint32_t tile = unit % p.tilesX, rest = unit / p.tilesX, y = rest % p.height, group = rest / p.height;
    const uint32_t px = lane & 15u, quarter = lane >> 4, x = tile * 16u + px;
    const uint32_t kBlocks = (p.padA + p.padB) / 32u, outBlocks = p.outPadded / 16u;
    nn_float4 acc[NB];
    for (int b = 0; b < NB; b++) acc[b] = nn_float4{0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t tap = 0; tap < (uint32_t)(K * K); tap++) {
        /* of the tap, not of the lane's pixel: a lane past the row end may still load (in bounds) */
        const int32_t sx = (int32_t)x + (int32_t)(tap % (uint32_t)K) - (K - 1) / 2, sy = (int32_t)y + (int32_t)(tap / (uint32_t)K) - (K - 1) / 2;
        for (uint32_t kb = 0; kb < kBlocks; kb++) {
            const nn_half8 act = nn_gather(p, sx, sy, kb, quarter);
            const nn_half8* w = (const nn_half8*)p.weight + ((size_t)(tap * kBlocks + kb) * outBlocks + group * (uint32_t)NB) * 64u + lane;
            for (int b = 0; b < NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[b * 64], act, acc[b], 0, 0, 0);
        }
    }
    if (x >= p.width) return;
    for (int b = 0; b < NB; b++) nn_store(p, x, y, group * (uint32_t)NB + (uint32_t)b, quarter, acc[b]);
}

/* The staged form.  A workgroup of four waves computes a tile of NNS_TX x NNS_TY output pixels for one group of NB x 16 output channels; wave w
 * takes the 16 columns (w & 1) and the 4 rows (w >> 1) of it.  The input tile plus its halo, (NNS_TX + K - 1) x (NNS_TY + K - 1) pixels of all
 * k-blocks, is staged in LDS once: source selection, the upsample gather and the zero padding happen there, so the inner loop is
 *   per tap and k-block: NB weight fragments from memory (as the plain form), 4 activation fragments by ds_read_b128, 4 NB MFMAs
 * against the plain form's NB + 1 loads for NB MFMAs.
 * The LDS image is [k-block][k-quarter][pixel][8 halves] with the quarter planes a multiple of 256 B apart: the 16 lanes of a ds_read_b128 lane
 * group are pixels 0-3 and 12-15 of one quarter and 4-11 of the next, 16 consecutive 16-B slots modulo a bank row, so no two share a bank
 * (MI355X_MICROARCH.md, LDS).  At most two k-blocks (nn_convk_staged_fits): 8 planes of 6 912 B for K = 5, 54 KiB, two workgroups per CU. */
#define NNS_TX 32u
#define NNS_TY 8u
#define NNS_ROWS 4u

template <int K> struct NnStagedTile {
    static constexpr uint32_t width = NNS_TX + (uint32_t)K - 1u, height = NNS_TY + (uint32_t)K - 1u, pixels = width * height;
    static constexpr uint32_t planeBytes = (pixels * 16u + 255u) / 256u * 256u;
};

template <int NB, int K> __global__ __launch_bounds__(NNK_THREADS) void nn_convk_staged_kernel(const NnConvK p)
{
    typedef NnStagedTile<K> T;
    extern __shared__ __attribute__((aligned(256))) uint8_t nns_image[];
    const uint32_t tilesY = (p.height + NNS_TY - 1u) / NNS_TY;
    const uint32_t tileX = blockIdx.x % p.tilesX, rest = blockIdx.x / p.tilesX, tileY = rest % tilesY, group = rest / tilesY;
    const int32_t originX = (int32_t)(tileX * NNS_TX) - (K - 1) / 2, originY = (int32_t)(tileY * NNS_TY) - (K - 1) / 2; /* of the staged tile, in the picture */
    const uint32_t kBlocks = (p.padA + p.padB) / 32u, outBlocks = p.outPadded / 16u;
    /* consecutive lanes: the four quarters of a pixel's k-block, then the next pixel -- 64 contiguous bytes of memory per pixel */
    for (uint32_t item = threadIdx.x; item < T::pixels * 4u * kBlocks; item += NNK_THREADS) {
        const uint32_t quarter = item & 3u, pixel = (item >> 2) % T::pixels, kb = (item >> 2) / T::pixels;
        const nn_half8 act = nn_gather(p, originX + (int32_t)(pixel % T::width), originY + (int32_t)(pixel / T::width), kb, quarter);
        *(nn_half8*)(nns_image + (kb * 4u + quarter) * T::planeBytes + pixel * 16u) = act;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, px = lane & 15u, quarter = lane >> 4;
    const uint32_t waveX = (wave & 1u) * 16u, waveY = (wave >> 1) * NNS_ROWS; /* in the tile */
    const uint32_t x = tileX * NNS_TX + waveX + px, y0 = tileY * NNS_TY + waveY;
    if (tileX * NNS_TX + waveX >= p.width || y0 >= p.height) return; /* the whole wave: nothing of its block lies in the picture */
    nn_float4 acc[NNS_ROWS][NB];
    for (uint32_t r = 0; r < NNS_ROWS; r++) for (int b = 0; b < NB; b++) acc[r][b] = nn_float4{0.0f, 0.0f, 0.0f, 0.0f};
    const uint8_t* const mine = nns_image + quarter * T::planeBytes + (waveY * T::width + waveX + px) * 16u;
    for (uint32_t tap = 0; tap < (uint32_t)(K * K); tap++) {
        const uint32_t tapPixel = (tap / (uint32_t)K) * T::width + tap % (uint32_t)K;
        for (uint32_t kb = 0; kb < kBlocks; kb++) {
            const nn_half8* w = (const nn_half8*)p.weight + ((size_t)(tap * kBlocks + kb) * outBlocks + group * (uint32_t)NB) * 64u + lane;
            nn_half8 wf[NB];
            for (int b = 0; b < NB; b++) wf[b] = w[b * 64];
            const uint8_t* const a = mine + kb * 4u * T::planeBytes + tapPixel * 16u;
            for (uint32_t r = 0; r < NNS_ROWS; r++) {
                const nn_half8 act = *(const nn_half8*)(a + r * T::width * 16u);
                for (int b = 0; b < NB; b++) acc[r][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[b], act, acc[r][b], 0, 0, 0);
            }
        }
    }
    if (x >= p.width) return;
    for (uint32_t r = 0; r < NNS_ROWS && y0 + r < p.height; r++)
        for (int b = 0; b < NB; b++) nn_store(p, x, y0 + r, group * (uint32_t)NB + (uint32_t)b, quarter, acc[r][b]);
}

/* a lane per output pixel: channels 0-2 of both tensors.  The sum of two binary16 values in fp32 and its rounding to binary16 is their exact sum
 * rounded once: fp32's 24 bits are 2 x 11 + 2, which makes the double rounding innocuous, and no such sum is an fp32 denormal */
__global__ __launch_bounds__(NNK_THREADS) void nn_sr_finish_kernel(const uint16_t* __restrict__ residual, const uint16_t* __restrict__ input,
    TbFloat4* __restrict__ out, uint32_t inW, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * NNK_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const uint32_t outW = inW * 2u, x = i % outW, y = i / outW;
    const nn_half4 a = *(const nn_half4*)(residual + (size_t)i * 32u);
    const nn_half4 b = *(const nn_half4*)(input + ((size_t)(y >> 1) * inW + (x >> 1)) * 32u);
    float v[3];
    for (int c = 0; c < 3; c++) {
        const _Float16 h = (_Float16)((float)a[c] + (float)b[c]);
        v[c] = __builtin_fabsf((float)h); /* clears the sign bit: a NaN stays a NaN */
    }
    out[i] = TbFloat4{v[0], v[1], v[2], 1.0f};
}

template <int K> void nnk_launch(bool four, dim3 grid, hipStream_t stream, const NnConvK& p)
{
    if (four) hipLaunchKernelGGL((nn_convk_kernel<4, K>), grid, dim3(NNK_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((nn_convk_kernel<2, K>), grid, dim3(NNK_THREADS), 0, stream, p);
}

template <int K> void nnk_launch_staged(bool four, hipStream_t stream, const NnConvK& p)
{
    const uint32_t tilesY = (p.height + NNS_TY - 1u) / NNS_TY, groups = p.outPadded / (four ? 64u : 32u);
    const dim3 grid(p.tilesX * tilesY * groups); /* <= 2^24 / 256 tiles (and their remainders) x 16 groups */
    const uint32_t lds = (p.padA + p.padB) / 32u * 4u * NnStagedTile<K>::planeBytes; /* <= 55 296 */
    if (four) hipLaunchKernelGGL((nn_convk_staged_kernel<4, K>), grid, dim3(NNK_THREADS), lds, stream, p);
    else hipLaunchKernelGGL((nn_convk_staged_kernel<2, K>), grid, dim3(NNK_THREADS), lds, stream, p);
}

} // namespace

extern "C" hipError_t nn_launch_convk(hipStream_t stream, uint32_t width, uint32_t height, uint32_t kernel, uint32_t form, const uint16_t* inA, uint32_t cA,
    uint32_t upsampleA, const uint16_t* inB, uint32_t cB, const uint16_t* weight, const float* bias, uint32_t cOut, uint32_t relu, uint16_t* out)
{
    if (!nn_frame(width, height) || !nn_tensor(inA) || !nn_tensor(weight) || !nn_tensor(out) || !nn_channels(cA) || !nn_channels(cOut))
        return hipErrorInvalidValue;
    if ((kernel != 3u && kernel != 5u) || form > 1u || (bias && !nn_tensor(bias))) return hipErrorInvalidValue;
    if (form == 1u && !nn_convk_staged_fits(cA, cB)) return hipErrorInvalidValue;
    if ((cB != 0u) != (inB != nullptr) || (cB && (!nn_tensor(inB) || !nn_channels(cB)))) return hipErrorInvalidValue;
    if (upsampleA && ((width | height) & 1u)) return hipErrorInvalidValue;
    if (out == inA || out == inB) return hipErrorInvalidValue;
    NnConvK p;
    p.inA = inA; p.inB = inB; p.weight = weight; p.bias = bias; p.out = out;
    p.width = width; p.height = height; p.padA = nn_padded_channels(cA); p.padB = cB ? nn_padded_channels(cB) : 0u; p.upsampleA = upsampleA ? 1u : 0u;
    p.cOut = cOut; p.outPadded = nn_padded_channels(cOut); p.relu = relu ? 1u : 0u;
    const bool four = p.outPadded % 64u == 0u; /* 64 output channels per wave where they divide, else 32: an activation fragment feeds that many MFMAs */
    if (form == 1u) {
        p.tilesX = (width + NNS_TX - 1u) / NNS_TX; p.units = 0u;
        if (kernel == 3u) nnk_launch_staged<3>(four, stream, p); else nnk_launch_staged<5>(four, stream, p);
        return hipGetLastError();
    }
    p.tilesX = (width + 15u) / 16u;
    const uint64_t units = (uint64_t)p.tilesX * height * (p.outPadded / (four ? 64u : 32u)); /* < 2^24 * 16 */
    p.units = (uint32_t)units;
    const dim3 grid((uint32_t)((units + NNK_WAVES - 1u) / NNK_WAVES));
    if (kernel == 3u) nnk_launch<3>(four, grid, stream, p); else nnk_launch<5>(four, grid, stream, p);
    return hipGetLastError();
}

extern "C" hipError_t nn_launch_sr_finish(hipStream_t stream, uint32_t inW, uint32_t inH, const uint16_t* residual, const uint16_t* input, TbFloat4* out)
{
    if (!inW || !inH || (uint64_t)inW * inH * 4u > (1ull << 24) || !nn_tensor(residual) || !nn_tensor(input) || !nn_tensor(out)) return hipErrorInvalidValue;
    const uint32_t nPixels = inW * inH * 4u;
    hipLaunchKernelGGL(nn_sr_finish_kernel, dim3((nPixels + NNK_THREADS - 1u) / NNK_THREADS), dim3(NNK_THREADS), 0, stream, residual, input, out, inW, nPixels);
    return hipGetLastError();
}
