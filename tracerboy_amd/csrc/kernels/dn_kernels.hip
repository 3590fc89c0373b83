/* dn_kernels.hip -- what a still's denoise adds around the a-trous filter of rt_kernels.hip (include/tracerboy_hip.h
 * tb_denoise).  A progressive render has no luminance moments; it has two independent halves of every pixel's samples: the jittered surface
 * holds the samples whose coin fell below 0.5, the output surface holds all of them (RayGenCommon.h:721-727).
 *
 *   dn_prepare_kernel     mean colour, and the variance of its luminance from the difference of the two halves' means
 *   dn_prefilter_kernel   3x3 Gaussian over that variance (a one-sample chi-square estimate per pixel), coordinates clamped to the frame
 *   dn_finish_kernel      (rgb, 1): a surface the output stage's division by .w leaves as it is
 *
 * Memory-bound passes over RGBA32F surfaces: a pixel per lane in row-major order, 16-B accesses, so a wave instruction covers 1 KiB of
 * consecutive bytes; the prefilter's nine taps read the .w word of neighbouring rows and columns, which the caches hold.  Arithmetic is spelled
 * out per operation (IEEE fp32, no contraction) and mirrored by tests/still_denoise_ref.py, bit for bit. */
#include "dn_launch.h"

#define DN_THREADS 256u

namespace {

__device__ __forceinline__ float dn_luma(float x, float y, float z) { return (x * 0.212671f + y * 0.715160f) + z * 0.072169f; } /* Tonemap.h:12-15 */

__global__ __launch_bounds__(DN_THREADS) void dn_prepare_kernel(const TbFloat4* __restrict__ output, const TbFloat4* __restrict__ jittered,
    TbFloat4* __restrict__ prepared, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const TbFloat4 o = output[i], q = jittered[i];
    const float n = o.w, m = q.w, r = n - m;
    TbFloat4 p{0.0f, 0.0f, 0.0f, 0.0f};
    if (n > 0.0f) { p.x = o.x / n; p.y = o.y / n; p.z = o.z / n; }
    if (m > 0.0f && r > 0.0f) {
        /* the halves' means j and k: E[(luma j - luma k)^2] = s^2 (1/m + 1/r) = s^2 n / (m r), and the mean's variance is s^2 / n */
        const float d = dn_luma(q.x / m, q.y / m, q.z / m) - dn_luma((o.x - q.x) / r, (o.y - q.y) / r, (o.z - q.z) / r);
        const float v = (d * d) * ((m * r) / (n * n));
        p.w = __builtin_fabsf(v) <= 3.402823466e+38f ? v : 0.0f; /* NaN or infinite (sums near FLT_MAX): no estimate */
    }
    prepared[i] = p;
}

__global__ __launch_bounds__(DN_THREADS) void dn_prefilter_kernel(const TbFloat4* __restrict__ prepared, TbFloat4* __restrict__ filtered, uint32_t W,
    uint32_t H, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const int x = (int)(i % W), y = (int)(i / W);
    const float k[2] = {0.5f, 0.25f};
    float acc = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int cx = min(max(x + dx, 0), (int)W - 1), cy = min(max(y + dy, 0), (int)H - 1);
            const float weight = k[dy < 0 ? -dy : dy] * k[dx < 0 ? -dx : dx];
            acc = acc + weight * prepared[(size_t)cy * W + (size_t)cx].w;
        }
    TbFloat4 p = prepared[i];
    p.w = acc;
    filtered[i] = p;
}

__global__ __launch_bounds__(DN_THREADS) void dn_finish_kernel(const TbFloat4* __restrict__ in, TbFloat4* __restrict__ final, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    TbFloat4 p = in[i];
    p.w = 1.0f;
    final[i] = p;
}

/* a frame has at most 16384 pixels a side (tb_render): 2^28 pixels, 2^20 workgroups */
bool dn_frame(uint32_t W, uint32_t H, uint32_t* nPixels, uint32_t* groups)
{
    if (W == 0 || H == 0 || W > 16384u || H > 16384u) return false;
    *nPixels = W * H; *groups = (*nPixels + DN_THREADS - 1u) / DN_THREADS;
    return true;
}
bool dn_surface(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }

} // namespace

extern "C" hipError_t dn_launch_prepare(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, TbFloat4* prepared, uint32_t W, uint32_t H)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(output) || !dn_surface(jittered) || !dn_surface(prepared)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_prepare_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, output, jittered, prepared, nPixels);
    return hipGetLastError();
}

extern "C" hipError_t dn_launch_prefilter(hipStream_t stream, const TbFloat4* prepared, TbFloat4* filtered, uint32_t W, uint32_t H)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(prepared) || !dn_surface(filtered) || prepared == filtered) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_prefilter_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, prepared, filtered, W, H, nPixels);
    return hipGetLastError();
}

extern "C" hipError_t dn_launch_finish(hipStream_t stream, const TbFloat4* in, TbFloat4* final, uint32_t W, uint32_t H)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(in) || !dn_surface(final)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_finish_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, in, final, nPixels);
    return hipGetLastError();
}
