/* dn_kernels.hip -- what a still's denoise adds around the a-trous filter of rt_kernels.hip (include/tracerboy_hip.h
 * tb_denoise).  A progressive render has no luminance moments; it has two independent halves of every pixel's samples: the jittered surface
 * holds the samples whose coin fell below 0.5, the output surface holds all of them (RayGenCommon.h:721-727).
 *
 *   dn_prepare_kernel     mean colour, and the variance of its luminance from the difference of the two halves' means
 *   dn_prefilter_kernel   3x3 Gaussian over that variance (a one-sample chi-square estimate per pixel), coordinates clamped to the frame
 *   dn_finish_kernel      (rgb, 1): a surface the output stage's division by .w leaves as it is
 * and for the chain that takes its guides from the guide pass (guide_kernels.hip; DESIGN.md section 13, option "denoise_guides"):
 *   dn_resolve_guides_kernel  the sums of the guide pass to the filter's normals and positions: sum / frames that hit, zero where none did
 *   dn_prepare_demod_kernel   dn_prepare_kernel with the mean colour and both halves' means divided by d = max(mean effective albedo, 0.01)
 *   dn_finish_remod_kernel    (rgb * d, 1)
 *
 * Memory-bound passes over RGBA32F surfaces: a pixel per lane in row-major order, 16-B accesses, so a wave instruction covers 1 KiB of
 * consecutive bytes; the prefilter's nine taps read the .w word of neighbouring rows and columns, which the caches hold.  Arithmetic is spelled
 * out per operation (IEEE fp32, no contraction) and mirrored by tests/still_denoise_ref.py, bit for bit. */
#include "dn_launch.h"
#include "tb_math.h"

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

/* ---- the guide pass's chain ---- */
__global__ __launch_bounds__(DN_THREADS) void dn_resolve_guides_kernel(const TbFloat4* __restrict__ gNormal, const TbFloat4* __restrict__ gPosition,
    TbFloat4* __restrict__ normals, TbFloat4* __restrict__ positions, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const TbFloat4 n = gNormal[i], p = gPosition[i];
    const float hits = n.w; /* one frame: a division by 1, the frame's AOVs bit for bit */
    TbFloat4 on{0.0f, 0.0f, 0.0f, 1.0f}, op{0.0f, 0.0f, 0.0f, 0.0f};
    if (hits > 0.0f) { on.x = n.x / hits; on.y = n.y / hits; on.z = n.z / hits; op.x = p.x / hits; op.y = p.y / hits; op.z = p.z / hits; op.w = p.w / hits; }
    /* The mean of several frames' normals is shorter than 1 where they disagree (a silhouette inside the pixel), and DenoiserCS raises the dot
     * product of two normals to NormalWeightingExponential: the centre tap's own weight |n|^(2 x 128) underflows to 0 from |n| = 0.5 down and
     * the pass divides 0 by 0.  More than one frame: the mean's direction, or no normal at all (the pixel keeps its mean) where the sum cancels. */
    if (hits > 1.0f) {
        const float l = tb_sqrt((on.x * on.x + on.y * on.y) + on.z * on.z);
        if (l > 0.0f) { on.x = on.x / l; on.y = on.y / l; on.z = on.z / l; } else { on.x = 0.0f; on.y = 0.0f; on.z = 0.0f; }
    }
    normals[i] = on; positions[i] = op;
}

/* d: the mean effective albedo per channel, held away from zero */
__device__ __forceinline__ float dn_demod(float sum, float frames) { const float a = sum / frames; return a > 0.01f ? a : 0.01f; }

__global__ __launch_bounds__(DN_THREADS) void dn_prepare_demod_kernel(const TbFloat4* __restrict__ output, const TbFloat4* __restrict__ jittered,
    const TbFloat4* __restrict__ gAlbedo, TbFloat4* __restrict__ prepared, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const TbFloat4 o = output[i], q = jittered[i], a = gAlbedo[i];
    const float dx = dn_demod(a.x, a.w), dy = dn_demod(a.y, a.w), dz = dn_demod(a.z, a.w);
    const float n = o.w, m = q.w, r = n - m;
    TbFloat4 p{0.0f, 0.0f, 0.0f, 0.0f};
    if (n > 0.0f) { p.x = (o.x / n) / dx; p.y = (o.y / n) / dy; p.z = (o.z / n) / dz; }
    if (m > 0.0f && r > 0.0f) {
        const float d = dn_luma((q.x / m) / dx, (q.y / m) / dy, (q.z / m) / dz) - dn_luma(((o.x - q.x) / r) / dx, ((o.y - q.y) / r) / dy, ((o.z - q.z) / r) / dz);
        const float v = (d * d) * ((m * r) / (n * n));
        p.w = __builtin_fabsf(v) <= 3.402823466e+38f ? v : 0.0f;
    }
    prepared[i] = p;
}

__global__ __launch_bounds__(DN_THREADS) void dn_finish_remod_kernel(const TbFloat4* __restrict__ in, const TbFloat4* __restrict__ gAlbedo,
    TbFloat4* __restrict__ final, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const TbFloat4 x = in[i], a = gAlbedo[i];
    final[i] = TbFloat4{x.x * dn_demod(a.x, a.w), x.y * dn_demod(a.y, a.w), x.z * dn_demod(a.z, a.w), 1.0f};
}

/* ---- the noise target of a sample budget (tb_budget_stop_converged) ----
 * A pixel that is still live at frame F (budget > F) stops -- budget = F -- once F has reached minFrames, the pixel holds samples and either its mean
 * is black or the prefiltered variance of the mean's luminance (filtered.w, the two passes above) is below relError^2 (luma^2 + 0.01), the floor of
 * section 12's relMSE.  NaN compares false: such a pixel stays live.  Every lane of a wave reaches the ballots; counts[0] += the pixels stopped,
 * counts[1] += the pixels live afterwards, one integer add per wave -- whatever the order, the same sums. */
__global__ __launch_bounds__(DN_THREADS) void budget_stop_kernel(const TbFloat4* __restrict__ output, const TbFloat4* __restrict__ jittered,
    const TbFloat4* __restrict__ filtered, uint32_t* __restrict__ budget, uint32_t nPixels, uint32_t F, uint32_t minFrames, float relError,
    unsigned long long* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * DN_THREADS + threadIdx.x;
    bool stop = false, liveAfter = false;
    if (i < nPixels && budget[i] > F) {
        const TbFloat4 o = output[i], q = jittered[i];
        const float n = o.w, m = q.w, r = n - m;
        if (F >= minFrames && n > 0.0f) {
            const float cx = o.x / n, cy = o.y / n, cz = o.z / n;
            const float l = dn_luma(cx, cy, cz), V = filtered[i].w;
            const float threshold = (relError * relError) * ((l * l) + 0.01f);
            stop = (cx <= 0.0f && cy <= 0.0f && cz <= 0.0f) || (m > 0.0f && r > 0.0f && V < threshold);
        }
        if (stop) budget[i] = F; else liveAfter = true;
    }
    const unsigned long long s = __ballot(stop), l = __ballot(liveAfter);
    if ((threadIdx.x & 63u) == 0) {
        if (s) atomicAdd(&counts[0], (unsigned long long)__popcll(s));
        if (l) atomicAdd(&counts[1], (unsigned long long)__popcll(l));
    }
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

extern "C" hipError_t dn_launch_resolve_guides(hipStream_t stream, const TbFloat4* gNormal, const TbFloat4* gPosition, TbFloat4* normals, TbFloat4* positions,
    uint32_t W, uint32_t H)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(gNormal) || !dn_surface(gPosition) || !dn_surface(normals) || !dn_surface(positions)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_resolve_guides_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, gNormal, gPosition, normals, positions, nPixels);
    return hipGetLastError();
}

extern "C" hipError_t dn_launch_prepare_demod(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, const TbFloat4* gAlbedo, TbFloat4* prepared,
    uint32_t W, uint32_t H)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(output) || !dn_surface(jittered) || !dn_surface(gAlbedo) || !dn_surface(prepared)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_prepare_demod_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, output, jittered, gAlbedo, prepared, nPixels);
    return hipGetLastError();
}

extern "C" hipError_t dn_launch_finish_remod(hipStream_t stream, const TbFloat4* in, const TbFloat4* gAlbedo, TbFloat4* final, uint32_t W, uint32_t H)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(in) || !dn_surface(gAlbedo) || !dn_surface(final)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_finish_remod_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, in, gAlbedo, final, nPixels);
    return hipGetLastError();
}

extern "C" hipError_t dn_launch_budget_stop(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, const TbFloat4* filtered, uint32_t* budget,
    uint32_t W, uint32_t H, uint32_t frame, uint32_t minFrames, float relError, unsigned long long* counts)
{
    uint32_t nPixels, groups;
    if (!dn_frame(W, H, &nPixels, &groups) || !dn_surface(output) || !dn_surface(jittered) || !dn_surface(filtered) || !budget || !counts) return hipErrorInvalidValue;
    hipLaunchKernelGGL(budget_stop_kernel, dim3(groups), dim3(DN_THREADS), 0, stream, output, jittered, filtered, budget, nPixels, frame, minFrames, relError, counts);
    return hipGetLastError();
}
