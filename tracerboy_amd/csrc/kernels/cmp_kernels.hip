/* cmp_kernels.hip -- image-quality metrics on the device (include/tracerboy_hip.h tb_run_compare / tb_compare): a test
 * surface against a reference surface, both RGBA32F, alpha ignored.
 *
 *   cmp_pointwise  squared, absolute and relative squared error of every included pixel in fp64, their sums, the largest absolute error and
 *                  the counts; on request the fp32 squared-error map.  Streams both surfaces once with 16-B loads, a pixel per lane per trip of a
 *                  grid-stride loop, four trips' loads in flight: HBM bandwidth is its roofline.
 *   cmp_ssim       SSIM of Wang et al. 2004 (11-tap Gaussian, sigma 1.5, valid region) in fp32 on clamp(x, 0, peak).  One workgroup takes a tile
 *                  of 32 x 32 windows: per channel it stages the two clamped planes of the 42 x 42 pixels under them in LDS, filters the five
 *                  moment planes along rows into LDS and along columns out of it.  No moment image goes to memory; a tile's pixels come from
 *                  HBM for the first channel and from the L2 for the other two.
 *   cmp_finish     one workgroup adds the workgroups' records in index order.
 *
 * A pixel is excluded when it is unsampled (the test surface holds sums and its weight is 0) or when one of its six colour values is not
 * finite; an excluded pixel contributes to nothing, and a window that holds one is skipped.  Every workgroup writes one CmpRecord at its own
 * index: no floating-point atomic, so the sums are the same bits on every call for a given size.  The arithmetic is spelled out per operation
 * (no contraction, IEEE division) and restated by tests/metrics_ref.py: the maps bit for bit, the sums within the any-order bound. */
#include "cmp_launch.h"

#define CMP_THREADS 256u
#define CMP_WAVES (CMP_THREADS / 64u)
#define CMP_HALO (CMP_SSIM_TAPS - 1u)                 /* 10 */
#define CMP_IN (CMP_SSIM_TILE + CMP_HALO)             /* 42: input pixels per tile and axis */
#define CMP_IN_PITCH (CMP_IN + 1u)                    /* 43 */
#define CMP_ROW_PITCH (CMP_SSIM_TILE + 1u)            /* 33: the column reads of the vertical pass step through the banks */
#define CMP_IN_PIXELS (CMP_IN * CMP_IN)               /* 1764 */

namespace {

/* exp(-(i - 5)^2 / 4.5) / sum, rounded to binary32 once and for all: literals here and in the restatement */
#define CMP_W(bits) __builtin_bit_cast(float, (uint32_t)(bits))
__device__ const float cmp_weights[CMP_SSIM_TAPS] = {CMP_W(0x3a86cab6u), CMP_W(0x3bf8ff01u), CMP_W(0x3d13758cu), CMP_W(0x3ddff87fu), CMP_W(0x3e5a1e20u),
    CMP_W(0x3e8832b0u), CMP_W(0x3e5a1e20u), CMP_W(0x3ddff87fu), CMP_W(0x3d13758cu), CMP_W(0x3bf8ff01u), CMP_W(0x3a86cab6u)};
#undef CMP_W
__device__ __forceinline__ float cmp_weight(int i) { return cmp_weights[i]; }

__device__ __forceinline__ bool cmp_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float cmp_clamp(float x, float peak) { return x < 0.0f ? 0.0f : (x > peak ? peak : x); }

/* A pixel of both surfaces as the metrics see it: the test colour (divided by its weight where the surface holds sums), the reference colour,
 * and whether the pixel is excluded / unsampled. */
struct CmpPixel { float a[3], r[3]; bool excluded, unsampled; };
__device__ __forceinline__ CmpPixel cmp_load(const TbFloat4* __restrict__ test, const TbFloat4* __restrict__ ref, size_t i, bool sums)
{
    const float4 t = ((const float4*)test)[i], q = ((const float4*)ref)[i];
    CmpPixel p;
    p.unsampled = sums && t.w == 0.0f;
    p.a[0] = sums ? t.x / t.w : t.x; p.a[1] = sums ? t.y / t.w : t.y; p.a[2] = sums ? t.z / t.w : t.z;
    p.r[0] = q.x; p.r[1] = q.y; p.r[2] = q.z;
    p.excluded = p.unsampled || !(cmp_finite(p.a[0]) && cmp_finite(p.a[1]) && cmp_finite(p.a[2]) && cmp_finite(p.r[0]) && cmp_finite(p.r[1]) &&
        cmp_finite(p.r[2]));
    return p;
}

/* The workgroup's record in thread 0: every field over the wave with shuffles, then the four waves through LDS in wave order.  d[3] is a
 * maximum, the rest are sums. */
__device__ __forceinline__ CmpRecord cmp_group_reduce(CmpRecord v)
{
    __shared__ CmpRecord perWave[CMP_WAVES];
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; k++) v.d[k] = v.d[k] + __shfl_down(v.d[k], (unsigned int)off, 64);
        const double m = __shfl_down(v.d[3], (unsigned int)off, 64);
        v.d[3] = m > v.d[3] ? m : v.d[3];
        for (int k = 0; k < 4; k++) v.n[k] += __shfl_down((unsigned long long)v.n[k], (unsigned int)off, 64);
    }
    __syncthreads(); /* perWave may still be read by a previous call */
    if ((threadIdx.x & 63u) == 0) perWave[threadIdx.x >> 6] = v;
    __syncthreads();
    CmpRecord total = perWave[0];
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < CMP_WAVES; w++) {
            for (int k = 0; k < 3; k++) total.d[k] = total.d[k] + perWave[w].d[k];
            total.d[3] = perWave[w].d[3] > total.d[3] ? perWave[w].d[3] : total.d[3];
            for (int k = 0; k < 4; k++) total.n[k] += perWave[w].n[k];
        }
    return total;
}

/* one pixel into its lane's record, and into the map */
__device__ __forceinline__ void cmp_accumulate(CmpRecord& acc, const CmpPixel& p, double eps, float* __restrict__ sqErrMap, uint32_t i)
{
    float mapValue = 0.0f;
    if (p.excluded) { acc.n[1]++; acc.n[2] += p.unsampled ? 1u : 0u; }
    else {
        double se[3], ae[3], re[3];
        for (int c = 0; c < 3; c++) {
            const double r = (double)p.r[c], d = (double)p.a[c] - r;
            se[c] = d * d; ae[c] = __builtin_fabs(d); re[c] = se[c] / (r * r + eps);
            acc.d[3] = ae[c] > acc.d[3] ? ae[c] : acc.d[3];
        }
        const double pse = (se[0] + se[1]) + se[2];
        acc.d[0] = acc.d[0] + pse;
        acc.d[1] = acc.d[1] + ((ae[0] + ae[1]) + ae[2]);
        acc.d[2] = acc.d[2] + ((re[0] + re[1]) + re[2]);
        acc.n[0]++;
        mapValue = (float)(pse / 3.0);
    }
    if (sqErrMap) sqErrMap[i] = mapValue;
}

__global__ __launch_bounds__(CMP_THREADS) void cmp_pointwise(const TbFloat4* __restrict__ test, const TbFloat4* __restrict__ ref, uint32_t nPixels,
    uint32_t sums, double eps, CmpRecord* __restrict__ partial, float* __restrict__ sqErrMap)
{
    const uint32_t stride = gridDim.x * CMP_THREADS; /* at most 2^19, nPixels at most 2^26: i + 3 stride stays far below 2^32 */
    CmpRecord acc = {{0.0, 0.0, 0.0, 0.0}, {0, 0, 0, 0}};
    uint32_t i = blockIdx.x * CMP_THREADS + threadIdx.x;
    for (; i + 3u * stride < nPixels; i += 4u * stride) { /* eight independent 16-B loads in flight per lane; the pixels still go in in index order */
        const CmpPixel p0 = cmp_load(test, ref, i, sums != 0u), p1 = cmp_load(test, ref, i + stride, sums != 0u),
            p2 = cmp_load(test, ref, i + 2u * stride, sums != 0u), p3 = cmp_load(test, ref, i + 3u * stride, sums != 0u);
        cmp_accumulate(acc, p0, eps, sqErrMap, i); cmp_accumulate(acc, p1, eps, sqErrMap, i + stride);
        cmp_accumulate(acc, p2, eps, sqErrMap, i + 2u * stride); cmp_accumulate(acc, p3, eps, sqErrMap, i + 3u * stride);
    }
    for (; i < nPixels; i += stride) cmp_accumulate(acc, cmp_load(test, ref, i, sums != 0u), eps, sqErrMap, i);
    const CmpRecord total = cmp_group_reduce(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

/* Workgroup (bx, by) takes the windows [32 bx, 32 bx + 32) x [32 by, 32 by + 32) of the (w - 10) x (h - 10) map; window (x, y) covers the pixels
 * [x, x + 11) x [y, y + 11). */
__global__ __launch_bounds__(CMP_THREADS, 3) void cmp_ssim(const TbFloat4* __restrict__ test, const TbFloat4* __restrict__ ref, uint32_t w, uint32_t h,
    uint32_t sums, float peak, float c1, float c2, CmpRecord* __restrict__ partial, float* __restrict__ ssimMap)
{
    __shared__ float sA[CMP_IN * CMP_IN_PITCH], sR[CMP_IN * CMP_IN_PITCH]; /* the clamped planes of one channel */
    __shared__ float sRow[5][CMP_IN * CMP_ROW_PITCH];                      /* a, r, a a, r r, a r filtered along rows */
    __shared__ uint8_t sBad[CMP_IN * CMP_IN], sBadRow[CMP_IN * CMP_SSIM_TILE]; /* excluded pixels; any in the 11 of a row */
    __shared__ double sValue[CMP_SSIM_TILE * CMP_SSIM_TILE];               /* a window's channel values added up in fp64, in the order r, g, b */
    const uint32_t tid = threadIdx.x, ox = blockIdx.x * CMP_SSIM_TILE, oy = blockIdx.y * CMP_SSIM_TILE, mapW = w - CMP_HALO, mapH = h - CMP_HALO;

    /* Every loop but the taps' stays rolled: unrolled, the filter passes' LDS reads are hoisted by the hundred and spill.  So a window's value
     * lives in LDS, where its own thread alone touches it */
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        const uint32_t lane = tid;
        /* the channel's two clamped planes under the tile, an excluded pixel as 0; the first channel also leaves the flags.  Pixels past the
         * frame's edge lie under no window of the map: zeros, not flagged */
#pragma unroll 1
        for (uint32_t idx = lane; idx < CMP_IN_PIXELS; idx += CMP_THREADS) {
            const uint32_t iy = idx / CMP_IN, ix = idx - iy * CMP_IN, gx = ox + ix, gy = oy + iy;
            float a = 0.0f, r = 0.0f;
            bool bad = false;
            if (gx < w && gy < h) {
                const CmpPixel p = cmp_load(test, ref, (size_t)gy * w + gx, sums != 0u);
                bad = p.excluded;
                if (!bad) { a = cmp_clamp(c == 0 ? p.a[0] : c == 1 ? p.a[1] : p.a[2], peak); r = cmp_clamp(c == 0 ? p.r[0] : c == 1 ? p.r[1] : p.r[2], peak); }
            }
            sA[iy * CMP_IN_PITCH + ix] = a; sR[iy * CMP_IN_PITCH + ix] = r;
            if (c == 0) sBad[idx] = bad ? 1u : 0u;
        }
        __syncthreads(); /* also: the previous channel's vertical pass is done with sRow */
#pragma unroll 1
        for (uint32_t o = lane; o < CMP_IN * CMP_SSIM_TILE; o += CMP_THREADS) {
            const uint32_t row = o / CMP_SSIM_TILE, col = o % CMP_SSIM_TILE;
            float ea = 0.0f, er = 0.0f, eaa = 0.0f, err = 0.0f, ear = 0.0f;
#pragma unroll
            for (uint32_t i = 0; i < CMP_SSIM_TAPS; i++) {
                const float a = sA[row * CMP_IN_PITCH + col + i], r = sR[row * CMP_IN_PITCH + col + i], wt = cmp_weight((int)i);
                ea = ea + wt * a; er = er + wt * r; eaa = eaa + wt * (a * a); err = err + wt * (r * r); ear = ear + wt * (a * r);
            }
            const uint32_t at = row * CMP_ROW_PITCH + col;
            sRow[0][at] = ea; sRow[1][at] = er; sRow[2][at] = eaa; sRow[3][at] = err; sRow[4][at] = ear;
            if (c == 0) {
                uint32_t bad = 0;
                for (uint32_t i = 0; i < CMP_SSIM_TAPS; i++) bad |= sBad[row * CMP_IN + col + i];
                sBadRow[o] = (uint8_t)bad;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t o = lane; o < CMP_SSIM_TILE * CMP_SSIM_TILE; o += CMP_THREADS) {
            const uint32_t ty = o / CMP_SSIM_TILE, tx = o % CMP_SSIM_TILE;
            float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (uint32_t i = 0; i < CMP_SSIM_TAPS; i++) {
                const uint32_t at = (ty + i) * CMP_ROW_PITCH + tx;
                const float wt = cmp_weight((int)i);
                for (int p = 0; p < 5; p++) m[p] = m[p] + wt * sRow[p][at];
            }
            const float mua = m[0], mur = m[1];
            const float vA = m[2] - mua * mua, vR = m[3] - mur * mur, cov = m[4] - mua * mur;
            const float num = ((2.0f * mua) * mur + c1) * (2.0f * cov + c2);
            const float den = ((mua * mua + mur * mur) + c1) * ((vA + vR) + c2);
            const double s = (double)(num / den);
            sValue[o] = c == 0 ? s : sValue[o] + s;
        }
    }

    CmpRecord acc = {{0.0, 0.0, 0.0, 0.0}, {0, 0, 0, 0}};
#pragma unroll 1
    for (uint32_t o = tid; o < CMP_SSIM_TILE * CMP_SSIM_TILE; o += CMP_THREADS) {
        const uint32_t ty = o / CMP_SSIM_TILE, tx = o % CMP_SSIM_TILE, wx = ox + tx, wy = oy + ty;
        if (wx >= mapW || wy >= mapH) continue;
        uint32_t bad = 0;
        for (uint32_t i = 0; i < CMP_SSIM_TAPS; i++) bad |= sBadRow[(ty + i) * CMP_SSIM_TILE + tx];
        const double mean = sValue[o] / 3.0;
        if (bad) acc.n[1]++;
        else { acc.n[0]++; acc.d[0] = acc.d[0] + mean; }
        if (ssimMap) ssimMap[(size_t)wy * mapW + wx] = bad ? 0.0f : (float)mean;
    }
    const CmpRecord total = cmp_group_reduce(acc);
    if (tid == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = total;
}

/* one workgroup: result[0] = the nPointwise records in front, result[1] = the nSsim records behind them.  Thread t adds its run of consecutive
 * records in index order; the 256 sums are then reduced as a workgroup's lanes are everywhere here, in a fixed order */
__global__ __launch_bounds__(CMP_THREADS) void cmp_finish(const CmpRecord* __restrict__ partial, uint32_t nPointwise, uint32_t nSsim,
    CmpRecord* __restrict__ result)
{
    for (uint32_t kind = 0; kind < 2u; kind++) {
        const CmpRecord* __restrict__ from = partial + (kind ? nPointwise : 0u);
        const uint32_t count = kind ? nSsim : nPointwise, run = (count + CMP_THREADS - 1u) / CMP_THREADS;
        const uint32_t begin = threadIdx.x * run < count ? threadIdx.x * run : count, end = begin + run < count ? begin + run : count;
        CmpRecord acc = {{0.0, 0.0, 0.0, 0.0}, {0, 0, 0, 0}};
        for (uint32_t g = begin; g < end; g++) {
            const CmpRecord v = from[g];
            for (int k = 0; k < 3; k++) acc.d[k] = acc.d[k] + v.d[k];
            acc.d[3] = v.d[3] > acc.d[3] ? v.d[3] : acc.d[3];
            for (int k = 0; k < 4; k++) acc.n[k] += v.n[k];
        }
        const CmpRecord total = cmp_group_reduce(acc);
        if (threadIdx.x == 0) result[kind] = total;
    }
}

bool cmp_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

} // namespace

extern "C" uint32_t cmp_pointwise_groups(uint32_t w, uint32_t h)
{
    const uint64_t want = ((uint64_t)w * h + CMP_THREADS - 1u) / CMP_THREADS;
    return (uint32_t)(want < 1u ? 1u : want > CMP_MAX_POINTWISE_GROUPS ? CMP_MAX_POINTWISE_GROUPS : want);
}

extern "C" uint32_t cmp_ssim_groups(uint32_t w, uint32_t h)
{
    if (w < CMP_SSIM_TAPS || h < CMP_SSIM_TAPS) return 0u;
    return ((w - CMP_HALO + CMP_SSIM_TILE - 1u) / CMP_SSIM_TILE) * ((h - CMP_HALO + CMP_SSIM_TILE - 1u) / CMP_SSIM_TILE);
}

extern "C" size_t cmp_result_offset(uint32_t w, uint32_t h) { return ((size_t)cmp_pointwise_groups(w, h) + cmp_ssim_groups(w, h)) * sizeof(CmpRecord); }
extern "C" size_t cmp_scratch_bytes(uint32_t w, uint32_t h) { return cmp_result_offset(w, h) + 2u * sizeof(CmpRecord); }

extern "C" hipError_t cmp_launch(hipStream_t stream, uint32_t w, uint32_t h, const TbFloat4* test, const TbFloat4* ref, uint32_t flags, float peak,
    float relEpsilon, void* scratch, float* sqErrMap, float* ssimMap)
{
    if (!test || !ref || !scratch || !cmp_aligned(test) || !cmp_aligned(ref) || !cmp_aligned(scratch) || w == 0 || h == 0 ||
        (uint64_t)w * h > CMP_MAX_PIXELS || (flags & ~(CMP_FLAG_SSIM | CMP_FLAG_TEST_SUMS))) return hipErrorInvalidValue;
    const uint32_t nPointwise = cmp_pointwise_groups(w, h), nSsim = (flags & CMP_FLAG_SSIM) ? cmp_ssim_groups(w, h) : 0u;
    const uint32_t sums = (flags & CMP_FLAG_TEST_SUMS) ? 1u : 0u;
    CmpRecord* const partial = (CmpRecord*)scratch;
    hipLaunchKernelGGL(cmp_pointwise, dim3(nPointwise), dim3(CMP_THREADS), 0, stream, test, ref, w * h, sums, (double)relEpsilon, partial, sqErrMap);
    if (nSsim) {
        const float c1 = (float)((0.01 * (double)peak) * (0.01 * (double)peak)), c2 = (float)((0.03 * (double)peak) * (0.03 * (double)peak));
        const dim3 grid((w - CMP_HALO + CMP_SSIM_TILE - 1u) / CMP_SSIM_TILE, (h - CMP_HALO + CMP_SSIM_TILE - 1u) / CMP_SSIM_TILE);
        hipLaunchKernelGGL(cmp_ssim, grid, dim3(CMP_THREADS), 0, stream, test, ref, w, h, sums, peak, c1, c2, partial + nPointwise, ssimMap);
    }
    hipLaunchKernelGGL(cmp_finish, dim3(1), dim3(CMP_THREADS), 0, stream, (const CmpRecord*)partial, nPointwise, nSsim,
        (CmpRecord*)((char*)scratch + cmp_result_offset(w, h)));
    return hipGetLastError();
}
