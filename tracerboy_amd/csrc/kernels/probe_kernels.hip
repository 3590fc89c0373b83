/* probe_kernels.hip -- light probes around the two queries (include/tracerboy_hip.h tb_bake_probes, tb_sample_probes).
 * probe_launch.h states the arithmetic, which is the contract.
 *
 *   probe_rays     one lane per (probe, texel): the texel's direction, the radiance record and the distance record of that ray
 *   probe_project  one wave per probe: lane l folds the rays l, l + 64, ... of the probe into 27 SH sums and five statistics, six butterfly steps
 *                  of cross-lane shuffles leave the totals in every lane, lane k stores dword k of the 128-B record.  No LDS, no atomics.
 *   probe_sample   one lane per point: the eight corners of its cell, the invalid ones left out
 * Every index a kernel forms is below a count it was given: rays below n * M * M, probes below n (below the grid's product in probe_sample, every
 * corner index clamped to its axis), points below n. */
#include <hip/hip_runtime.h>
#include "tb_abi.h"
#include "probe_launch.h"

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ bool finite3(const float* p) { return probe_finite(p[0]) && probe_finite(p[1]) && probe_finite(p[2]); }

__global__ __launch_bounds__(BLOCK) void probe_rays(const float* __restrict__ positions, uint32_t n, uint32_t M, uint32_t firstNumber,
    TbRadianceRay* __restrict__ radianceRays, TbQueryRay* __restrict__ queryRays)
{
    const uint32_t texels = M * M;
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= (uint64_t)n * texels) return;
    const uint32_t i = (uint32_t)(r / texels), t = (uint32_t)(r % texels);
    const float* P = positions + 3ull * i;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, e = a;
    if (finite3(P)) {
        float d[3], w;
        probe_direction(M, t % M, t / M, d, &w);
        a = make_float4(P[0], P[1], P[2], (float)(firstNumber + i)); b = make_float4(d[0], d[1], d[2], (float)t);
        c = make_float4(P[0], P[1], P[2], __builtin_inff()); e = make_float4(d[0], d[1], d[2], 0.0f); /* Flags 0 */
    }
    float4* rr = (float4*)(radianceRays + r); float4* qr = (float4*)(queryRays + r);
    rr[0] = a; rr[1] = b; qr[0] = c; qr[1] = e;
}

__device__ __forceinline__ float other(float v, int distance) { return __shfl_xor(v, distance, 64); }

__global__ __launch_bounds__(BLOCK) void probe_project(const float* __restrict__ positions, uint32_t n, uint32_t M, const TbFloat4* __restrict__ sums,
    const TbQueryHit* __restrict__ hits, TbProbe* __restrict__ probes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * (BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6); /* the wave's probe */
    if (i >= n) return;
    const uint32_t texels = M * M;
    const uint64_t first = (uint64_t)i * texels;
    float acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0f;
    float W = 0.0f, D = 0.0f, H = 0.0f, B = 0.0f, Dmin = __builtin_inff();
    for (uint32_t t = lane; t < texels; t += 64u) {
        float d[3], w;
        probe_direction(M, t % M, t / M, d, &w);
        const TbFloat4 s = sums[first + t];
        const TbQueryHit* hit = hits + first + t;
        const float T = hit->T, nx = hit->Normal[0], ny = hit->Normal[1], nz = hit->Normal[2];
        if (s.w > 0.0f) {
            float Y[9];
            probe_basis(d[0], d[1], d[2], Y);
            const float q[3] = {(s.x / s.w) * w, (s.y / s.w) * w, (s.z / s.w) * w};
#pragma unroll
            for (int j = 0; j < 9; j++) {
#pragma unroll
                for (int c = 0; c < 3; c++) acc[j * 3 + c] = acc[j * 3 + c] + (q[c] * Y[j]);
            }
            W = W + w;
        }
        if (T >= 0.0f) {
            D = D + T; H = H + 1.0f; Dmin = fminf(Dmin, T);
            if (((nx * d[0]) + (ny * d[1])) + nz * d[2] > 0.0f) B = B + 1.0f;
        }
    }
#pragma unroll
    for (int distance = 32; distance >= 1; distance >>= 1) {
#pragma unroll
        for (int k = 0; k < 27; k++) acc[k] = acc[k] + other(acc[k], distance);
        W = W + other(W, distance); D = D + other(D, distance); H = H + other(H, distance); B = B + other(B, distance);
        Dmin = fminf(Dmin, other(Dmin, distance));
    }
    const bool placed = finite3(positions + 3ull * i);
    const bool lit = placed && W != 0.0f, met = placed && H != 0.0f;
    /* lane k keeps dword k of the record: a chain of selects, no indexed register array */
    float mine = 0.0f;
#pragma unroll
    for (int k = 0; k < 27; k++) if (lane == (uint32_t)k) mine = lit ? (PROBE_FOUR_PI * acc[k]) / W : 0.0f;
    if (lane == 27u) mine = placed ? W : 0.0f;
    if (lane == 28u) mine = placed ? H : 0.0f;
    if (lane == 29u) mine = placed ? B : 0.0f;
    if (lane == 30u) mine = met ? Dmin : -1.0f;
    if (lane == 31u) mine = met ? D / H : -1.0f;
    if (lane < 32u) ((float*)(probes + i))[lane] = mine;
}

__global__ __launch_bounds__(BLOCK) void probe_sample(tb_probe_grid grid, uint32_t M, float backfaceLimit, const TbProbe* __restrict__ probes, uint32_t n,
    const float* __restrict__ points, const float* __restrict__ normals, TbFloat4* __restrict__ out)
{
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    uint32_t i0[3]; float f[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float g = (points[3ull * p + a] - grid.origin[a]) / grid.spacing[a];
        g = fminf(fmaxf(g, 0.0f), (float)(grid.count[a] - 1u));
        const int whole = grid.count[a] == 1u ? 0 : min((int)floorf(g), (int)grid.count[a] - 2);
        i0[a] = (uint32_t)whole; f[a] = g - (float)whole;
    }
    const float most = backfaceLimit * (float)(M * M);
    float S[27];
#pragma unroll
    for (int k = 0; k < 27; k++) S[k] = 0.0f;
    float Wsum = 0.0f;
#pragma unroll 1 /* one corner's record in registers at a time: unrolled, the eight gathers are hoisted together and the kernel takes 169 VGPRs */
    for (int c = 0; c < 8; c++) {
        const uint32_t dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const uint32_t ix = min(i0[0] + dx, grid.count[0] - 1u), iy = min(i0[1] + dy, grid.count[1] - 1u), iz = min(i0[2] + dz, grid.count[2] - 1u);
        const float wc = ((dx ? f[0] : 1.0f - f[0]) * (dy ? f[1] : 1.0f - f[1])) * (dz ? f[2] : 1.0f - f[2]);
        const float4* rec = (const float4*)(probes + ((uint64_t)iz * grid.count[1] + iy) * grid.count[0] + ix);
        const float4 tail = rec[7]; /* Hits, Backfaces, MinDistance, MeanDistance; Weight is rec[6].w */
        const float4 r6 = rec[6];
        if (!(r6.w > 0.0f && tail.y <= most)) continue;
        float v[28];
#pragma unroll
        for (int k = 0; k < 6; k++) { const float4 r = rec[k]; v[4 * k] = r.x; v[4 * k + 1] = r.y; v[4 * k + 2] = r.z; v[4 * k + 3] = r.w; }
        v[24] = r6.x; v[25] = r6.y; v[26] = r6.z;
#pragma unroll
        for (int k = 0; k < 27; k++) S[k] = S[k] + (wc * v[k]);
        Wsum = Wsum + wc;
    }
    TbFloat4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    if (Wsum != 0.0f) {
        float Y[9];
        probe_basis(normals[3ull * p], normals[3ull * p + 1], normals[3ull * p + 2], Y);
        /* nine quotients at a time: scheduled for ILP all 27 divisions run side by side and their temporaries take the kernel to 169 VGPRs */
#pragma unroll
        for (int k = 0; k < 27; k++) { S[k] = S[k] / Wsum; if (k % 9 == 8) __builtin_amdgcn_sched_barrier(0); }
        o.x = probe_sh9_channel(S + 0, 3, Y); o.y = probe_sh9_channel(S + 1, 3, Y); o.z = probe_sh9_channel(S + 2, 3, Y); o.w = Wsum;
    }
    out[p] = o;
}

} // namespace

extern "C" hipError_t probe_launch_rays(hipStream_t stream, const float* positions, uint32_t n, uint32_t M, uint32_t firstNumber, TbRadianceRay* radianceRays,
    TbQueryRay* queryRays)
{
    if (!n) return hipSuccess;
    if (M < PROBE_MIN_RES || M > PROBE_MAX_RES || !positions || !radianceRays || !queryRays) return hipErrorInvalidValue;
    const uint64_t rays = (uint64_t)n * M * M;
    if (rays > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_rays, dim3((uint32_t)((rays + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, positions, n, M, firstNumber, radianceRays, queryRays);
    return hipGetLastError();
}

extern "C" hipError_t probe_launch_project(hipStream_t stream, const float* positions, uint32_t n, uint32_t M, const TbFloat4* sums, const TbQueryHit* hits,
    TbProbe* probes)
{
    if (!n) return hipSuccess;
    if (M < PROBE_MIN_RES || M > PROBE_MAX_RES || !positions || !sums || !hits || !probes || (uint64_t)n * M * M > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_project, dim3((n + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, stream, positions, n, M, sums, hits, probes);
    return hipGetLastError();
}

extern "C" hipError_t probe_launch_sample(hipStream_t stream, const tb_probe_grid* grid, uint32_t M, float backfaceLimit, const TbProbe* probes, uint32_t n,
    const float* points, const float* normals, TbFloat4* out)
{
    if (!n) return hipSuccess;
    if (!grid || M < PROBE_MIN_RES || M > PROBE_MAX_RES || !probes || !points || !normals || !out) return hipErrorInvalidValue;
    if (!grid->count[0] || !grid->count[1] || !grid->count[2] || (uint64_t)grid->count[0] * grid->count[1] * grid->count[2] > (1ull << 24)) return hipErrorInvalidValue;
    if (n > (1u << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_sample, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, *grid, M, backfaceLimit, probes, n, points, normals, out);
    return hipGetLastError();
}
