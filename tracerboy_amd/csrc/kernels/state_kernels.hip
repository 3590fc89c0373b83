/* state_kernels.hip -- the two device passes of a render state (include/tracerboy_hip.h tb_state_save / tb_state_load /
 * tb_accum_digest): the digest of the accumulation surfaces as they lie in HBM, and the sum of two states.  Both stream each surface once --
 * HBM bandwidth is their roofline -- with 16-B accesses per lane (a wave instruction covers 1 KiB of consecutive bytes), a capped grid and a
 * grid-stride loop that keeps four independent loads in flight per lane.  One launch covers both surfaces (blockIdx.y).
 *
 * state_digest: a 64-bit partial per lane, reduced over the wave with shuffles, over the workgroup through LDS, one partial per workgroup into
 * a small buffer; a second, single-workgroup step adds those up into the two results.  The terms are added mod 2^64 (include/tb_state.h), so
 * no reduction order, grid size or workgroup placement can change the value, and nothing travels to the host in between.
 * state_add: dst += src, IEEE binary32 additions; the translation unit is built like every other one here (no fast math, denormals kept:
 * the accumulated sums rely on exact denormals the way tb_math.h does). */
#include "state_launch.h"
#include "tb_state.h"

#define STATE_THREADS 256u

__device__ __forceinline__ uint64_t state_vec_terms(uint64_t v, uint4 q)
{
    const uint64_t i = v * 4u;
    return tb_state_term(i, q.x) + tb_state_term(i + 1u, q.y) + tb_state_term(i + 2u, q.z) + tb_state_term(i + 3u, q.w);
}

/* the workgroup's sum in thread 0 (wave64: shuffles, then the four waves through LDS) */
__device__ __forceinline__ uint64_t state_group_sum(uint64_t s)
{
    __shared__ uint64_t perWave[STATE_THREADS / 64u];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down((unsigned long long)s, (unsigned int)off, 64);
    __syncthreads(); /* perWave may still be read by a previous call */
    if ((threadIdx.x & 63u) == 0) perWave[threadIdx.x >> 6] = s;
    __syncthreads();
    uint64_t total = 0;
    if (threadIdx.x == 0) for (uint32_t w = 0; w < STATE_THREADS / 64u; w++) total += perWave[w];
    return total;
}

__global__ __launch_bounds__(STATE_THREADS) void state_digest_partials(const uint4* __restrict__ a, const uint4* __restrict__ b, uint64_t nVec,
    uint64_t nWords, uint64_t* __restrict__ partial)
{
    const uint4* __restrict__ p = blockIdx.y ? b : a;
    const uint64_t stride = (uint64_t)gridDim.x * STATE_THREADS;
    uint64_t v = (uint64_t)blockIdx.x * STATE_THREADS + threadIdx.x;
    uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (; v + 3u * stride < nVec; v += 4u * stride) {
        const uint4 q0 = p[v], q1 = p[v + stride], q2 = p[v + 2u * stride], q3 = p[v + 3u * stride];
        s0 += state_vec_terms(v, q0); s1 += state_vec_terms(v + stride, q1);
        s2 += state_vec_terms(v + 2u * stride, q2); s3 += state_vec_terms(v + 3u * stride, q3);
    }
    for (; v < nVec; v += stride) s0 += state_vec_terms(v, p[v]);
    /* the words behind the last whole vector (none for a surface: a pixel is one vector) */
    const uint64_t tail = nVec * 4u + threadIdx.x;
    if (blockIdx.x == 0 && tail < nWords) s1 += tb_state_term(tail, ((const uint32_t*)p)[tail]);
    const uint64_t total = state_group_sum(s0 + s1 + s2 + s3);
    if (threadIdx.x == 0) partial[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

/* one workgroup: result[k] = sum of surface k's `groups` partials */
__global__ __launch_bounds__(STATE_THREADS) void state_digest_final(const uint64_t* __restrict__ partial, uint32_t groups, uint64_t* __restrict__ result)
{
    for (uint32_t k = 0; k < 2u; k++) {
        uint64_t s = 0;
        for (uint32_t g = threadIdx.x; g < groups; g += STATE_THREADS) s += partial[(uint64_t)k * groups + g];
        const uint64_t total = state_group_sum(s);
        if (threadIdx.x == 0) result[k] = total;
    }
}

__device__ __forceinline__ float4 state_add4(float4 d, float4 s) { return make_float4(d.x + s.x, d.y + s.y, d.z + s.z, d.w + s.w); }

__global__ __launch_bounds__(STATE_THREADS) void state_add_kernel(float4* __restrict__ dstA, const float4* __restrict__ srcA, float4* __restrict__ dstB,
    const float4* __restrict__ srcB, uint64_t nVec, uint64_t nWords)
{
    float4* __restrict__ d = blockIdx.y ? dstB : dstA;
    const float4* __restrict__ s = blockIdx.y ? srcB : srcA;
    const uint64_t stride = (uint64_t)gridDim.x * STATE_THREADS;
    uint64_t v = (uint64_t)blockIdx.x * STATE_THREADS + threadIdx.x;
    for (; v + stride < nVec; v += 2u * stride) { /* four loads in flight, two stores */
        const float4 d0 = d[v], s0 = s[v], d1 = d[v + stride], s1 = s[v + stride];
        d[v] = state_add4(d0, s0); d[v + stride] = state_add4(d1, s1);
    }
    if (v < nVec) d[v] = state_add4(d[v], s[v]);
    const uint64_t tail = nVec * 4u + threadIdx.x;
    if (blockIdx.x == 0 && tail < nWords) ((float*)d)[tail] = ((const float*)d)[tail] + ((const float*)s)[tail];
}

static uint32_t state_groups(uint64_t nVec)
{
    const uint64_t want = (nVec + STATE_THREADS - 1u) / STATE_THREADS;
    return (uint32_t)(want < 1u ? 1u : want > TB_STATE_DIGEST_MAX_GROUPS ? TB_STATE_DIGEST_MAX_GROUPS : want);
}
static bool state_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" hipError_t state_launch_digest(hipStream_t stream, const uint32_t* surfaceA, const uint32_t* surfaceB, uint64_t nWords, uint64_t* scratch)
{
    if (!scratch || (nWords && (!surfaceA || !surfaceB)) || !state_aligned(surfaceA) || !state_aligned(surfaceB)) return hipErrorInvalidValue;
    const uint64_t nVec = nWords / 4u;
    const uint32_t groups = state_groups(nVec);
    hipLaunchKernelGGL(state_digest_partials, dim3(groups, 2), dim3(STATE_THREADS), 0, stream, (const uint4*)surfaceA, (const uint4*)surfaceB, nVec, nWords,
        scratch);
    hipLaunchKernelGGL(state_digest_final, dim3(1), dim3(STATE_THREADS), 0, stream, (const uint64_t*)scratch, groups,
        scratch + 2u * TB_STATE_DIGEST_MAX_GROUPS);
    return hipGetLastError();
}

extern "C" hipError_t state_launch_add(hipStream_t stream, float* dstA, const float* srcA, float* dstB, const float* srcB, uint64_t nWords)
{
    if (nWords == 0) return hipSuccess;
    if (!dstA || !srcA || !dstB || !srcB || !state_aligned(dstA) || !state_aligned(srcA) || !state_aligned(dstB) || !state_aligned(srcB))
        return hipErrorInvalidValue;
    const uint64_t nVec = nWords / 4u;
    hipLaunchKernelGGL(state_add_kernel, dim3(state_groups(nVec), 2), dim3(STATE_THREADS), 0, stream, (float4*)dstA, (const float4*)srcA, (float4*)dstB,
        (const float4*)srcB, nVec, nWords);
    return hipGetLastError();
}
