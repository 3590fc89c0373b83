/* state_launch.h -- the launchers of state_kernels.hip: the digest of the two accumulation surfaces and their sum with another state's
 * (DESIGN.md section 11).  Both kernels stream the surfaces once; neither knows about frames, tiles or files. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TB_STATE_DIGEST_MAX_GROUPS 2048u /* workgroups per surface of the first step; the grid-stride loop takes the rest */
/* 64-bit words of scratch the digest needs: one partial per workgroup and surface, then the two results */
#define TB_STATE_DIGEST_SCRATCH_WORDS (2u * TB_STATE_DIGEST_MAX_GROUPS + 2u)

extern "C" {
/* digest (include/tb_state.h) of surfaceA[0..nWords) and of surfaceB[0..nWords), 32-bit words, into scratch[2 * MAX_GROUPS + 0 / 1]; the surfaces
 * 16-B aligned.  Two launches on `stream`, nothing read back. */
hipError_t state_launch_digest(hipStream_t stream, const uint32_t* surfaceA, const uint32_t* surfaceB, uint64_t nWords, uint64_t* scratch);
/* dstA[i] += srcA[i], dstB[i] += srcB[i] for i < nWords: IEEE fp32 additions, denormals kept; all four 16-B aligned */
hipError_t state_launch_add(hipStream_t stream, float* dstA, const float* srcA, float* dstB, const float* srcB, uint64_t nWords);
}
