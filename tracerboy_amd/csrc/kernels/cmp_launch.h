/* cmp_launch.h -- the launcher of cmp_kernels.hip: image-quality metrics of one RGBA32F surface against another.  It knows
 * nothing about contexts or options.  test and ref are device surfaces of w x h pixels, row-major, 16-B aligned; both are only read.
 *
 * One call enqueues cmp_pointwise, cmp_ssim when CMP_FLAG_SSIM is set and the frame holds a window, and cmp_finish.  scratch holds
 * cmp_scratch_bytes(w, h) bytes: one CmpRecord per workgroup of the first two kernels, each written at the workgroup's own index, then the two
 * records cmp_finish adds them up to, at byte offset cmp_result_offset(w, h).  No floating-point atomic anywhere: for a given w x h the result
 * is the same bits on every call.
 *
 * The launcher refuses (hipErrorInvalidValue) a null or misaligned surface or scratch, a zero dimension, more than 2^26 pixels and unknown flags. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tb_abi.h"

#define CMP_FLAG_SSIM 1u      /* run cmp_ssim */
#define CMP_FLAG_TEST_SUMS 2u /* test holds sums: rgb / w per channel, and a pixel with w == 0 is unsampled */
#define CMP_SSIM_TILE 32u     /* cmp_ssim: windows per workgroup and axis */
#define CMP_SSIM_TAPS 11u
#define CMP_MAX_POINTWISE_GROUPS 2048u
#define CMP_MAX_PIXELS (1ull << 26)

/* What a workgroup, and in the end the call, reports.  cmp_pointwise: d = sum of squared errors, sum of absolute errors, sum of relative squared
 * errors, largest absolute error; n = included pixels, excluded pixels, unsampled pixels (part of the excluded), 0.  cmp_ssim: d[0] = sum of the
 * window values; n = windows that count, windows skipped.  The result holds one record of each kind, in that order. */
typedef struct CmpRecord { double d[4]; uint64_t n[4]; } CmpRecord;

extern "C" {
uint32_t cmp_pointwise_groups(uint32_t w, uint32_t h);
uint32_t cmp_ssim_groups(uint32_t w, uint32_t h); /* 0: the frame holds no window */
size_t cmp_result_offset(uint32_t w, uint32_t h);
size_t cmp_scratch_bytes(uint32_t w, uint32_t h);
/* sqErrMap (w x h floats) and ssimMap ((w - 10) x (h - 10) floats) may be null; ssimMap is not touched without a window */
hipError_t cmp_launch(hipStream_t stream, uint32_t w, uint32_t h, const TbFloat4* test, const TbFloat4* ref, uint32_t flags, float peak, float relEpsilon,
                      void* scratch, float* sqErrMap, float* ssimMap);
}
