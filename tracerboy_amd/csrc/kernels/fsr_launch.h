/* fsr_launch.h -- the launchers of fsr_kernels.hip: FSR 1's two passes.  Neither knows about contexts or options.
 * surface is TB_FSR_SURFACE_UNORM8 (4-B texels, 4-B aligned) or TB_FSR_SURFACE_F32 (16-B texels, 16-B aligned); in and out are device
 * surfaces of that type, row-major, row 0 = top, and must not be the same (both passes read neighbours).  A launcher refuses
 * (hipErrorInvalidValue) a null, misaligned or aliased surface, an unknown surface type, a zero dimension and more than 2^24 pixels. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tb_abi.h"

extern "C" {
/* EASU: in is inW x inH, out is outW x outH; con0 = TbFsrConstants::easu[0..3] (the only words the integer-tap form reads) */
hipError_t fsr_launch_easu(hipStream_t stream, uint32_t surface, const uint32_t con0[4], uint32_t inW, uint32_t inH, uint32_t outW, uint32_t outH,
                           const void* in, void* out);
/* RCAS: in and out are W x H; con = TbFsrConstants::rcas[0] */
hipError_t fsr_launch_rcas(hipStream_t stream, uint32_t surface, uint32_t con, uint32_t W, uint32_t H, const void* in, void* out);
}
