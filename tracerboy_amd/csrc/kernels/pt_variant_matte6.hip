/* pt_variant_matte6.hip -- feature set "matte" at 6 waves per SIMD (80 VGPRs, 96 B of scratch, none of it inside the walk loops), for scenes in LDS
 * only: the frame-group kernels with the whole stack in LDS.  Chosen over the 5-wave copy (pt_variant_matte5.hip) when six workgroups per CU fit
 * (stack + the walk's LDS image <= 26 KB, launch_plan.h LdsCopyFits): cornell-box 1920x1080x64 7 136 -> 7 426 Msamples/s (docs/experiments/r7.md).
 * Scenes fetched from memory keep the 5-wave copy. */
#include "pt_device_features.h"
#define PT_FEATURES 0u
#define PT_NAME matte6
#define PT_COUNT 0
#define PT_ONLY_PERSISTENT 1
#define PT_ONLY_LDS_GROUPS 1
#ifndef TB_MATTE_LDS_WAVES
#define TB_MATTE_LDS_WAVES 6 /* context.cpp reads the same macro */
#endif
#define PT_PERSISTENT_ATTR __attribute__((amdgpu_waves_per_eu(TB_MATTE_LDS_WAVES))) /* keep in step with kVariants[].wavesLds, context.cpp */
#include "pt_variant.inc"
