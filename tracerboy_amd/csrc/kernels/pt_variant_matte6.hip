/* pt_variant_matte6.hip -- copy "matte6" of pt_copies.h: feature set "matte" at 6 waves per SIMD (80 VGPRs, 96 B of scratch, none of it inside the walk
 * loops), for scenes in LDS only: the frame-group kernels with the whole stack in LDS.  Chosen over the 5-wave copy (pt_variant_matte5.hip) when six
 * workgroups per CU fit (stack + the walk's LDS image <= 26 KB, launch_plan.h LdsCopyFits): cornell-box 1920x1080x64 7 136 -> 7 426 Msamples/s
 * (docs/experiments/r7.md).  Scenes fetched from memory keep the 5-wave copy. */
#define PT_COPY matte6
#include "pt_variant.inc"
