/* pt_variant_vol.hip -- copy "vol" of pt_copies.h: the base copy of feature set "vol" (pt_device_features.h).
 * The SSS / mix-material path state needs ~200 VGPRs (2 waves per SIMD); the scenes that use it are large and wait on memory,
 * so the kernel is held to 3 waves per SIMD (168 VGPRs, the rest spilled to scratch: +37 % on the 0.7 M-triangle van-class
 * scene, +39 % on the 3 M-triangle bistro-class scene at 4K).  pt_variant_vol4.hip is the same at 4 waves per SIMD, used when
 * the traversal stack leaves LDS for four workgroups per CU. */
#define PT_COPY vol
#include "pt_variant.inc"
