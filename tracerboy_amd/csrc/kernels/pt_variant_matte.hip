/* pt_variant_matte.hip -- copy "matte" of pt_copies.h: the base copy of feature set "matte" (pt_device_features.h),
 * 113 VGPRs, 4 waves per SIMD.  pt_variant_matte5.hip is the copy at 5 waves per SIMD the host prefers when LDS has room. */
#define PT_COPY matte
#include "pt_variant.inc"
