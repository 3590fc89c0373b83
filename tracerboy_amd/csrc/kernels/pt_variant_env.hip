/* pt_variant_env.hip -- copy "env" of pt_copies.h: the base copy of feature set "env" (pt_device_features.h),
 * 4 waves per SIMD.  pt_variant_env5.hip is the copy at a higher occupancy the host prefers when LDS has room. */
#define PT_COPY env
#include "pt_variant.inc"
