/* pt_variant_full.hip -- copy "full" of pt_copies.h: feature set "full" (pt_device_features.h), with the counting kernels.
 * 231-250 VGPRs (2 waves per SIMD) held to 168 + scratch: +27 % on cornell-box and the 870 k scene with every feature on; 4 waves lose. */
#define PT_COPY full
#include "pt_variant.inc"
