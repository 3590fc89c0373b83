/* pt_variant_matte5.hip -- copy "matte5" of pt_copies.h: feature set "matte" at 5 waves per SIMD (96 VGPRs, about ten registers in scratch), lock-step only.
 * Chosen when five workgroups per CU fit in LDS (stack + scene image <= 32 KB): cornell-box 1920x1080x64 +9 %.  Frame-group launches of scenes in LDS
 * whose stack and image fit six workgroups per CU run pt_variant_matte6.hip instead. */
#define PT_COPY matte5
#include "pt_variant.inc"
