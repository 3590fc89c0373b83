/* pt_variant_sss.hip -- copy "sss" of pt_copies.h: the base copy of feature set "sss", everything "vol" has except mix materials.
 * Without MIX_MATERIAL_FLAG judging a shadow feeler draws no random number, so the kernel finishes the bounce before it traces the
 * feeler (pt_persistent.inc, slot 2) and carries only the compact between-bounces state across that walk: held to the same occupancy
 * it spills half as much as "vol" (4 waves per SIMD: 136 against 264 spilled registers).  The glass / translucent scenes of
 * BASELINE.json configs[3] and [4] have no mix materials and run here. */
#define PT_COPY sss
#include "pt_variant.inc"
