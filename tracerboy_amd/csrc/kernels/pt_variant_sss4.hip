/* pt_variant_sss4.hip -- copy "sss4" of pt_copies.h: feature set "sss" held to a higher occupancy (TB_SSS_WAVES = 6 waves per SIMD, 80 VGPRs + scratch;
 * the file name dates from the 4-wave copy), lock-step only; chosen when that many workgroups per CU fit in LDS, deeper trees with the
 * last stack entries in global memory (split stack).
 * Waves per SIMD.  Round 3, when the walk loop still reloaded spilled values at every step: 3 / 4 / 5 / 6 waves = 1 102 / 1 211 / 1 316 /
 * 1 263 (bistro-class), - / 1 495 / 1 564 / 1 501 (van-class) Msamples/s.  Round 4, walk loops free of scratch (walk_owns, pt_device.hpp): 4 / 5 / 6 / 7 / 8
 * waves = 1 332 / 1 374 / 1 410 / 819 / 1 255 (bistro-class), 1 688 / 1 657 / 1 706 / 969 / 1 517 (van-class; 7 workgroups per CU do not divide the work
 * lists).  Experiments: -DTB_SSS_WAVES=n (scripts/build_sss_sweep.py, scripts/sss_waves_timing.sh); -DTB_SSS_STASH=n: an LDS stash of a path's cold
 * state like the env copy's (pt_variant_env5.hip). */
#define PT_COPY sss4
#include "pt_variant.inc"
