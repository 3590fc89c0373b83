/* pt_variant_vol4.hip -- copy "vol4" of pt_copies.h: feature set "vol" held to a higher occupancy (TB_VOL_WAVES = 4 waves per SIMD; the file name
 * dates from the 4-wave copy): chosen over pt_variant_vol.hip when that many workgroups per CU fit in LDS (split stack for deeper trees).
 * Waves per SIMD (128 VGPRs + scratch).  Round 4, walk loops free of scratch (walk_owns, pt_device.hpp), the reference's vw-van at 4K x 8: 4 / 5 / 6
 * waves = 1 824 / 1 617 / 1 582 Msamples/s flattened, 1 608 / 1 601 / 1 028 as a two-level scene (at 6 its 53-level tree leaves the tuned copy); 1080p
 * 1 379 / 1 266 / 1 243.  Experiments: -DTB_VOL_WAVES=n (scripts/ab_device_flags.sh); -DTB_VOL_STASH=n: an LDS stash of a path's cold state like the
 * env copy's (pt_variant_env5.hip). */
#define PT_COPY vol4
#include "pt_variant.inc"
