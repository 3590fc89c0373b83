/* pt_variant_surf.hip -- copy "surf" of pt_copies.h: the one copy of feature set "surf" (pt_device_features.h).
 * Waves per SIMD it is held to.  Rounds 2-4 (max-ILP scheduler): Teapot 1080p x 16 at 3 / 4 / 5 / 6 waves = 3 140 / 3 007 /
 * 2 412 / 2 299 Msamples/s -- 3 it was.  Round 5: under the memory-clause scheduler (build.py TU_SCHEDULER: this unit and vol4) the
 * 4-wave copy (128 VGPRs) spills a fifth of what it did and wins: 3 / 4 / 5 waves = 3 005 / 3 110 / 2 609 (2 913 for the round-4 build on
 * the same box; scripts/ab_variants.sh, profiles/r5/ab_sched2.json, ab_sched3.json).  Experiments: -DTB_SURF_WAVES=n.
 * This feature set has no higher-occupancy copy: the primary-visibility pre-pass is compiled here (Teapot: env-lit, a large part of its rays are
 * camera rays). */
#define PT_COPY surf
#include "pt_variant.inc"
