/* pt_variant_matte6.hip -- copy "matte6" of pt_copies.h: feature set "matte" at 6 waves per SIMD (80 VGPRs, 80 B of scratch, none of it inside the walk
 * loops), for scenes in LDS only: the frame-group kernels with the whole stack in LDS.  Chosen over the 5-wave copy (pt_variant_matte5.hip) when six
 * workgroups per CU fit (stack + the walk's LDS image <= 26 KB, launch_plan.h LdsCopyFits): cornell-box 1920x1080x64 7 136 -> 7 426 Msamples/s
 * (docs/experiments/r7.md).  Scenes fetched from memory keep the 5-wave copy.
 *
 * What this unit assumes of a launch (docs/experiments/r10.md): every index its kernels can form into the shading tables is in range -- the geometry
 * index and the primitive of every triangle record, the three vertices of its index triple, its hit group's material, and a light index below
 * numLights.  The host launches this copy only for a scene whose tables SceneTablesInRange (host/lds_image.h) has checked and a call whose LightCount
 * is at most numLights and below 2^23 (context_render.cpp pickCopy); any other runs the 5-wave copy, whose fetches are guarded. */
#define PT_COPY matte6
#define PT_TABLES_CHECKED 1 /* fetch_surface, load_vertex, fetch_material, fetch_light, shadow_hit_is_light fetch without a bounds check (pt_device.hpp) */
#define PT_SHADING_SHORT_FORMS 1 /* tb_sincos, x / PI without the division, reorient's zero component by a select (pt_device.hpp) */
#include "pt_variant.inc"
