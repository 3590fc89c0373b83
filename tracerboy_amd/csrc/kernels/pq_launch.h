/* pq_launch.h -- the launchers of pq_kernels.hip: point queries on device buffers (include/tracerboy_hip.h tb_nearest_points,
 * tb_bake_distance_field; the rule: include/tb_nearest.h).
 *   pq_launch_nearest   one point per lane through the nearest-first walk of the layout-B tree in memory; a 32-B record per point
 *   pq_launch_field     the same walk over the cells of a grid, positions made from the cell number; 4 B per cell, the record's Distance
 * Every pointer is a device pointer, points and records 16-B aligned, distances 4-B.  n, and the grid's cells, <= 2^31.  One-level scenes only.
 * The stack is one dword per entry and lane in dynamic LDS, ds->stackDepth entries -- the FULL depth of the tree, as rq_launch_closest sizes it:
 * the split stack (stackOverflow) is not used, and a tree too deep for 160 KB of LDS (depth 160) is refused by the runtime.  One push per level is
 * the most the walk makes, so a walk holds at most stackDepth - 1 entries.  flags: TB_NEAREST_SIGNED alone.  The launchers know neither contexts
 * nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "pt_scene.h"

#define PQ_SIGNED 1u /* = TB_NEAREST_SIGNED */

extern "C" {
hipError_t pq_launch_nearest(hipStream_t stream, const TbDeviceScene* ds, uint32_t flags, uint32_t n, const TbQueryPoint* points, TbNearest* out);
hipError_t pq_launch_field(hipStream_t stream, const TbDeviceScene* ds, uint32_t flags, const tb_probe_grid* grid, float maxDistance, float* out);
}
