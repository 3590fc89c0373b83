/* wn_launch.h -- the launchers of wn_kernels.hip: generalized winding numbers on device buffers (include/tracerboy_hip.h
 * tb_winding_numbers .. tb_bake_distance_field_winding; the rule: include/tb_winding.h).
 *   wn_launch_fit     the moments of every subtree: one launch over the sorted triangles (the TbTriB corners as the last refit left them), then one
 *                     launch per level of the refit's schedule, chained on the stream -- the few-node top levels in one single-workgroup launch, as
 *                     refit_launch_fit runs them.  A lane reads only what earlier launches, or earlier levels of its own workgroup, wrote.
 *   wn_launch_points  one point per lane through the depth-first walk of the moment records; WN_WRITE: 4 B per point, w; WN_SIGN_RECORDS: the
 *                     Distance of the point's TbNearest record negated in place where the record is a hit and tb_winding_inside(w)
 *   wn_launch_grid    the same walk over the cells of a grid, positions made from the cell number as pq_launch_field makes them; WN_WRITE: w per
 *                     cell; WN_SIGN_CELLS: the cell's distance negated in place where it is not +inf and tb_winding_inside(w)
 * Every pointer is a device pointer, points and records 16-B aligned, floats 4-B.  n, and the grid's cells, <= 2^31.  One-level scenes only.  The
 * stack is one dword per entry and lane in dynamic LDS, ds->stackDepth entries, as pq_launch sizes it: the walk pushes at most one entry per level.
 * The launchers know neither contexts nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "pt_scene.h"

/* The moments of a layout-B node's two children, interleaved like TbNodeB's boxes: four 16-B loads.  left / right: the node's device child refs. */
typedef struct TbMomentsB { float Nx[2], Ny[2], Nz[2], cx[2], cy[2], cz[2], r[2]; uint32_t left, right; } TbMomentsB;
TB_STATIC_ASSERT(sizeof(TbMomentsB) == 64, "a moment record is 64 B");

/* The tables of a fit.  A slot names where a subtree's moments are stored: node * 2 + side of the record that holds them as a child's, WN_ROOT_SLOT for
 * the root's own (root: N xyz, centre xyz, radius, area).  triSlot, nodeSlot, schedule: the refit's (refit_launch.h RefitTables). */
#define WN_ROOT_SLOT 0xffffffffu
typedef struct WnTables {
    const uint32_t* triSlot; const uint32_t* nodeSlot; const uint32_t* schedule;
    const TbTriB* tris; const TbNodeB* nodes;   /* the scene's: corners, device child refs */
    TbMomentsB* moments; float* areas;          /* areas: one float per slot, read by the fit alone */
    float* root;                                /* 8 floats */
    uint32_t numTris, numNodes;
} WnTables;

#define WN_WRITE 0
#define WN_SIGN_RECORDS 1
#define WN_SIGN_CELLS 2

extern "C" {
/* levelFirst, levelFirstDevice, fusedFirstLevel: as refit_launch_fit's */
hipError_t wn_launch_fit(hipStream_t stream, const WnTables* t, const uint32_t* levelFirst, uint32_t numLevels, const uint32_t* levelFirstDevice,
                         uint32_t fusedFirstLevel);
hipError_t wn_launch_points(hipStream_t stream, const TbDeviceScene* ds, const TbMomentsB* moments, const float* root, int mode, uint32_t n,
                            const TbQueryPoint* points, float beta, void* out);
hipError_t wn_launch_grid(hipStream_t stream, const TbDeviceScene* ds, const TbMomentsB* moments, const float* root, int mode, const tb_probe_grid* grid,
                          float beta, float* out);
}
