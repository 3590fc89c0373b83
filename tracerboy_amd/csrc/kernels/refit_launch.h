/* refit_launch.h -- the launchers of refit_kernels.hip: moved vertices into a tree whose topology stands (include/tracerboy_hip.h
 * tb_commit_geometry).
 *   refit_launch_stage    a caller's xyz triples into a range of the staged position / normal array (device to device, on the stream)
 *   refit_launch_normals  staged normals of a vertex range into the Normal field of the vertex buffer's 32-B records
 *   refit_launch_face_vectors / refit_launch_vertex_normals  smooth normals of marked vertices made again from the positions (tb_recompute_normals)
 *   refit_launch_fit      the refit: one launch over the sorted triangles (new vertices, leaf boxes), then one launch per level of the precomputed
 *                         schedule, chained on the stream -- the few-node top levels optionally in one single-workgroup launch.  A lane reads only
 *                         what earlier launches, or earlier levels of its own workgroup, wrote; nothing comes back to the host.
 * Every pointer is a device pointer.  The launchers know neither contexts nor options. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "tb_abi.h"

/* The tables of a refit, made once per topology (host/context_dynamic.cpp).  A slot names where a box is stored: node * 2 + side of the layout-B node
 * that holds it as a child's box, REFIT_ROOT_SLOT for the root's own box (rootBox: centre xyz, half-extent xyz). */
#define REFIT_ROOT_SLOT 0xffffffffu
typedef struct RefitTables {
    const float* positions;     /* 3 floats per vertex: the staged positions */
    const uint32_t* triVerts;   /* 3 vertex numbers per sorted triangle */
    const uint32_t* triSlot;    /* per sorted triangle: the slot of its leaf box */
    const uint32_t* nodeSlot;   /* per layout-B node: the slot of its own box */
    const uint32_t* schedule;   /* node indices grouped by height, lowest first */
    TbTriB* tris; TbNodeB* nodes; float* rootBox;
    uint32_t numTris, numNodes;
} RefitTables;

/* The tables of a normal recomputation (tb_recompute_normals), made once per topology at the first call (host/context_dynamic.cpp makeNormalTables).
 * A face-vector slot is a triangle's number in geometry order.  Row v of the vertex -> corner table, slots[rowStart[v] .. rowStart[v + 1]), lists the
 * slots of the corners that name vertex v in exactly include/tb_normals.h's order; the rows of an emissive geometry's vertices are empty. */
typedef struct RefitNormalTables {
    const float* positions;     /* 3 floats per vertex: the staged positions, as the commit leaves them */
    const uint32_t* triVerts;   /* 3 absolute vertex numbers per triangle, geometry order */
    const uint32_t* rowStart;   /* numVertices + 1 offsets into slots */
    const uint32_t* slots;
    float* faceVectors;         /* 3 floats per triangle */
    float* vertexBuffer;        /* the scene's 32-B vertex records */
    uint32_t numTris, numVertices, numSlots;
} RefitNormalTables;

extern "C" {
/* every face vector; then the normals of the vertices firstVertex .. firstVertex + numVertices, which read them */
hipError_t refit_launch_face_vectors(hipStream_t stream, const RefitNormalTables* t);
hipError_t refit_launch_vertex_normals(hipStream_t stream, const RefitNormalTables* t, uint32_t firstVertex, uint32_t numVertices);
hipError_t refit_launch_stage(hipStream_t stream, float* staged, uint32_t firstVertex, uint32_t numVertices, const float* xyz);
hipError_t refit_launch_normals(hipStream_t stream, float* vertexBuffer, const float* staged, uint32_t firstVertex, uint32_t numVertices);
/* levelFirst: numLevels + 1 offsets into schedule (host memory), levelFirstDevice: the same on the device.  Levels [0, fusedFirstLevel) run one launch
 * each; levels [fusedFirstLevel, numLevels) run in one single-workgroup kernel with a barrier between them (fusedFirstLevel >= numLevels: none does).
 * refit_fused_first_level: the first level from which every level holds at most REFIT_FUSED_MAX_NODES nodes (numLevels where fewer than two do). */
#define REFIT_FUSED_MAX_NODES 1024u
uint32_t refit_fused_first_level(const uint32_t* levelFirst, uint32_t numLevels);
hipError_t refit_launch_fit(hipStream_t stream, const RefitTables* t, const uint32_t* levelFirst, uint32_t numLevels, const uint32_t* levelFirstDevice,
                            uint32_t fusedFirstLevel);
}
