/* refit_kernels.hip -- moved vertices into a tree whose topology stands.
 *
 * The arithmetic is the builder's fit pass (bvh_kernels.hip bvh_fit_leaves / bvh_fit_up), expression for expression, so a refit from the positions a
 * tree was built of gives back its bytes:
 *   leaf    mn = min(min(v0, v1), v2), mx = max(max(v0, v1), v2); mn = min(mn, mx - 0.001); c = (mn + mx) * 0.5; h = mx - c
 *   parent  from the children's STORED boxes: mn = min(lc - lh, rc - rh), mx = max(lc + lh, rc + rh), then the same c, h
 * A layout-B node holds its two children's boxes, so a node's own box is stored with its parent ("slot", refit_launch.h), the root's in rootBox.
 *
 * The builder does not know its topology while it runs and reads a progress word between wave-fronts; here the topology is known, and the host has
 * grouped the nodes by height once.  refit_fit_leaves writes every leaf box; launch h of refit_fit_level takes the nodes of height h, whose
 * children's boxes lie in their own record, written by earlier launches -- visible at the kernel boundary, with no fence, no counter, no waiting
 * workgroup and nothing read back.  One lane per node; nodes of one height never touch the same word. */
#include <hip/hip_runtime.h>
#include "tb_math.h"
#include "tb_vec.h"
#include "tb_normals.h"
#include "tb_abi.h"
#include "refit_launch.h"

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ void store_box(const RefitTables& t, uint32_t slot, tb3 mn, tb3 mx)
{
    const tb3 c = (mn + mx) * 0.5f, h = mx - c;
    if (slot == REFIT_ROOT_SLOT) { float* r = t.rootBox; r[0] = c.x; r[1] = c.y; r[2] = c.z; r[3] = h.x; r[4] = h.y; r[5] = h.z; return; }
    const uint32_t node = slot >> 1, s = slot & 1u;
    if (node >= t.numNodes) return;
    TbNodeB* n = t.nodes + node;
    n->cx[s] = c.x; n->cy[s] = c.y; n->cz[s] = c.z; n->hx[s] = h.x; n->hy[s] = h.y; n->hz[s] = h.z;
}

__global__ __launch_bounds__(BLOCK) void refit_fit_leaves(RefitTables t)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= t.numTris) return;
    const float* p0 = t.positions + 3ull * t.triVerts[3ull * k], * p1 = t.positions + 3ull * t.triVerts[3ull * k + 1],
        * p2 = t.positions + 3ull * t.triVerts[3ull * k + 2];
    const tb3 v0 = tb3_make(p0[0], p0[1], p0[2]), v1 = tb3_make(p1[0], p1[1], p1[2]), v2 = tb3_make(p2[0], p2[1], p2[2]);
    TbTriB* tri = t.tris + k; /* the metadata words stay */
    tri->v0[0] = v0.x; tri->v0[1] = v0.y; tri->v0[2] = v0.z;
    tri->v1[0] = v1.x; tri->v1[1] = v1.y; tri->v1[2] = v1.z;
    tri->v2[0] = v2.x; tri->v2[1] = v2.y; tri->v2[2] = v2.z;
    tb3 mn = tb3_min(tb3_min(v0, v1), v2), mx = tb3_max(tb3_max(v0, v1), v2);
    mn = tb3_min(mn, mx - tb3_splat(0.001f));
    store_box(t, t.triSlot[k], mn, mx);
}

__device__ __forceinline__ void fit_node(const RefitTables& t, uint32_t node)
{
    if (node >= t.numNodes) return;
    const TbNodeB n = t.nodes[node];
    const tb3 lcen = tb3_make(n.cx[0], n.cy[0], n.cz[0]), lhal = tb3_make(n.hx[0], n.hy[0], n.hz[0]);
    const tb3 rcen = tb3_make(n.cx[1], n.cy[1], n.cz[1]), rhal = tb3_make(n.hx[1], n.hy[1], n.hz[1]);
    const tb3 mn = tb3_min(lcen - lhal, rcen - rhal), mx = tb3_max(lcen + lhal, rcen + rhal);
    store_box(t, t.nodeSlot[node], mn, mx);
}

__global__ __launch_bounds__(BLOCK) void refit_fit_level(RefitTables t, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < count) fit_node(t, t.schedule[first + i]);
}

/* The few-node top levels in ONE workgroup: what a level stores, the next level's lanes of the same workgroup read after the barrier (__syncthreads is
 * a workgroup-scope release / acquire, and a workgroup's waves share their CU's L1); the levels below were written by earlier launches.  Bounded by
 * the levels of the schedule. */
__global__ __launch_bounds__(BLOCK) void refit_fit_top(RefitTables t, const uint32_t* levelFirst, uint32_t firstLevel, uint32_t numLevels)
{
    for (uint32_t l = firstLevel; l < numLevels; l++) {
        const uint32_t end = levelFirst[l + 1];
        for (uint32_t i = levelFirst[l] + threadIdx.x; i < end; i += BLOCK) fit_node(t, t.schedule[i]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(BLOCK) void refit_stage(float* staged, uint32_t firstVertex, uint32_t numVertices, const float* xyz)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= 3ull * numVertices) return;
    staged[3ull * firstVertex + i] = xyz[i];
}

__global__ __launch_bounds__(BLOCK) void refit_normals(float* vertexBuffer, const float* staged, uint32_t firstVertex, uint32_t numVertices)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= numVertices) return;
    const uint64_t v = (uint64_t)firstVertex + i;
    float* n = vertexBuffer + 8ull * v; /* TbVertex: Normal leads the record */
    n[0] = staged[3ull * v]; n[1] = staged[3ull * v + 1]; n[2] = staged[3ull * v + 2];
}

/* Smooth normals again from the positions as they stand (tb_recompute_normals; include/tb_normals.h states the rule, DESIGN.md section 24 the shape).
 * Two launches: every face vector once, 12 B per triangle, coalesced by triangle; then one lane per marked vertex walks its row of the vertex ->
 * corner table, which lists the face-vector slots of its corners in the rule's order (ascending primitive, corners 0, 1, 2), adds them in that order,
 * normalises and stores the Normal field.  The second launch reads what the first wrote: visible at the kernel boundary.  No atomics, no LDS, no fence;
 * every loop is bounded by the table, every index it forms is checked against the table's sizes.  An empty row (a vertex no triangle names, a vertex
 * of an emissive geometry) writes nothing. */
__global__ __launch_bounds__(BLOCK) void refit_face_vectors(RefitNormalTables t)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= t.numTris) return;
    const uint32_t i0 = t.triVerts[3ull * k], i1 = t.triVerts[3ull * k + 1], i2 = t.triVerts[3ull * k + 2];
    if (i0 >= t.numVertices || i1 >= t.numVertices || i2 >= t.numVertices) return;
    const float* p0 = t.positions + 3ull * i0, * p1 = t.positions + 3ull * i1, * p2 = t.positions + 3ull * i2;
    const tb3 f = tb_face_vector(tb3_make(p0[0], p0[1], p0[2]), tb3_make(p1[0], p1[1], p1[2]), tb3_make(p2[0], p2[1], p2[2]));
    float* o = t.faceVectors + 3ull * k;
    o[0] = f.x; o[1] = f.y; o[2] = f.z;
}

__global__ __launch_bounds__(BLOCK) void refit_vertex_normals(RefitNormalTables t, uint32_t firstVertex, uint32_t numVertices)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= numVertices) return;
    const uint64_t v = (uint64_t)firstVertex + i;
    if (v >= t.numVertices) return;
    const uint32_t begin = t.rowStart[v], rowEnd = t.rowStart[v + 1], end = rowEnd < t.numSlots ? rowEnd : t.numSlots;
    if (begin >= end) return;
    tb3 acc = tb3_splat(0.0f);
    for (uint32_t j = begin; j < end; j++) {
        const uint32_t slot = t.slots[j];
        if (slot >= t.numTris) continue;
        const float* f = t.faceVectors + 3ull * slot;
        acc = tb_normal_accumulate(acc, tb3_make(f[0], f[1], f[2]));
    }
    const tb3 n = tb_normal_finish(acc);
    float* o = t.vertexBuffer + 8ull * v; /* TbVertex: Normal leads the record */
    o[0] = n.x; o[1] = n.y; o[2] = n.z;
}

inline uint32_t blocksFor(uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }
/* hipGetLastError is sticky: an error an earlier call left unread (tb_sync asks never-recorded events for a time) is not this launch's */
inline void forgetEarlierErrors() { (void)hipGetLastError(); }

} // namespace

extern "C" hipError_t refit_launch_stage(hipStream_t stream, float* staged, uint32_t firstVertex, uint32_t numVertices, const float* xyz)
{
    if (!numVertices) return hipSuccess;
    forgetEarlierErrors();
    hipLaunchKernelGGL(refit_stage, dim3(blocksFor(3ull * numVertices)), dim3(BLOCK), 0, stream, staged, firstVertex, numVertices, xyz);
    return hipGetLastError();
}

extern "C" hipError_t refit_launch_normals(hipStream_t stream, float* vertexBuffer, const float* staged, uint32_t firstVertex, uint32_t numVertices)
{
    if (!numVertices) return hipSuccess;
    forgetEarlierErrors();
    hipLaunchKernelGGL(refit_normals, dim3(blocksFor(numVertices)), dim3(BLOCK), 0, stream, vertexBuffer, staged, firstVertex, numVertices);
    return hipGetLastError();
}

extern "C" hipError_t refit_launch_face_vectors(hipStream_t stream, const RefitNormalTables* t)
{
    if (!t->numTris) return hipSuccess;
    forgetEarlierErrors();
    hipLaunchKernelGGL(refit_face_vectors, dim3(blocksFor(t->numTris)), dim3(BLOCK), 0, stream, *t);
    return hipGetLastError();
}

extern "C" hipError_t refit_launch_vertex_normals(hipStream_t stream, const RefitNormalTables* t, uint32_t firstVertex, uint32_t numVertices)
{
    if (!numVertices) return hipSuccess;
    forgetEarlierErrors();
    hipLaunchKernelGGL(refit_vertex_normals, dim3(blocksFor(numVertices)), dim3(BLOCK), 0, stream, *t, firstVertex, numVertices);
    return hipGetLastError();
}

extern "C" uint32_t refit_fused_first_level(const uint32_t* levelFirst, uint32_t numLevels)
{
    uint32_t first = numLevels;
    while (first > 0 && levelFirst[first] - levelFirst[first - 1] <= REFIT_FUSED_MAX_NODES) first--;
    return numLevels - first >= 2 ? first : numLevels; /* one level alone is the chain's own launch */
}

extern "C" hipError_t refit_launch_fit(hipStream_t stream, const RefitTables* t, const uint32_t* levelFirst, uint32_t numLevels, const uint32_t* levelFirstDevice,
    uint32_t fusedFirstLevel)
{
    if (!t->numTris) return hipSuccess;
    forgetEarlierErrors();
    hipLaunchKernelGGL(refit_fit_leaves, dim3(blocksFor(t->numTris)), dim3(BLOCK), 0, stream, *t);
    const uint32_t chained = fusedFirstLevel < numLevels ? fusedFirstLevel : numLevels;
    for (uint32_t l = 0; l < chained; l++) {
        const uint32_t first = levelFirst[l], count = levelFirst[l + 1] - first;
        if (!count) continue;
        hipLaunchKernelGGL(refit_fit_level, dim3(blocksFor(count)), dim3(BLOCK), 0, stream, *t, first, count);
    }
    if (chained < numLevels) hipLaunchKernelGGL(refit_fit_top, dim3(1), dim3(BLOCK), 0, stream, *t, levelFirstDevice, chained, numLevels);
    return hipGetLastError();
}
