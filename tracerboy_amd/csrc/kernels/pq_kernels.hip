/* pq_kernels.hip -- point queries on device buffers (include/tracerboy_hip.h tb_nearest_points, tb_bake_distance_field): for
 * every point the nearest point of the scene's triangles, by the rule of include/tb_nearest.h -- which the host states with the same functions
 * (host_api.cpp tb_host_scene_nearest), so the records agree on bits.
 *
 * pq_nearest_kernel: one point per lane, a nearest-first walk of the layout-B tree in memory with a shrinking bound.  At an inner node
 * (load_node: four 16-B loads) tb_box_d2 of both children; the lane descends into the nearer child and pushes the farther one iff its bound does
 * not exceed `cull`, tb_nearest_cull of min(limit, best D2 so far) -- the rule's conservative culling value, made again only when the best
 * improves.  At a leaf (load_tri: three 16-B loads; TbTriB carries the corners, no index or vertex buffer is read) tb_nearest_on_triangle and the
 * candidate rule with its tie-break.  The stack is per lane in dynamic LDS, one dword per entry: the ref alone.  An entry popped after the best
 * has improved is judged against the cull of the moment by what it is: an inner node's children meet the current value, a leaf's triangle the
 * candidate rule -- a stale leaf costs one triangle test, a stale inner node one node fetch.  (The other form, the bound stored beside the ref,
 * would skip those at twice the LDS.)
 * RECORDS: a 32-B record per point (two 16-B stores) or its Distance alone (4 B, consecutive lanes consecutive cells).  GRID: the point is a
 * 16-B load, or made from the cell number: cell (i, j, k) at origin + (i, j, k) * spacing, i fastest.  TB_NEAREST_SIGNED is a run-time bit.
 * No wave waits for another; every loop is bounded by n and by the tree, and is left on wave-uniform conditions (ballots), as rq_occluded_kernel's
 * are: the inner-node loop runs while at least parkMin lanes descend.  A point's answer does not depend on which lane walks it or when. */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pq_launch.h"
#include "../../../include/tb_nearest.h"

/* Measurement build (scripts/build_variant.py --flags -DTB_PQ_STACK_BOUNDS=1 --tus kernels/pq_kernels.hip; never shipped): the other form of the
 * stack, the far child's bound beside its ref -- two dwords per entry, twice the LDS -- and an entry whose bound exceeds the cull of the moment
 * dropped at the pop instead of fetched.  Same records; DESIGN.md section 27 has both forms' rates. */
#ifndef TB_PQ_STACK_BOUNDS
#define TB_PQ_STACK_BOUNDS 0
#endif

namespace {

constexpr uint32_t PQ_ENTRY = TB_PQ_STACK_BOUNDS ? 2u : 1u; /* dwords per stack entry */

template <bool RECORDS, bool GRID>
__global__ __launch_bounds__(BLOCK) void pq_nearest_kernel(TbDeviceScene ds, uint32_t flags, uint32_t n, const TbQueryPoint* __restrict__ points, tb_probe_grid grid,
    float maxDistance, TbNearest* __restrict__ records, float* __restrict__ distances)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* const stack = (uint32_t*)smem + threadIdx.x;
    SceneRefs sc; make_refs<false>(sc, ds, nullptr);
    constexpr uint32_t DONE = 0xffffffffu; /* an idle lane: has the leaf bit, so it takes no inner-node step either */
    const int parkMin = (int)ds.parkMin > 1 ? (int)ds.parkMin : 1;
    const uint32_t index = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t ref = DONE, top = 0;
    tb3 p = tb3_splat(0.0f);
    float limit = -1.0f, slack = 0.0f, cull = 0.0f;
    float bestD2 = tb_u2f(0x7f800000u), bestU = 0.0f, bestV = 0.0f;
    uint32_t bestGeom = TB_NEAREST_NONE, bestPrim = TB_NEAREST_NONE;
    tb3 bestPoint = tb3_splat(0.0f);
    bool behind = false;
    if (index < n) {
        float maxD = maxDistance;
        if (GRID) {
            const uint32_t ci = index % grid.count[0], rest = index / grid.count[0], cj = rest % grid.count[1], ck = rest / grid.count[1];
            p = ld3(grid.origin) + tb3_make((float)ci, (float)cj, (float)ck) * ld3(grid.spacing);
        } else {
            const uint4 a = *(const uint4*)(points + index); /* 16 B, 16-B aligned: one load */
            p = tb3_make(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)); maxD = __uint_as_float(a.w);
        }
        limit = tb_nearest_limit(maxD);
        if (tb_nearest_finite3(p) && limit >= 0.0f) {
            const tb3 rc = ld3(ds.rootCenter), rh = ld3(ds.rootHalf);
            slack = tb_nearest_slack(tb_nearest_scale(p, rc, rh));
            cull = tb_nearest_cull(limit, slack);
            if (!(tb_box_d2(p, rc, rh) > cull)) ref = ds.rootRef; /* a point farther from the root box than it may look leaves at once */
        }
    }
    auto pop = [&]() -> uint32_t {
        while (top) {
            --top;
            if (!TB_PQ_STACK_BOUNDS || !(__uint_as_float(stack[(top * PQ_ENTRY + 1u) * BLOCK]) > cull)) return stack[top * PQ_ENTRY * BLOCK];
        }
        return DONE;
    };
    for (;;) {
        unsigned long long inner = __ballot(!(ref & TB_BVH_LEAF_FLAG));
        const unsigned long long atLeaf = __ballot(ref != DONE && (ref & TB_BVH_LEAF_FLAG));
        if ((inner | atLeaf) == 0ull) break;
        if (inner != 0ull) {
            do {
                if (!(ref & TB_BVH_LEAF_FLAG)) {
                    const TbNodeB nd = load_node(sc, ref);
                    const float dl = tb_box_d2(p, tb3_make(nd.cx[0], nd.cy[0], nd.cz[0]), tb3_make(nd.hx[0], nd.hy[0], nd.hz[0]));
                    const float dr = tb_box_d2(p, tb3_make(nd.cx[1], nd.cy[1], nd.cz[1]), tb3_make(nd.hx[1], nd.hy[1], nd.hz[1]));
                    const bool lh = !(dl > cull), rh = !(dr > cull);
                    if (lh && rh) {
                        const bool rightFirst = dr < dl;
                        stack[top * PQ_ENTRY * BLOCK] = rightFirst ? nd.left : nd.right;
                        if (TB_PQ_STACK_BOUNDS) stack[(top * PQ_ENTRY + 1u) * BLOCK] = __float_as_uint(rightFirst ? dl : dr);
                        top++;
                        ref = rightFirst ? nd.right : nd.left;
                    } else if (lh || rh) ref = rh ? nd.right : nd.left;
                    else ref = pop();
                }
                inner = __ballot(!(ref & TB_BVH_LEAF_FLAG));
            } while (__popcll(inner) >= parkMin);
        }
        if (ref != DONE && (ref & TB_BVH_LEAF_FLAG)) {
            const TbTriB tri = load_tri(sc, ref);
            const tb3 v0 = ld3(tri.v0), v1 = ld3(tri.v1), v2 = ld3(tri.v2);
            const TbNearestOnTriangle r = tb_nearest_on_triangle(p, v0, v1, v2);
            if (r.D2 <= limit && tb_nearest_better(r.D2, tri.geometryIndex, tri.primitiveIndex, bestD2, bestGeom, bestPrim)) {
                bestD2 = r.D2; bestGeom = tri.geometryIndex; bestPrim = tri.primitiveIndex; bestU = r.U; bestV = r.V; bestPoint = r.Point;
                behind = tb_nearest_behind(p, r.Point, v0, v1, v2);
                cull = tb_nearest_cull(bestD2, slack);
            }
            ref = pop();
        }
    }
    if (index >= n) return;
    const bool found = !(bestGeom == TB_NEAREST_NONE && bestPrim == TB_NEAREST_NONE);
    const float d = tb_sqrt(bestD2);
    const float distance = found ? (((flags & PQ_SIGNED) && behind) ? -d : d) : tb_u2f(0x7f800000u);
    if (!RECORDS) { distances[index] = distance; return; }
    uint4* o = (uint4*)(records + index); /* 32 B, 16-B aligned: two 16-B stores */
    o[0] = make_uint4(__float_as_uint(found ? bestPoint.x : 0.0f), __float_as_uint(found ? bestPoint.y : 0.0f), __float_as_uint(found ? bestPoint.z : 0.0f),
        __float_as_uint(distance));
    o[1] = make_uint4(__float_as_uint(found ? bestU : 0.0f), __float_as_uint(found ? bestV : 0.0f), bestPrim, bestGeom);
}

bool pq_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1u)) == 0; }

template <class K> hipError_t pq_launch(K kernel, hipStream_t stream, const TbDeviceScene* ds, uint32_t flags, uint32_t n, const TbQueryPoint* points,
    const tb_probe_grid& grid, float maxDistance, TbNearest* records, float* distances)
{
    if (!ds || !n || n > 0x80000000u || ds->numInstances || !ds->numTris || (flags & ~PQ_SIGNED)) return hipErrorInvalidValue;
    TbDeviceScene scene = *ds; scene.nodesC = nullptr; scene.stackOverflow = nullptr; scene.stackOverflowLanes = 0; /* layout B, the whole stack in LDS */
    const size_t lds = (size_t)scene.stackDepth * BLOCK * 4 * PQ_ENTRY;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    const dim3 blocks((uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK));
    hipLaunchKernelGGL(kernel, blocks, dim3(BLOCK), lds, stream, scene, flags, n, points, grid, maxDistance, records, distances);
    return hipGetLastError();
}

} // namespace

extern "C" hipError_t pq_launch_nearest(hipStream_t stream, const TbDeviceScene* ds, uint32_t flags, uint32_t n, const TbQueryPoint* points, TbNearest* out)
{
    if (!pq_aligned(points, 16) || !pq_aligned(out, 16)) return hipErrorInvalidValue;
    return pq_launch(pq_nearest_kernel<true, false>, stream, ds, flags, n, points, tb_probe_grid{}, 0.0f, out, nullptr);
}

extern "C" hipError_t pq_launch_field(hipStream_t stream, const TbDeviceScene* ds, uint32_t flags, const tb_probe_grid* grid, float maxDistance, float* out)
{
    if (!grid || !pq_aligned(out, 4) || !grid->count[0] || !grid->count[1] || !grid->count[2]) return hipErrorInvalidValue;
    const uint64_t plane = (uint64_t)grid->count[0] * grid->count[1], cells = plane * grid->count[2];
    if (plane > 0x80000000ull || cells > 0x80000000ull) return hipErrorInvalidValue;
    return pq_launch(pq_nearest_kernel<false, true>, stream, ds, flags, (uint32_t)cells, nullptr, *grid, maxDistance, nullptr, out);
}
