/* rq_kernels.hip -- ray queries on device buffers (include/tracerboy_hip.h tb_trace_rays): a caller's rays through the
 * renderer's traversal, hit records or occlusion flags out.
 *
 * rq_closest_kernel: trace_closest_kernel's walks (pt_kernels.hip) -- traverse<true, true> / traverse_instanced<true, true>, the scene fetched from
 * memory, fetch_surface on a hit -- on 32-B ray records in and 48-B hit records out, one ray per lane.  The walk itself does not know the ray's
 * range: the closest hit inside (MIN_T, TMax) exists iff the overall closest hit lies inside it, and is that hit, so the record is kept iff
 * t < TMax and every field has tb_trace_closest's bits.  RECORDS = false writes that comparison alone, one byte per ray: occluded mode of
 * two-level scenes, and the side the any-hit walk is measured against.
 *
 * rq_occluded_kernel: the any-hit walk of one-level scenes.  traverse()'s pieces -- ray_cannot_hit, ray_prepare, the root box, box_test2,
 * load_node, load_tri, tri_test<ALPHA>, the per-lane LDS stack, the parking rule -- with `closest` held at min(TMax, MAX_T): tri_test accepts
 * t > MIN_T && t < closest (and, under option alpha_test, IsValidHit), and the first accepted candidate ends the ray.  Rays of one wave then end
 * many steps apart -- one at its first leaf, its neighbour after the whole tree.  Two forms, chosen by the launcher's caller (rq_launch.h
 * rq_refill_for has the measurements' rule):
 *   REFILL = false  one ray per lane, a wave leaves when its 64 rays are done: the faster form on small trees and on coherent rays;
 *   REFILL = true   a persistent grid that refills at the wave level: when refillMin lanes of a wave are idle, they take consecutive ray indices,
 *                   by their rank among the idle lanes, from the wave's pool -- RQ_CHUNK indices that lane 0 claims from *counter with one atomic
 *                   add whenever the pool is empty (one add per ray batch of 64 saturated the counter's one address: 4.8 Grays/s whatever the
 *                   scene).  A wave leaves once the counter has passed n, its pool is empty and none of its lanes is live.
 * No wave waits for another; every loop is bounded by n and by the tree, and is left on wave-uniform conditions (ballots), as the walk steps of
 * docs/experiments/r9.md are.  A ray's answer does not depend on which lane walks it or when: it is written by index, one byte. */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"
#include "rq_launch.h"

namespace {

struct RqRay { tb3 o, d; float tMax; uint32_t flags; };
__device__ __forceinline__ RqRay rq_load_ray(const TbQueryRay* rays, uint32_t i) /* 32 B, 16-B aligned: two 16-B loads */
{
    const uint4* p = (const uint4*)(rays + i);
    const uint4 a = p[0], b = p[1];
    RqRay q;
    q.o = tb3_make(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)); q.tMax = __uint_as_float(a.w);
    q.d = tb3_make(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)); q.flags = b.w;
    return q;
}
/* what is traced at all: not a disabled ray, not a TMax that is a NaN or leaves no room above MIN_T */
__device__ __forceinline__ bool rq_traced(const RqRay& q) { return !(q.flags & TB_QUERY_RAY_DISABLED) && q.tMax > MIN_T; }

template <bool RECORDS>
__global__ __launch_bounds__(BLOCK) void rq_closest_kernel(TbDeviceScene ds, uint32_t n, const TbQueryRay* __restrict__ rays, TbQueryHit* __restrict__ hits,
    uint8_t* __restrict__ occluded)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* stack = (uint32_t*)smem + threadIdx.x;
    SceneRefs sc; make_refs<false>(sc, ds, nullptr);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const RqRay q = rq_load_ray(rays, i);
    Hit h; uint32_t nb = 0, nt = 0;
    bool hit = false;
    if (rq_traced(q)) {
        hit = ds.numInstances ? traverse_instanced<true, true>(sc, ds, q.o, q.d, h, stack, BLOCK, nb, nt) : traverse<true, true>(sc, ds, q.o, q.d, h, stack,
            BLOCK, nb, nt);
        hit = hit && h.t < q.tMax;
    }
    if (!RECORDS) { occluded[i] = hit ? 1 : 0; return; }
    Surface s; s.normal = tb3_splat(0.0f); s.u = s.v = 0.0f; s.material = -1;
    if (hit) fetch_surface(sc, h, s, false);
    uint4* o = (uint4*)(hits + i); /* 48 B, 16-B aligned: three 16-B stores */
    o[0] = make_uint4(__float_as_uint(hit ? h.t : -1.0f), __float_as_uint(hit ? h.u : 0.0f), __float_as_uint(hit ? h.v : 0.0f), hit ? h.prim : 0xffffffffu);
    o[1] = make_uint4(hit ? h.geom : 0xffffffffu, (uint32_t)s.material, __float_as_uint(s.u), __float_as_uint(s.v));
    o[2] = make_uint4(__float_as_uint(s.normal.x), __float_as_uint(s.normal.y), __float_as_uint(s.normal.z), 0u);
}

template <bool ALPHA, bool REFILL>
__global__ __launch_bounds__(BLOCK) void rq_occluded_kernel(TbDeviceScene ds, uint32_t n, const TbQueryRay* __restrict__ rays, uint8_t* __restrict__ occluded,
    uint32_t* counter, uint32_t refillMin)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* const stack = (uint32_t*)smem + threadIdx.x;
    SceneRefs sc; make_refs<false>(sc, ds, nullptr);
    constexpr uint32_t DONE = 0xffffffffu; /* an idle lane: has the leaf bit, so it takes no inner-node step either */
    const uint32_t lane = threadIdx.x & 63u;
    const int parkMin = (int)ds.parkMin > 1 ? (int)ds.parkMin : 1;
    uint32_t ref = DONE, top = 0, index = 0;
    float tMax = 0.0f;
    RayPre r{};
    /* a lane whose stack is empty has found nothing */
    auto pop = [&]() -> uint32_t {
        if (!top) { occluded[index] = 0; return DONE; }
        --top;
        return stack[top * BLOCK];
    };
    auto begin = [&](uint32_t i) {
        const RqRay q = rq_load_ray(rays, i);
        index = i;
        bool go = rq_traced(q) && !ray_cannot_hit(q.o, q.d);
        if (go) {
            tMax = q.tMax < MAX_T ? q.tMax : MAX_T;
            r = ray_prepare(q.o, q.d);
            float unusedT;
            go = box_test(unusedT, tMax, r, ld3(ds.rootCenter), ld3(ds.rootHalf));
        }
        if (go) { ref = ds.rootRef; top = 0; }
        else occluded[i] = 0;
    };
    /* wave-uniform: the wave's pool of claimed indices; dry: the counter has passed n, this wave claims no more */
    uint32_t poolNext = 0, poolEnd = 0;
    bool dry = !REFILL;
    if (!REFILL) { const uint32_t i = blockIdx.x * BLOCK + threadIdx.x; if (i < n) begin(i); }
    for (;;) {
        if (REFILL) {
            const unsigned long long idle = __ballot(ref == DONE);
            const uint32_t want = (uint32_t)__popcll(idle);
            if ((!dry || poolNext != poolEnd) && want >= refillMin) {
                if (poolNext == poolEnd) { /* (then not dry) */
                    uint32_t base = 0;
                    if (lane == 0) base = __hip_atomic_fetch_add(counter, RQ_CHUNK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    base = __builtin_amdgcn_readfirstlane(base); /* n <= 2^31 and every wave overshoots once, by one chunk: no wrap */
                    poolNext = base < n ? base : n; poolEnd = base + RQ_CHUNK < n ? base + RQ_CHUNK : n;
                    dry = base + RQ_CHUNK >= n;
                }
                const uint32_t i = poolNext + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                if (ref == DONE && i < poolEnd) begin(i);
                poolNext = poolNext + want < poolEnd ? poolNext + want : poolEnd;
            }
        }
        unsigned long long inner = __ballot(!(ref & TB_BVH_LEAF_FLAG));
        const unsigned long long atLeaf = __ballot(ref != DONE && (ref & TB_BVH_LEAF_FLAG));
        if ((inner | atLeaf) == 0ull) { /* nobody walks: every ray drawn ended where it began, or none was left to draw */
            if (dry && poolNext == poolEnd) break;
            continue;
        }
        if (inner != 0ull) {
            do {
                if (!(ref & TB_BVH_LEAF_FLAG)) {
                    const TbNodeB nd = load_node(sc, ref);
                    float lt, rt; bool lh, rh;
                    box_test2(lh, rh, lt, rt, tMax, r, nd);
                    if (lh && rh) {
                        const bool rightFirst = rt < lt;
                        stack[top * BLOCK] = rightFirst ? nd.left : nd.right;
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
            Hit best; best.t = tMax; best.u = best.v = 0.0f; best.prim = best.geom = 0u;
            tri_test<ALPHA>(best, MIN_T, r.o, r, tri, false, sc, ds);
            if (best.t < tMax) { occluded[index] = 1; ref = DONE; } /* the first accepted candidate ends the ray */
            else ref = pop();
        }
    }
}

size_t rq_stack_lds(const TbDeviceScene& ds) { return (size_t)ds.stackDepth * BLOCK * 4; }
bool rq_aligned16(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }

template <class K> hipError_t rq_launch_any_hit(K kernel, hipStream_t stream, const TbDeviceScene& ds, uint32_t n, const TbQueryRay* rays, uint8_t* occluded,
    uint32_t* counter, uint32_t refillMin)
{
    const size_t lds = rq_stack_lds(ds);
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    uint64_t blocks = ((uint64_t)n + BLOCK - 1) / BLOCK; /* one ray per lane */
    if (refillMin) {
        int numCUs = 0, perCU = 0;
        e = pt_device_cus(&numCUs); if (e != hipSuccess) return e;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, BLOCK, lds); if (e != hipSuccess) return e;
        /* about the workgroups the device holds at once (capped at 8 per CU like the other resident grids), and no more waves than pools; nothing
         * waits for a workgroup, so a count that is one too high only queues it */
        const uint64_t resident = (uint64_t)(perCU > 0 ? (perCU > 8 ? 8 : perCU) : 1) * (uint64_t)(numCUs > 0 ? numCUs : 1);
        const uint64_t pools = ((uint64_t)n + 4u * RQ_CHUNK - 1) / (4u * RQ_CHUNK);
        blocks = pools < resident ? pools : resident;
        e = hipMemsetAsync(counter, 0, 4, stream); if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(BLOCK), lds, stream, ds, n, rays, occluded, counter, refillMin);
    return hipGetLastError();
}

} // namespace

extern "C" hipError_t rq_launch_closest(hipStream_t stream, const TbDeviceScene* ds, uint32_t n, const TbQueryRay* rays, TbQueryHit* hits, uint8_t* occluded)
{
    if (!ds || !n || n > 0x80000000u || !rq_aligned16(rays) || (hits ? !rq_aligned16(hits) || occluded : !occluded)) return hipErrorInvalidValue;
    TbDeviceScene scene = *ds; scene.nodesC = nullptr; /* layout B */
    const size_t lds = rq_stack_lds(scene);
    const void* fn = hits ? (const void*)rq_closest_kernel<true> : (const void*)rq_closest_kernel<false>;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    const dim3 grid((uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK));
    if (hits) hipLaunchKernelGGL(rq_closest_kernel<true>, grid, dim3(BLOCK), lds, stream, scene, n, rays, hits, occluded);
    else hipLaunchKernelGGL(rq_closest_kernel<false>, grid, dim3(BLOCK), lds, stream, scene, n, rays, hits, occluded);
    return hipGetLastError();
}

extern "C" hipError_t rq_launch_occluded(hipStream_t stream, const TbDeviceScene* ds, uint32_t n, const TbQueryRay* rays, uint8_t* occluded, uint32_t* counter,
    uint32_t refillMin)
{
    if (!ds || !n || n > 0x80000000u || !rq_aligned16(rays) || !occluded || (refillMin && !counter) || refillMin > 64u) return hipErrorInvalidValue;
    if (ds->numInstances) return hipErrorInvalidValue; /* the any-hit walk is the one-level walk */
    TbDeviceScene scene = *ds; scene.nodesC = nullptr; /* layout B */
    if (!refillMin) return scene.alphaTest ? rq_launch_any_hit(rq_occluded_kernel<true, false>, stream, scene, n, rays, occluded, counter, 0u)
                                           : rq_launch_any_hit(rq_occluded_kernel<false, false>, stream, scene, n, rays, occluded, counter, 0u);
    return scene.alphaTest ? rq_launch_any_hit(rq_occluded_kernel<true, true>, stream, scene, n, rays, occluded, counter, refillMin)
                           : rq_launch_any_hit(rq_occluded_kernel<false, true>, stream, scene, n, rays, occluded, counter, refillMin);
}
