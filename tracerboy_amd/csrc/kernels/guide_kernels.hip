/* guide_kernels.hip -- the guide pass of a still's denoise (include/tracerboy_hip.h tb_render_guides).
 *
 * A sample's seed depends on (x, y, frame) alone, so the first bounce of any frame can be traced again after a render that ran at full speed.
 * pt_guides walks pt_first's sequence (pt_persistent.inc) for the full feature set with FEAT_EXT -- path_begin, the closest-hit walk,
 * path_on_closest, path_scatter -- and keeps the AOV side channel of Path instead of a hand-over record: after the sequence aovNormal, aovAlbedo,
 * aovWorldPos and aovNeighbor hold what the lock-step kernel of an AOV render writes for that frame (pt_persistent.inc, the stores behind
 * `if (F & FEAT_EXT)`).  The feeler of the first hit is not walked: judging it adds to L, counts a GetMaterial call and -- with mix materials --
 * draws one random number, and path_scatter takes nothing from the random stream into the AOVs (the albedo is stored by every bounce that is not an
 * interior walk, whatever direction it sampled), so the feeler's walk cannot reach a guide.
 *
 * Shape: a workgroup of 256 owns one 16 x 16 region (block_region, pt_first's lane mapping) for ALL frames of the pass; each lane loops over the
 * frames in ascending order with its three sums in registers and writes them once.  No atomics, no cleared buffers; the grid strides over the
 * regions.  Traversal stack in LDS, [entry][lane], with the global overflow of the HYBRID form where the tree is deeper than the LDS share
 * (guide_launch.h). */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"
#include "guide_launch.h"

namespace {

/* 170 / 172 registers as written: held to three waves per SIMD, two registers away, like the lock-step copy of the same feature set (pt_copies.h
 * row `full`) -- 168 registers, 4-5 of them in scratch.  -DTB_GUIDES_WAVES=0 leaves the kernel as the compiler makes it (two waves, nothing
 * spilled): the other side of scripts/still_guides_waves_ab.py, whose figures are in DESIGN.md section 13. */
#ifndef TB_GUIDES_WAVES
#define TB_GUIDES_WAVES 3
#endif
#if TB_GUIDES_WAVES > 0
#define PT_GUIDES_ATTR __attribute__((amdgpu_waves_per_eu(TB_GUIDES_WAVES)))
#else
#define PT_GUIDES_ATTR
#endif
template <bool HYBRID>
__global__ __launch_bounds__(BLOCK) PT_GUIDES_ATTR void pt_guides(TbDeviceScene ds, TbPerFrameConstants pf, TbDeviceTargets tg, uint32_t W, uint32_t H, uint32_t firstFrame,
    uint32_t numFrames, TbTileMap tiles, TbFloat4* __restrict__ gAlbedo, TbFloat4* __restrict__ gNormal, TbFloat4* __restrict__ gPosition)
{
    constexpr uint32_t F = FEAT_ALL; /* what settingsFeatureMask(..., aov = true) selects: every scene the AOV path renders */
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SceneRefs sc;
    make_refs<false>(sc, ds, nullptr);
    uint32_t* stack = (uint32_t*)smem + threadIdx.x;
    uint32_t* const overflow = HYBRID ? ds.stackOverflow + (size_t)blockIdx.x * BLOCK + threadIdx.x : nullptr;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t regions = tb_persistent_grid(W, H, tiles);
    for (uint32_t region = blockIdx.x; region < regions; region += gridDim.x) {
        uint32_t bx, by;
        block_region(tiles, W, H, region, bx, by);
        const uint32_t x = bx * 16u + (wave & 1u) * 8u + (lane & 7u), y = by * 16u + (wave >> 1) * 8u + (lane >> 3);
        if (x >= W || y >= H) continue;
        TbFloat4 sa{0.0f, 0.0f, 0.0f, 0.0f}, sn{0.0f, 0.0f, 0.0f, 0.0f}, sp{0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t f = 0; f < numFrames; f++) {
            Path p;
            path_begin<F>(p, ds, pf, firstFrame + f, W, H, x, y, &tg);
            if (p.state == ST_EXTEND) {
                Hit h; uint32_t nb = 0, nt = 0;
                bool isHit;
                /* the walks of the full feature set: two levels where the scene has instances, the IsValidHit filter compiled in (ds.alphaTest) */
                if (ds.numInstances) isHit = traverse_instanced<false, true, HYBRID>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, overflow);
                else isHit = traverse<false, true, HYBRID, false, false, true>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, nullptr, overflow);
                path_on_closest<F>(p, sc, ds, pf, isHit, h);
                if (p.state == ST_SHADOW) p.state = ST_SCATTER; /* the feeler: not walked, see above */
                if (p.state == ST_SCATTER) path_scatter<F>(p, pf);
            }
            const tb3 n = p.aovNormal, a = p.aovAlbedo;
            const bool hit = n.x != 0.0f || n.y != 0.0f || n.z != 0.0f, lit = a.x != 0.0f || a.y != 0.0f || a.z != 0.0f;
            /* a miss, a light, a path that ended before it stored its albedo: the effective albedo is 1 */
            sa.x = sa.x + (lit ? a.x : 1.0f); sa.y = sa.y + (lit ? a.y : 1.0f); sa.z = sa.z + (lit ? a.z : 1.0f); sa.w = sa.w + 1.0f;
            if (hit) {
                sn.x = sn.x + n.x; sn.y = sn.y + n.y; sn.z = sn.z + n.z; sn.w = sn.w + 1.0f;
                sp.x = sp.x + p.aovWorldPos.x; sp.y = sp.y + p.aovWorldPos.y; sp.z = sp.z + p.aovWorldPos.z; sp.w = sp.w + p.aovNeighbor;
            }
        }
        const size_t pix = (size_t)y * W + x;
        gAlbedo[pix] = sa; gNormal[pix] = sn; gPosition[pix] = sp;
    }
}

bool guide_surface(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }
size_t guide_lds(const GuidePlan& plan) { return (size_t)plan.ldsEntries * BLOCK * 4; }

template <class K> hipError_t guide_residency(K kernel, const GuidePlan& plan, int* perCU)
{
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)guide_lds(plan)); if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, kernel, BLOCK, guide_lds(plan));
}

} // namespace

extern "C" hipError_t guide_plan_grid(GuidePlan* plan, uint32_t regions)
{
    if (!plan || !plan->ok || !plan->ldsEntries) return hipErrorInvalidValue;
    int numCUs = 0, perCU = 0;
    hipError_t e = pt_device_cus(&numCUs); if (e != hipSuccess) return e;
    e = plan->overflowEntries ? guide_residency(pt_guides<true>, *plan, &perCU) : guide_residency(pt_guides<false>, *plan, &perCU); if (e != hipSuccess) return e;
    /* residency capped at 8 workgroups per CU like the pre-pass grids (pt_variant.inc launchKernel) */
    const uint64_t resident = (uint64_t)(perCU > 0 ? (perCU > 8 ? 8 : perCU) : 1) * (uint64_t)numCUs;
    plan->grid = (uint32_t)(regions < 2 * resident ? regions : 2 * resident);
    plan->lanes = plan->grid * BLOCK;
    return hipSuccess;
}

extern "C" hipError_t guide_launch(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W, uint32_t H,
    uint32_t firstFrame, uint32_t numFrames, const TbTileMap* tiles, const GuidePlan* plan, uint32_t* overflow, TbFloat4* albedo, TbFloat4* normal,
    TbFloat4* position)
{
    if (!ds || !pf || !tg || !tiles || !plan || !plan->ok || !plan->grid || !W || !H || W > 16384u || H > 16384u || !numFrames) return hipErrorInvalidValue;
    if (!guide_surface(albedo) || !guide_surface(normal) || !guide_surface(position)) return hipErrorInvalidValue;
    if (plan->grid > tb_persistent_grid(W, H, *tiles) || plan->lanes != plan->grid * BLOCK) return hipErrorInvalidValue;
    if (plan->ldsEntries + plan->overflowEntries < ds->stackDepth) return hipErrorInvalidValue; /* a stack shallower than the tree */
    if ((plan->overflowEntries != 0) != (overflow != nullptr)) return hipErrorInvalidValue;
    TbDeviceScene scene = *ds; /* the scene as this launch walks it: layout B, this launch's split of the stack */
    scene.nodesC = nullptr; scene.stackDepth = plan->ldsEntries; scene.stackOverflow = overflow; scene.stackOverflowLanes = overflow ? plan->lanes : 0u;
    const size_t lds = guide_lds(*plan);
    if (overflow) {
        const hipError_t e = hipFuncSetAttribute((const void*)pt_guides<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pt_guides<true>, dim3(plan->grid), dim3(BLOCK), lds, stream, scene, *pf, *tg, W, H, firstFrame, numFrames, *tiles, albedo, normal, position);
    } else {
        const hipError_t e = hipFuncSetAttribute((const void*)pt_guides<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pt_guides<false>, dim3(plan->grid), dim3(BLOCK), lds, stream, scene, *pf, *tg, W, H, firstFrame, numFrames, *tiles, albedo, normal, position);
    }
    return hipGetLastError();
}
