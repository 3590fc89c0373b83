/* pt_kernels.hip -- gfx950 kernels of the path tracer and their launchers.
 *
 * pt_persistent<SCENE_LDS, COUNT>: the replacement of SoftwareRayTraceCS::main
 * (/root/reference/TracerBoy/SoftwareRayTraceCS.hlsl:9-51).  One lane owns one pixel for ALL
 * frames of the launch ("persistent" lanes with path regeneration): when its path ends it
 * accumulates the sample exactly like RayGenCommon.h:704-727 and immediately starts the next
 * frame's path, so a wavefront only idles at the very end of the launch instead of at the end of
 * every frame's longest path.  Per-pixel sample order is frame order, so the fp32 accumulation is
 * bit-identical to the reference's one-dispatch-per-frame loop.
 *   - every loop iteration casts exactly one ray per live lane (bounce, shadow or SSS ray), through
 *     ONE traversal instance -> no duplicated traversal code, ray types share the wave;
 *   - wave = 8x8 pixel tile (the reference's thread-group shape), block = 2x2 tiles;
 *   - traversal stack in LDS, [entry][lane] layout (bank-conflict free, unlike the reference's
 *     lane*16+entry, TraverseFunction.hlsli:147-154);
 *   - SCENE_LDS: scenes whose whole kernel-visible image (nodes, triangles, hit-group records,
 *     indices, vertices, materials, lights) fits the LDS budget are copied into LDS once per block
 *     with coalesced 16-B loads; all traversal and shading fetches are then ds_reads.
 */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"

namespace {

/* Closest-hit batch for the traversal parity tests (IntersectWithMaxDistance, RayGenCommon.h:365-414); NODEC: through the compact
 * layout-C nodes (one-level scenes) */
template <bool NODEC>
__global__ __launch_bounds__(BLOCK) void trace_closest_kernel(TbDeviceScene ds, uint32_t n, const float* origins, const float* dirs, float* outT, int* outMat,
                                                               float* outBary, uint32_t* outPrim, uint32_t* outGeom, float* outNormal, float* outUV,
                                                               uint32_t* outBoxes, uint32_t* outTris)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* stack = (uint32_t*)smem + threadIdx.x;
    SceneRefs sc; make_refs<false>(sc, ds, nullptr);
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    tb3 o = ld3(origins + 3 * i), d = ld3(dirs + 3 * i);
    Hit h; uint32_t nb = 0, nt = 0;
    bool hit;
    if (NODEC) hit = traverse<true, true, false, true>(sc, ds, o, d, h, stack, BLOCK, nb, nt);
    else hit = ds.numInstances ? traverse_instanced<true, true>(sc, ds, o, d, h, stack, BLOCK, nb, nt) : traverse<true, true>(sc, ds, o, d, h, stack, BLOCK,
        nb, nt);
    outT[i] = hit ? h.t : -1.0f;
    if (outBary) { outBary[2 * i] = hit ? h.u : 0.0f; outBary[2 * i + 1] = hit ? h.v : 0.0f; }
    if (outPrim) outPrim[i] = hit ? h.prim : 0xffffffffu;
    if (outGeom) outGeom[i] = hit ? h.geom : 0xffffffffu;
    if (outBoxes) outBoxes[i] = nb;
    if (outTris) outTris[i] = nt;
    Surface s; s.normal = tb3_splat(0.0f); s.u = s.v = 0.0f; s.material = -1;
    if (hit) fetch_surface(sc, h, s, false);
    if (outMat) outMat[i] = s.material;
    if (outNormal) { outNormal[3 * i] = s.normal.x; outNormal[3 * i + 1] = s.normal.y; outNormal[3 * i + 2] = s.normal.z; }
    if (outUV) { outUV[2 * i] = s.u; outUV[2 * i + 1] = s.v; }
}

__global__ void device_math_kernel(int fn, uint32_t n, const float* a, const float* b, float* out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b ? b[i] : 0.0f, r = 0.0f;
    switch (fn) {
    case 0: r = tb_sin(x); break; case 1: r = tb_cos(x); break; case 2: r = tb_acos(x); break; case 3: r = tb_atan2(x, y); break;
    case 4: r = tb_exp(x); break; case 5: r = tb_log(x); break; case 6: r = tb_pow(x, y); break; case 7: r = tb_sqrt(x); break;
    case 8: r = tb_exp2(x); break; case 9: r = tb_log2(x); break; case 10: r = tb_asin(x); break;
    case 11: r = x / y; break; case 12: r = tb_frac(tb_sin(x + y) * 43758.5453123f); break; case 13: r = hash13(x, y, 0.0f); break;
    case 14: r = tb_min(x, y); break; case 15: r = tb_max(x, y); break; case 16: r = tb_frac(x); break; case 17: r = tb_floor(x); break;
        case 18: r = tb_rcp(x); break;
    /* 19 .. 22: the short forms of tb_math.h, which the oracle does not call (device only; tests/test_shading_short_forms.py): tb_sincos's sine, its cosine */
    case 19: tb_sincos(x, &r, &y); break; case 20: tb_sincos(x, &y, &r); break; case 21: r = tb_div_pi(x); break; case 22: r = tb_zero_over_sqrt(x); break;
    default: break;
    }
    out[i] = r;
}

/* tile-major pack of the pixels this rank owns (tb_pack_owned_device) */
__global__ void pack_owned_kernel(const TbFloat4* full, TbFloat4* packed, uint32_t W, uint32_t H, TbTileMap tiles, uint32_t numOwnedTiles)
{
    uint32_t tilesX = (W + tiles.tileW - 1) / tiles.tileW;
    uint32_t local = blockIdx.x; /* index among owned tiles */
    if (local >= numOwnedTiles) return;
    uint32_t t = tiles.rank + local * tiles.world;
    uint32_t tx = t % tilesX, ty = t / tilesX;
    uint32_t x0 = tx * tiles.tileW, y0 = ty * tiles.tileH;
    uint32_t tw = min(tiles.tileW, W - x0), th = min(tiles.tileH, H - y0);
    size_t base = (size_t)local * tiles.tileW * tiles.tileH;
    for (uint32_t i = threadIdx.x; i < tw * th; i += blockDim.x) {
        uint32_t lx = i % tw, ly = i / tw;
        packed[base + i] = full[(size_t)(y0 + ly) * W + (x0 + lx)];
    }
}

/* rank 0 of a tile split: the inverse of pack_owned_kernel over the gathered buffers of all ranks (tb_unpack_gathered_device).
 * gathered = world x capacity pixels, rank r's packed tiles at r * capacity; one workgroup per tile of the frame. */
__global__ void unpack_gathered_kernel(const TbFloat4* gathered, size_t capacity, TbFloat4* full, uint32_t W, uint32_t H, uint32_t world, uint32_t tileW,
    uint32_t tileH)
{
    const uint32_t tilesX = (W + tileW - 1) / tileW, t = blockIdx.x;
    const uint32_t rank = t % world, local = t / world;
    const uint32_t x0 = (t % tilesX) * tileW, y0 = (t / tilesX) * tileH;
    const uint32_t tw = min(tileW, W - x0), th = min(tileH, H - y0);
    const TbFloat4* src = gathered + (size_t)rank * capacity + (size_t)local * tileW * tileH;
    for (uint32_t i = threadIdx.x; i < tw * th; i += blockDim.x) {
        const uint32_t lx = i % tw, ly = i / tw;
        full[(size_t)(y0 + ly) * W + (x0 + lx)] = src[i];
    }
}

/* Ordered sum of the frame-group mode's sample buffer (TbDeviceTargets::samples): RayGenCommon.h:721-727 per pixel,
 * frames in order.  One lane per owned pixel; reads numFrames x 16 B, HBM-bound. */
__global__ __launch_bounds__(256) void accumulate_samples_kernel(const TbFloat4* samples, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames,
    TbTileMap tiles,
                                                                 TbFloat4* output, TbFloat4* jittered)
{
    const uint32_t n = W * H;
    for (uint32_t pix = blockIdx.x * 256u + threadIdx.x; pix < n; pix += gridDim.x * 256u) {
        if (tiles.world > 1) {
            const uint32_t x = pix % W, y = pix / W, tx = (W + tiles.tileW - 1) / tiles.tileW;
            if ((((y / tiles.tileH) * tx + (x / tiles.tileW)) % tiles.world) != tiles.rank) continue;
        }
        TbFloat4 acc = {0, 0, 0, 0}, jacc = {0, 0, 0, 0};
        if (firstFrame > 0) { acc = output[pix]; jacc = jittered[pix]; }
        for (uint32_t f = 0; f < numFrames; f++) {
            const TbFloat4 s = samples[(size_t)f * n + pix];
            const uint32_t frame = firstFrame + f;
            const float o3 = tb_abs(s.w);
            const bool coinLow = (__float_as_uint(s.w) >> 31) != 0;
            if (frame == 0) acc = TbFloat4{0, 0, 0, 0};
            acc = TbFloat4{s.x + acc.x, s.y + acc.y, s.z + acc.z, o3 + acc.w};
            if (frame == 0 || coinLow) {
                if (frame == 0) jacc = TbFloat4{0, 0, 0, 0};
                jacc = TbFloat4{s.x + jacc.x, s.y + jacc.y, s.z + jacc.z, o3 + jacc.w};
            }
        }
        output[pix] = acc; jittered[pix] = jacc;
    }
}

/* The same fold for the list-driven frame-group launch (TbDeviceTargets::liveList, pt_scene.h): one lane per list entry, the same fp32 sums in the
 * same order; the pixels that are not on the list have no samples in the buffer and keep their sums.  The count is read here, from the 16 bytes
 * before the list; the grid is sized by an upper bound. */
__global__ __launch_bounds__(256) void accumulate_live_kernel(const TbFloat4* samples, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames,
    const uint32_t* __restrict__ list, TbFloat4* output, TbFloat4* jittered)
{
    const uint32_t n = W * H, count = list[-TB_LIVE_COUNT_WORDS];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
        const uint32_t xy = list[i], pix = (xy >> 16) * W + (xy & 0xffffu);
        TbFloat4 acc = {0, 0, 0, 0}, jacc = {0, 0, 0, 0};
        if (firstFrame > 0) { acc = output[pix]; jacc = jittered[pix]; }
        for (uint32_t f = 0; f < numFrames; f++) {
            const TbFloat4 s = samples[(size_t)f * n + pix];
            const uint32_t frame = firstFrame + f;
            const float o3 = tb_abs(s.w);
            const bool coinLow = (__float_as_uint(s.w) >> 31) != 0;
            if (frame == 0) acc = TbFloat4{0, 0, 0, 0};
            acc = TbFloat4{s.x + acc.x, s.y + acc.y, s.z + acc.z, o3 + acc.w};
            if (frame == 0 || coinLow) {
                if (frame == 0) jacc = TbFloat4{0, 0, 0, 0};
                jacc = TbFloat4{s.x + jacc.x, s.y + jacc.y, s.z + jacc.z, o3 + jacc.w};
            }
        }
        output[pix] = acc; jittered[pix] = jacc;
    }
}

} // namespace

/* TbDeviceTargets::regionOrder from TbDeviceTargets::regionCost (pt_scene.h): one workgroup of 1024.  order[0] = items moved to the front, order[1 ...] =
 * a permutation of the launch's items (group << 20 | region, claim_work_item's usual list: group by group, regions ascending): first the items of
 * COUNTED regions that the usual list holds at position lateFrom or later, then everything else, both parts in their usual order -- neighbours stay
 * neighbours in the list (a first version sorted counted regions by count with atomics: what ran side by side was then scattered over the frame,
 * and the whole-frame van-class step lost 1.2 % to the caches), and a launch much longer than its longest path keeps its usual order except for
 * its end.  keys (regions words of scratch) holds the ONE reading of every count that all passes use: other launches keep counting while this
 * runs, and an item read as moved in one pass and as not moved in the next would be handed out twice or never. */
__global__ __launch_bounds__(1024) void region_order_kernel(const uint32_t* __restrict__ cost, TbTileMap tiles, uint32_t W, uint32_t H,
    uint32_t regions, uint32_t numGroups, uint32_t lateFrom, uint32_t* __restrict__ order, uint32_t* __restrict__ keys)
{
    __shared__ uint32_t waveSum[16], base[2], moved;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, items = regions * numGroups;
    if (t == 0) moved = 0;
    for (uint32_t i = t; i < regions; i += 1024u) {
        uint32_t bx, by; block_region(tiles, W, H, i, bx, by);
        keys[i] = __hip_atomic_load(cost + ((by & 1023u) << 10 | (bx & 1023u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
    }
    __syncthreads(); /* (a workgroup's own global writes are visible to it after the barrier) */
    uint32_t mine = 0;
    for (uint32_t i = lateFrom + t; i < items; i += 1024u) mine += keys[i % regions];
    if (mine) atomicAdd(&moved, mine);
    __syncthreads();
    if (t == 0) { order[0] = moved; base[1] = 0; base[0] = moved; }
    __syncthreads();
    for (uint32_t i0 = 0; i0 < items; i0 += 1024u) {
        const uint32_t i = i0 + t, group = i < items ? i / regions : 0u, region = i - group * regions;
        const bool in = i < items, front = in && i >= lateFrom && keys[region] != 0u;
        const unsigned long long m = __ballot(front);
        const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) waveSum[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t frontBefore = before, total = 0;
        for (uint32_t w = 0; w < 16u; w++) { const uint32_t v = waveSum[w]; if (w < wave) frontBefore += v; total += v; }
        /* (system scope, as claim_work_item reads it) */
        if (front) __hip_atomic_store(order + 1u + base[1] + frontBefore, group << 20 | region, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else if (in) __hip_atomic_store(order + 1u + base[0] + (t - frontBefore), group << 20 | region, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __syncthreads();
        if (t == 0) { base[1] += total; base[0] += 1024u - total; }
        __syncthreads();
    }
}

/* The live list of the adaptive launch (TbDeviceTargets::liveList, pt_scene.h): one pass over the context's owned regions in tb_persistent_grid /
 * block_region order -- the regions of its tiles, or the whole frame.  live_list_count applies the skip test (tb_adaptive_skip, pt_device.hpp) at the
 * launch's first frame to the 256 pixels of a region in the lock-step kernel's own lane mapping (wave w = the 8x8 tile (w & 1, w >> 1), lane =
 * (lane & 7, lane >> 3)), keeps the four waves' ballots and the region's count, and leaves a skipped pixel's AOVs (the reference's ClearAOVs +
 * OutputLivePixels); live_list_scan turns the counts into every region's first entry (exclusive, in place) and the total; live_list_scatter writes
 * x | y << 16 of each live pixel at its region's first entry + the live pixels of the waves before + mbcnt.  Region, then wave, then lane: a wholly
 * live region gives the dense launch's own waves.  Nothing is ordered by atomics, so the list depends on the surfaces alone. */
__global__ __launch_bounds__(256) void live_list_count(const TbFloat4* __restrict__ output, const TbFloat4* __restrict__ jittered, TbTileMap tiles, uint32_t W,
    uint32_t H, uint32_t frame, uint32_t minFrames, float minConvergence, unsigned long long* __restrict__ masks, uint32_t* __restrict__ counts,
    TbFloat4* __restrict__ aovNormals, TbFloat4* __restrict__ aovCustom, uint32_t livePixelsMode)
{
    __shared__ uint32_t waveLive[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, region = blockIdx.x;
    uint32_t bx, by; block_region(tiles, W, H, region, bx, by);
    const uint32_t x = bx * 16u + (wave & 1u) * 8u + (lane & 7u), y = by * 16u + (wave >> 1) * 8u + (lane >> 3);
    bool live = x < W && y < H;
    if (live && frame > minFrames) {
        const size_t pix = (size_t)y * W + x;
        const TbFloat4 o = output[pix];
        if (tb_adaptive_skip(o, jittered[pix], minConvergence)) {
            live = false;
            if (aovNormals) aovNormals[pix] = TbFloat4{0, 0, 0, 1.0f};
            if (aovCustom) aovCustom[pix] = livePixelsMode ? TbFloat4{o.x / o.w, o.y / o.w, o.z / o.w, o.w / o.w} : TbFloat4{0, 0, 0, 1.0f};
        }
    }
    const unsigned long long m = __ballot(live);
    if (lane == 0) { masks[(size_t)region * 4u + wave] = m; waveLive[wave] = (uint32_t)__popcll(m); }
    __syncthreads();
    if (threadIdx.x == 0) counts[region] = waveLive[0] + waveLive[1] + waveLive[2] + waveLive[3];
}

/* live_list_count for a call under a sample budget (tb_set_sample_budget): the same lane mapping, ballots and AOV writes; a
 * pixel is live iff the launch's first frame is below its budget -- and, where the adaptive test is on too (minFrames is 0xffffffff where it is
 * not: no frame is past it), the skip test does not hold.  The surfaces are read only where the skip test or the LIVE_PIXELS tint needs them. */
__global__ __launch_bounds__(256) void live_list_count_budget(const TbFloat4* __restrict__ output, const TbFloat4* __restrict__ jittered,
    const uint32_t* __restrict__ budget, TbTileMap tiles, uint32_t W, uint32_t H, uint32_t frame, uint32_t minFrames, float minConvergence,
    unsigned long long* __restrict__ masks, uint32_t* __restrict__ counts, TbFloat4* __restrict__ aovNormals, TbFloat4* __restrict__ aovCustom,
    uint32_t livePixelsMode)
{
    __shared__ uint32_t waveLive[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, region = blockIdx.x;
    uint32_t bx, by; block_region(tiles, W, H, region, bx, by);
    const uint32_t x = bx * 16u + (wave & 1u) * 8u + (lane & 7u), y = by * 16u + (wave >> 1) * 8u + (lane >> 3);
    bool live = x < W && y < H;
    if (live) {
        const size_t pix = (size_t)y * W + x;
        bool skip = !(frame < budget[pix]);
        const bool test = !skip && frame > minFrames;
        TbFloat4 o = {0, 0, 0, 0};
        if (test || (skip && aovCustom && livePixelsMode)) o = output[pix];
        if (test) skip = tb_adaptive_skip(o, jittered[pix], minConvergence);
        if (skip) {
            live = false;
            if (aovNormals) aovNormals[pix] = TbFloat4{0, 0, 0, 1.0f};
            if (aovCustom) aovCustom[pix] = livePixelsMode ? TbFloat4{o.x / o.w, o.y / o.w, o.z / o.w, o.w / o.w} : TbFloat4{0, 0, 0, 1.0f};
        }
    }
    const unsigned long long m = __ballot(live);
    if (lane == 0) { masks[(size_t)region * 4u + wave] = m; waveLive[wave] = (uint32_t)__popcll(m); }
    __syncthreads();
    if (threadIdx.x == 0) counts[region] = waveLive[0] + waveLive[1] + waveLive[2] + waveLive[3];
}

/* one workgroup: thread t sums a contiguous run of the counts, the 1024 sums are scanned in LDS, the runs are rewritten as first entries */
__global__ __launch_bounds__(1024) void live_list_scan(uint32_t* __restrict__ counts, uint32_t regions, uint32_t* __restrict__ total)
{
    __shared__ uint32_t sums[1024];
    const uint32_t t = threadIdx.x, per = (regions + 1023u) / 1024u;
    const uint32_t b = t * per < regions ? t * per : regions, e = b + per < regions ? b + per : regions;
    uint32_t own = 0;
    for (uint32_t i = b; i < e; i++) own += counts[i];
    sums[t] = own;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
        const uint32_t v = t >= off ? sums[t - off] : 0u;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    uint32_t run = sums[t] - own;
    for (uint32_t i = b; i < e; i++) { const uint32_t c = counts[i]; counts[i] = run; run += c; }
    if (t == 1023u) *total = sums[1023];
}

__global__ __launch_bounds__(256) void live_list_scatter(TbTileMap tiles, uint32_t W, uint32_t H, const unsigned long long* __restrict__ masks,
    const uint32_t* __restrict__ first, uint32_t* __restrict__ list)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, region = blockIdx.x;
    const unsigned long long* m = masks + (size_t)region * 4u;
    const unsigned long long mine = m[wave];
    if (!((mine >> lane) & 1ull)) return;
    uint32_t pos = first[region];
    for (uint32_t w = 0; w < wave; w++) pos += (uint32_t)__popcll(m[w]);
    pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
    uint32_t bx, by; block_region(tiles, W, H, region, bx, by);
    list[pos] = (bx * 16u + (wave & 1u) * 8u + (lane & 7u)) | (by * 16u + (wave >> 1) * 8u + (lane >> 3)) << 16;
}

extern "C" {

hipError_t pt_launch_accumulate_samples(hipStream_t stream, const TbFloat4* samples, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames,
    const TbTileMap* tiles,
                                        TbFloat4* output, TbFloat4* jittered)
{
    hipLaunchKernelGGL(accumulate_samples_kernel, dim3(2048), dim3(256), 0, stream, samples, W, H, firstFrame, numFrames, *tiles, output, jittered);
    return hipGetLastError();
}

hipError_t pt_launch_accumulate_live(hipStream_t stream, const TbFloat4* samples, uint32_t W, uint32_t H, uint32_t firstFrame, uint32_t numFrames,
                                     const uint32_t* list, uint64_t maxEntries, TbFloat4* output, TbFloat4* jittered)
{
    const uint64_t blocks = (maxEntries + 255u) / 256u;
    if (blocks) hipLaunchKernelGGL(accumulate_live_kernel, dim3((uint32_t)(blocks < 2048u ? blocks : 2048u)), dim3(256), 0, stream, samples, W, H, firstFrame,
        numFrames, list, output, jittered);
    return hipGetLastError();
}

hipError_t pt_launch_region_order(hipStream_t stream, const uint32_t* cost, const TbTileMap* tiles, uint32_t W, uint32_t H, uint32_t regions,
                                  uint32_t numGroups, uint32_t lateFrom, uint32_t* order, uint32_t* keys)
{
    hipLaunchKernelGGL(region_order_kernel, dim3(1), dim3(1024), 0, stream, cost, *tiles, W, H, regions, numGroups, lateFrom, order, keys);
    return hipGetLastError();
}

/* TbDeviceTargets::liveList / liveCount for the launch whose first frame is `frame` (live_list_* above).  scratch: tb_live_list_scratch_bytes(regions).
 * budget: null, or W x H frame indices (live_list_count_budget in live_list_count's place; minFrames 0xffffffff: no skip test) */
hipError_t pt_launch_live_list(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, const uint32_t* budget, const TbTileMap* tiles, uint32_t W,
                               uint32_t H, uint32_t frame, uint32_t minFrames, float minConvergence, TbFloat4* aovNormals, TbFloat4* aovCustom,
                               int livePixelsMode, void* scratch, uint32_t* list, uint32_t* count)
{
    const uint32_t regions = tb_persistent_grid(W, H, *tiles);
    unsigned long long* masks = (unsigned long long*)scratch;
    uint32_t* counts = (uint32_t*)(masks + (size_t)regions * 4u);
    if (regions && budget) hipLaunchKernelGGL(live_list_count_budget, dim3(regions), dim3(256), 0, stream, output, jittered, budget, *tiles, W, H, frame,
        minFrames, minConvergence, masks, counts, aovNormals, aovCustom, livePixelsMode ? 1u : 0u);
    else if (regions) hipLaunchKernelGGL(live_list_count, dim3(regions), dim3(256), 0, stream, output, jittered, *tiles, W, H, frame, minFrames, minConvergence, masks,
        counts, aovNormals, aovCustom, livePixelsMode ? 1u : 0u);
    hipLaunchKernelGGL(live_list_scan, dim3(1), dim3(1024), 0, stream, counts, regions, count);
    if (regions) hipLaunchKernelGGL(live_list_scatter, dim3(regions), dim3(256), 0, stream, *tiles, W, H, (const unsigned long long*)masks,
        (const uint32_t*)counts, list);
    return hipGetLastError();
}

hipError_t pt_launch_trace_closest(hipStream_t stream, const TbDeviceScene* ds, uint32_t n, const float* origins, const float* dirs, float* outT, int* outMat,
                                   float* outBary, uint32_t* outPrim, uint32_t* outGeom, float* outNormal, float* outUV, uint32_t* outBoxes, uint32_t* outTris)
{
    size_t lds = (size_t)ds->stackDepth * BLOCK * 4;
    if (ds->nodesC && ds->numInstances) return hipErrorInvalidValue; /* layout C is built for one-level scenes */
    const void* fn = ds->nodesC ? (const void*)trace_closest_kernel<true> : (const void*)trace_closest_kernel<false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (ds->nodesC) hipLaunchKernelGGL(trace_closest_kernel<true>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), lds, stream, *ds, n, origins, dirs, outT,
        outMat, outBary, outPrim, outGeom, outNormal, outUV, outBoxes, outTris);
    else hipLaunchKernelGGL(trace_closest_kernel<false>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), lds, stream, *ds, n, origins, dirs, outT, outMat, outBary,
        outPrim, outGeom, outNormal, outUV, outBoxes, outTris);
    return hipGetLastError();
}

hipError_t pt_launch_device_math(hipStream_t stream, int fn, uint32_t n, const float* a, const float* b, float* out)
{
    hipLaunchKernelGGL(device_math_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, n, a, b, out);
    return hipGetLastError();
}

hipError_t pt_launch_unpack_gathered(hipStream_t stream, const TbFloat4* gathered, size_t capacity, TbFloat4* full, uint32_t W, uint32_t H, uint32_t world,
    uint32_t tileW, uint32_t tileH)
{
    const uint32_t tilesTotal = ((W + tileW - 1) / tileW) * ((H + tileH - 1) / tileH);
    if (tilesTotal == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_gathered_kernel, dim3(tilesTotal), dim3(256), 0, stream, gathered, capacity, full, W, H, world, tileW, tileH);
    return hipGetLastError();
}

hipError_t pt_launch_pack_owned(hipStream_t stream, const TbFloat4* full, TbFloat4* packed, uint32_t W, uint32_t H, const TbTileMap* tiles,
    uint32_t numOwnedTiles)
{
    if (numOwnedTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_owned_kernel, dim3(numOwnedTiles), dim3(256), 0, stream, full, packed, W, H, *tiles, numOwnedTiles);
    return hipGetLastError();
}

} // extern "C"
