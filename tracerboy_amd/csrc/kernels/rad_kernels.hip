/* rad_kernels.hip -- radiance queries (include/tracerboy_hip.h tb_trace_radiance / tb_make_camera_rays): the path tracer on a
 * caller's rays.
 *
 * rad_paths<F, HYBRID, REFILL>: pt_paths' loop for a lane that never waits (vis_kernels.hip; pt_stream.inc:51-118) -- walk the pending ray, then
 * path_on_closest / path_on_shadow / path_on_sss by the path's state, then path_scatter -- for the feature set F, the scene fetched from memory, two
 * levels where the scene has instances, the stack in LDS [entry][lane] with the deepest entries in the lane's global column where the tree is deeper
 * than the LDS share (HYBRID, guide_launch.h).  A lane owns one RAY and runs its samples in order with the sum in registers: a sample begins where
 * path_begin would leave the renderer's path (T = 1, L = 0, bounce 0, weight 1, the seed hash13(SeedX, SeedY, s) stepped on by seed_advance) on the record's origin
 * and direction -- in hemisphere mode on GenerateCosineWeightedDirection(normal, r0, r1) of two numbers drawn first --, and ends as pt_paths' does
 * (vis_kernels.hip:79-84): the firefly clamp, the NaN filter, acc = acc + sample.  A lane whose path ends begins its next sample in the next pass of
 * the one loop: the sample loop is the path regeneration.  The record is read again for every sample rather than held in eight registers.
 * Rays reach lanes from a wave's pool of consecutive indices, by the lane's rank among the idle lanes:
 *   REFILL = false  the pool is a batch of 64 rays, taken when all 64 lanes are idle; a wave's batches are strided over the grid's waves (a grid
 *                   that covers n: one batch per wave);
 *   REFILL = true   a persistent grid; the pool is `chunk` indices that lane 0 claims from *counter with one atomic add when it is empty, taken from
 *                   whenever refillMin lanes are idle (rq_kernels.hip has the design and why a claim per refill was given up).
 * No wave waits for another and there is no fence: a ray's result is written once, by index, by the lane that owned it.  The loop is left on
 * wave-uniform conditions (ballots); it is bounded by n (every pass without a live path draws rays or retires some), num_samples, MaxBounces and
 * the tree.  A ray's value depends on its record, the call and the scene alone -- not on the lane, the wave, the form or the grid.
 *
 * rad_camera_rays: path_begin<FEAT_ALL> per pixel of a window, stored as ray records; the seed's advance is read off the first pixel's path. */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"
#include "rad_launch.h"

namespace {

struct RadRay { tb3 o, d; float seedX, seedY; };
__device__ __forceinline__ RadRay rad_load_ray(const TbRadianceRay* rays, uint32_t i) /* 32 B, 16-B aligned: two 16-B loads */
{
    const uint4* p = (const uint4*)(rays + i);
    const uint4 a = p[0], b = p[1];
    RadRay q;
    q.o = tb3_make(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)); q.seedX = __uint_as_float(a.w);
    q.d = tb3_make(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z)); q.seedY = __uint_as_float(b.w);
    return q;
}
__device__ __forceinline__ bool rad_finite(float x) { return tb_abs(x) < __builtin_inff(); } /* false for a NaN */
/* what is traced at all: a finite origin, a finite direction that is not all zero */
__device__ __forceinline__ bool rad_traced(const RadRay& q)
{
    const bool finite = rad_finite(q.o.x) && rad_finite(q.o.y) && rad_finite(q.o.z) && rad_finite(q.d.x) && rad_finite(q.d.y) && rad_finite(q.d.z);
    return finite && (q.d.x != 0.0f || q.d.y != 0.0f || q.d.z != 0.0f);
}
/* GenerateCosineWeightedDirection, kernel.glsl:1025-1041, as path_scatter's diffuse side has it */
__device__ __forceinline__ tb3 rad_cosine_direction(tb3 n, float r0, float r1)
{
    const float r = tb_sqrt(r0), theta = (2.0f * PI) * r1;
    return reorient(tb3_make(r * tb_cos(theta), tb_sqrt(tb_max(EPSILON, 1.0f - r0)), r * tb_sin(theta)), n);
}

/* seedSteps, seedRest: the call's seed_advance as whole steps of 1 (at most RAD_SEED_STEPS) and what is left of it, added last */
struct RadArgs { uint32_t n, firstSample, numSamples, hemisphere, accumulate, refillMin, chunk, seedSteps; float seedRest; };

template <uint32_t F, bool HYBRID, bool REFILL>
__global__ __launch_bounds__(BLOCK) void rad_paths(TbDeviceScene ds, TbPerFrameConstants pf, RadArgs k, const TbRadianceRay* __restrict__ rays,
    TbFloat4* __restrict__ out, uint32_t* counter)
{
    constexpr bool ALPHA = (F & FEAT_EXT) != 0; /* the IsValidHit filter: the host picks the full set where option alpha_test is on */
    constexpr uint32_t NONE = 0xffffffffu;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SceneRefs sc;
    make_refs<false>(sc, ds, nullptr);
    uint32_t* const stack = (uint32_t*)smem + threadIdx.x;
    uint32_t* const overflow = HYBRID ? ds.stackOverflow + (size_t)blockIdx.x * BLOCK + threadIdx.x : nullptr;
    const uint32_t lane = threadIdx.x & 63u, n = k.n;
    const uint32_t refillMin = REFILL ? k.refillMin : 64u;
    /* the lane's ray (NONE: idle), how many of its samples have begun, their sum */
    uint32_t index = NONE, begun = 0;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    Path p;
    p.state = ST_DONE;
    /* wave-uniform: the pool of indices [poolNext, poolEnd); dry: this wave claims no more */
    uint32_t poolNext = 0, poolEnd = 0;
    bool dry = false;
    uint64_t batch = (uint64_t)blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6); /* REFILL = false: the wave's next batch of 64 */
    for (;;) {
        const unsigned long long idle = __ballot(index == NONE);
        const uint32_t want = (uint32_t)__popcll(idle);
        if ((!dry || poolNext != poolEnd) && want >= refillMin) {
            if (poolNext == poolEnd) { /* (then not dry) */
                if (REFILL) {
                    uint32_t base = 0;
                    if (lane == 0) base = __hip_atomic_fetch_add(counter, k.chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    base = __builtin_amdgcn_readfirstlane(base); /* n <= 2^31, chunk <= 2^16 and every wave overshoots once: no wrap */
                    poolNext = base < n ? base : n; poolEnd = base + k.chunk < n ? base + k.chunk : n;
                    dry = base + k.chunk >= n;
                } else {
                    const uint64_t base = batch * 64u;
                    batch += (uint64_t)gridDim.x * (BLOCK / 64u);
                    poolNext = base < n ? (uint32_t)base : n; poolEnd = base + 64u < n ? (uint32_t)(base + 64u) : n;
                    dry = batch * 64u >= n;
                }
            }
            const uint32_t i = poolNext + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            if (index == NONE && i < poolEnd) {
                if (rad_traced(rad_load_ray(rays, i))) {
                    index = i; begun = 0;
                    a0 = a1 = a2 = a3 = 0.0f;
                    if (k.accumulate) { const TbFloat4 o = out[i]; a0 = o.x; a1 = o.y; a2 = o.z; a3 = o.w; }
                } else if (!k.accumulate) out[i] = TbFloat4{0.0f, 0.0f, 0.0f, 0.0f}; /* not traced: zeros, or what out[i] holds */
            }
            poolNext = poolNext + want < poolEnd ? poolNext + want : poolEnd;
        }
        /* a lane with a ray and no path under way: the sample that has just ended goes to the sum, then the next one begins or the ray retires */
        if (index != NONE && p.state == ST_DONE) {
            if (begun) { /* vis_kernels.hip:79-84; the weight is 1 */
                tb3 color = p.L;
                if (pf.FireflyClampValue >= EPSILON) color = tb3_min(color, tb3_splat(pf.FireflyClampValue));
                if (!(tb_isnan(color.x) || tb_isnan(color.y) || tb_isnan(color.z))) { a0 = a0 + color.x; a1 = a1 + color.y; a2 = a2 + color.z; a3 = a3 + 1.0f; }
            }
            if (begun == k.numSamples) { out[index] = TbFloat4{a0, a1, a2, a3}; index = NONE; }
            else {
                const RadRay q = rad_load_ray(rays, index);
                const uint32_t s = k.firstSample + begun;
                begun++;
                p.flags = 0; p.bounce = 0; p.lastBoxes = p.lastTris = 0; p.nMat = p.nLight = 0;
                p.aovNormal = p.aovAlbedo = p.aovEmissive = p.aovWorldPos = tb3_splat(0.0f); p.aovNeighbor = 0.0f; p.aovDepth = 0.0f;
                p.weight = 1.0f; p.L = tb3_splat(0.0f); p.T = tb3_splat(1.0f);
                /* the advance as rand() makes it, in steps of 1: hash13 has bits below the ulp of hash13 + 16, and a chain of sixteen rounded
                 * additions is not the one addition (pixel (10, 0) of frame 0 already differs) */
                p.seed = hash13(q.seedX, q.seedY, (float)s);
                for (uint32_t j = 0; j < k.seedSteps; j++) p.seed = p.seed + 1.0f;
                p.seed = p.seed + k.seedRest;
                p.ro = q.o; p.rd = q.d;
                if (k.hemisphere) { const float r0 = rnd(p.seed, pf.Time); const float r1 = rnd(p.seed, pf.Time); p.rd = rad_cosine_direction(q.d, r0, r1); }
                p.neighborDir = p.rd;
                p.state = pf.MaxBounces > 0 ? ST_EXTEND : ST_DONE;
            }
        }
        if (__ballot(p.state != ST_DONE) == 0ull) {
            /* nobody walks: samples that ended where they began (MaxBounces 0), rays that retired, rays that were not traced, or nothing left */
            if (__ballot(index != NONE) == 0ull && dry && poolNext == poolEnd) break;
            continue;
        }
        if (p.state != ST_DONE) {
            /* the pending ray: the bounce ray, a feeler or a step of an interior walk */
            float travel = 0.0f;
            if ((F & FEAT_SSS) && p.state == ST_SSS) travel = sss_travel(p, pf);
            Hit h; uint32_t nb = 0, nt = 0;
            bool isHit;
            if (ds.numInstances) isHit = traverse_instanced<false, ALPHA, HYBRID>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, overflow);
            else isHit = traverse<false, ALPHA, HYBRID, false, false, (F & FEAT_SSS) != 0>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, nullptr, overflow);
            if (p.state == ST_EXTEND) path_on_closest<F>(p, sc, ds, pf, isHit, h);
            else if (p.state == ST_SHADOW) path_on_shadow<F>(p, sc, ds, pf, isHit, h);
            else if (F & FEAT_SSS) path_on_sss(p, sc, pf, isHit, h, travel);
            if (p.state == ST_SCATTER) path_scatter<F>(p, pf);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void rad_camera_rays(TbDeviceScene ds, TbPerFrameConstants pf, TbDeviceTargets tg, uint32_t W, uint32_t H, uint32_t x0,
    uint32_t y0, uint32_t x1, uint32_t y1, uint32_t frame, TbRadianceRay* __restrict__ out, float* __restrict__ advance)
{
    const uint32_t w = x1 - x0, i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= w * (y1 - y0)) return;
    const uint32_t x = x0 + i % w, y = y0 + i / w;
    Path p;
    path_begin<FEAT_ALL>(p, ds, pf, frame, W, H, x, y, &tg);
    uint4* o = (uint4*)(out + i);
    o[0] = make_uint4(__float_as_uint(p.ro.x), __float_as_uint(p.ro.y), __float_as_uint(p.ro.z), __float_as_uint((float)x));
    o[1] = make_uint4(__float_as_uint(p.rd.x), __float_as_uint(p.rd.y), __float_as_uint(p.rd.z), __float_as_uint((float)y));
    /* the seed moves in steps of 1 (rnd), and the difference of two floats that lie whole steps apart is the step count to within an ulp */
    if (i == 0) *advance = __builtin_rintf(p.seed - hash13((float)x, (float)y, (float)frame));
}

bool rad_aligned16(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }
size_t rad_lds(const RadPlan& plan) { return (size_t)plan.stack.ldsEntries * BLOCK * 4; }

/* the kernel of a plan: feature set x split stack x form */
template <uint32_t F> const void* rad_kernel_of(bool hybrid, bool refill)
{
    if (hybrid) return refill ? (const void*)rad_paths<F, true, true> : (const void*)rad_paths<F, true, false>;
    return refill ? (const void*)rad_paths<F, false, true> : (const void*)rad_paths<F, false, false>;
}
const void* rad_kernel(const RadPlan& plan)
{
    const bool hybrid = plan.stack.overflowEntries != 0, refill = plan.form != 0;
    switch (plan.features) {
    case 0u: return rad_kernel_of<0u>(hybrid, refill);
    case PT_FEAT_ENV: return rad_kernel_of<PT_FEAT_ENV>(hybrid, refill);
    case PT_FEATS_SURF: return rad_kernel_of<PT_FEATS_SURF>(hybrid, refill);
    case PT_FEATS_SSS: return rad_kernel_of<PT_FEATS_SSS>(hybrid, refill);
    case PT_FEATS_VOL: return rad_kernel_of<PT_FEATS_VOL>(hybrid, refill);
    case PT_FEAT_ALL: return rad_kernel_of<PT_FEAT_ALL>(hybrid, refill);
    }
    return nullptr; /* a feature set that is not compiled: an error, never another kernel */
}
bool rad_plan_ok(const RadPlan& p)
{
    return p.stack.ok && p.stack.ldsEntries && p.form <= 1u && p.refillMin >= 1u && p.refillMin <= 64u && p.chunk >= 16u && p.chunk <= 65536u && p.maxPaths;
}

} // namespace

extern "C" hipError_t rad_plan_grid(RadPlan* plan, uint64_t n, uint32_t gridOverride)
{
    if (!plan || !rad_plan_ok(*plan) || !n || n > 0x80000000ull) return hipErrorInvalidValue;
    const void* kernel = rad_kernel(*plan);
    if (!kernel) return hipErrorInvalidValue;
    const size_t lds = rad_lds(*plan);
    int numCUs = 0, perCU = 0;
    hipError_t e = pt_device_cus(&numCUs); if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, BLOCK, lds); if (e != hipSuccess) return e;
    /* the workgroups the device holds at once; nothing waits for a workgroup, so a count that is too high only queues some */
    const uint64_t resident = (uint64_t)(perCU > 0 ? perCU : 1) * (uint64_t)(numCUs > 0 ? numCUs : 1);
    uint64_t grid;
    if (plan->form) {
        const uint64_t pools = (n + (uint64_t)(BLOCK / 64u) * plan->chunk - 1) / ((uint64_t)(BLOCK / 64u) * plan->chunk); /* no more waves than pools */
        grid = gridOverride ? gridOverride : (pools < resident ? pools : resident);
    } else {
        grid = (n + BLOCK - 1) / BLOCK; /* a batch per wave; with a split stack no more columns than twice the residency: the waves stride */
        if (plan->stack.overflowEntries && grid > 2 * resident) grid = 2 * resident;
    }
    if (grid > 0x7fffffffull / BLOCK) grid = 0x7fffffffull / BLOCK;
    plan->stack.grid = (uint32_t)grid;
    plan->stack.lanes = plan->stack.grid * BLOCK;
    return hipSuccess;
}

extern "C" hipError_t rad_launch(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const RadCall* call, const RadPlan* plan,
    uint32_t* overflow, uint32_t* counter, uint64_t n, const TbRadianceRay* rays, TbFloat4* out, uint32_t* launches)
{
    if (!ds || !pf || !call || !plan || !rad_plan_ok(*plan) || !plan->stack.grid || plan->stack.lanes != plan->stack.grid * BLOCK) return hipErrorInvalidValue;
    if (!n || n > 0x80000000ull || !rad_aligned16(rays) || !rad_aligned16(out)) return hipErrorInvalidValue;
    if (!call->numSamples || call->numSamples > (1u << 24) || (uint64_t)call->firstSample + call->numSamples > (1ull << 32)) return hipErrorInvalidValue;
    if (plan->stack.ldsEntries + plan->stack.overflowEntries < ds->stackDepth) return hipErrorInvalidValue; /* a stack shallower than the tree */
    if ((plan->stack.overflowEntries != 0) != (overflow != nullptr) || (plan->form && !counter)) return hipErrorInvalidValue;
    const void* kernel = rad_kernel(*plan);
    if (!kernel) return hipErrorInvalidValue;
    TbDeviceScene scene = *ds; /* the scene as this launch walks it: layout B, this launch's split of the stack */
    scene.nodesC = nullptr; scene.stackDepth = plan->stack.ldsEntries; scene.stackOverflow = overflow; scene.stackOverflowLanes = overflow ? plan->stack.lanes : 0u;
    TbPerFrameConstants frame = *pf;
    const size_t lds = rad_lds(*plan);
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    /* sample ranges of the same rays, at most maxPaths paths each (at least one sample) */
    const uint64_t fit = plan->maxPaths / n;
    const uint32_t perLaunch = fit < 1 ? 1u : (fit > call->numSamples ? call->numSamples : (uint32_t)fit);
    uint32_t count = 0;
    for (uint32_t done = 0; done < call->numSamples; done += perLaunch, count++) {
        RadArgs k;
        k.n = (uint32_t)n; k.firstSample = call->firstSample + done; k.numSamples = call->numSamples - done < perLaunch ? call->numSamples - done : perLaunch;
        k.hemisphere = call->hemisphere ? 1u : 0u; k.accumulate = call->accumulate || done ? 1u : 0u;
        k.refillMin = plan->refillMin; k.chunk = plan->chunk;
        const float a = call->seedAdvance; /* finite (the caller's check); whole steps while there are any, at most RAD_SEED_STEPS */
        k.seedSteps = a >= 1.0f ? (a >= (float)RAD_SEED_STEPS ? RAD_SEED_STEPS : (uint32_t)a) : 0u;
        k.seedRest = a - (float)k.seedSteps;
        if (plan->form) { e = hipMemsetAsync(counter, 0, 4, stream); if (e != hipSuccess) return e; }
        const TbRadianceRay* r = rays; TbFloat4* o = out; uint32_t* cnt = counter;
        void* args[] = {&scene, &frame, &k, &r, &o, &cnt};
        e = hipLaunchKernel(kernel, dim3(plan->stack.grid), dim3(BLOCK), args, lds, stream); if (e != hipSuccess) return e;
    }
    if (launches) *launches = count;
    return hipGetLastError();
}

extern "C" hipError_t rad_launch_camera_rays(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W,
    uint32_t H, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t frame, TbRadianceRay* out, float* advance)
{
    if (!ds || !pf || !tg || !W || !H || W > 16384u || H > 16384u || (uint64_t)W * H > (1ull << 24)) return hipErrorInvalidValue;
    if (x0 >= x1 || y0 >= y1 || x1 > W || y1 > H || !rad_aligned16(out) || !advance) return hipErrorInvalidValue;
    const uint32_t pixels = (x1 - x0) * (y1 - y0);
    hipLaunchKernelGGL(rad_camera_rays, dim3((pixels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, *ds, *pf, *tg, W, H, x0, y0, x1, y1, frame, out, advance);
    return hipGetLastError();
}
