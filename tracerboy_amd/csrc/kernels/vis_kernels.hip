/* vis_kernels.hip -- the path inspector (include/tracerboy_hip.h tb_record_paths / tb_visualize_rays).
 *
 * pt_paths: a sample's seed depends on (x, y, frame) alone, so the complete paths of any pixel can be traced again after a render that ran at full
 * speed.  One lane per frame of ONE pixel, full feature set like pt_guides (guide_kernels.hip), the step functions in pt_stream's order for a lane
 * that never waits (pt_stream.inc:51-118): walk the pending ray, then path_on_closest / path_on_shadow / path_on_sss by the path's state, then
 * path_scatter.  What the reference's recorder keeps (RayGenCommon.h:600-630, called at kernel.glsl:1339 and :1350) is the closest-hit ray of every
 * bounce i > 0 that gets past the throughput early-out of :1319-1326: path_on_closest opens with that early-out, so the test is made here, on the
 * same throughput, before the call.  Feelers and interior steps are not recorded.
 * The kernel runs twice.  The first run counts: frames[f] = the sample's sum (o0..o3 of pt_stream.inc:86-91), its flags and the number of its rays.
 * vis_scan then gives every frame its place in the ray buffer -- a prefix sum over the frames behind the rays the buffer holds already, cut at the
 * cap -- and the second run stores each ray at that place + its index within the path.  The buffer's order is therefore frame, then bounce.
 *
 * vis_overlay: the reference's VisualizeRaysCS.hlsl:133-226 from its formulas -- a camera ray per pixel (no half-pixel offset, uv.y flipped), and per
 * stored ray a cylinder (iCylinder :34-77, its normal :80-88) and, for rays that hit, a capped cone over the last fifth (iCappedCone :92-131); the
 * nearest of them in front of the occluder is blended over the picture at alpha 0.75.  IEEE fp32, one operation per line of the reference's
 * expressions read left to right, unfused (the build's -ffp-contract=off); dot = (x x' + y y') + z z', normalize = v / sqrt(dot), lerp = a + s (b - a).
 * The divisions by zero the reference has (k2 == 0: a view ray parallel to the cylinder; bard == 0) are kept: their infinities and NaNs fail the
 * comparisons that follow.  tests/visualize_ref.py restates it in numpy.
 * A wave covers an 8 x 8 tile, a workgroup a 16 x 16 region.  The ray loop is uniform over the wave; TB_VIS_RAYS_IN_LDS chooses how the records
 * reach it: 0 = read from memory with wave-uniform addresses, which the compiler turns into scalar loads (the form that stayed: 4.2 against
 * 4.7 ms for 1024 rays over a 1920 x 1080 picture, 0.29 against 0.32 ms for 64), 1 = staged in LDS once per workgroup (32 KB, five workgroups a CU,
 * eight ds_read dwords per lane and ray).  scripts/visualize_timing.py measures the two; DESIGN.md section 19 has the figures. */
#include <hip/hip_runtime.h>
#include "pt_common.hpp"
#include "pt_launch.h"
#include "vis_launch.h"

#ifndef TB_VIS_RAYS_IN_LDS
#define TB_VIS_RAYS_IN_LDS 0
#endif

namespace {

template <bool HYBRID>
__global__ __launch_bounds__(BLOCK) void pt_paths(TbDeviceScene ds, TbPerFrameConstants pf, TbDeviceTargets tg, uint32_t W, uint32_t H, uint32_t x, uint32_t y,
    uint32_t firstFrame, uint32_t numFrames, TbPathFrame* __restrict__ frames, TbVisualizerRay* __restrict__ rays /* null: the counting run */)
{
    constexpr uint32_t F = FEAT_ALL;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SceneRefs sc;
    make_refs<false>(sc, ds, nullptr);
    uint32_t* stack = (uint32_t*)smem + threadIdx.x;
    uint32_t* const overflow = HYBRID ? ds.stackOverflow + (size_t)blockIdx.x * BLOCK + threadIdx.x : nullptr;
    const uint32_t f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= numFrames) return;
    const uint32_t frame = firstFrame + f;
    /* the storing run: the frame's place in the buffer and how many of its rays have room there (vis_scan) */
    uint32_t place = 0, room = 0;
    if (rays) { const TbPathFrame fr = frames[f]; place = fr.first_ray; room = place == 0xffffffffu ? 0u : TB_MAX_VISUALIZER_RAYS - place; }
    uint32_t numRays = 0;
    Path p;
    path_begin<F>(p, ds, pf, frame, W, H, x, y, &tg);
    while (p.state != ST_DONE) {
        /* the pending ray: the bounce ray, a feeler or a step of an interior walk */
        float travel = 0.0f;
        if (p.state == ST_SSS) travel = sss_travel(p, pf);
        Hit h; uint32_t nb = 0, nt = 0;
        bool isHit;
        if (ds.numInstances) isHit = traverse_instanced<false, true, HYBRID>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, overflow);
        else isHit = traverse<false, true, HYBRID, false, false, true>(sc, ds, p.ro, p.rd, h, stack, BLOCK, nb, nt, nullptr, overflow);
        if (p.state == ST_EXTEND) {
            /* kernel.glsl:1337-1351 behind :1319-1326 */
            if (p.bounce > 0 && !(p.T.x < EPSILON && p.T.y < EPSILON && p.T.z < EPSILON)) {
                if (numRays < room) {
                    TbVisualizerRay r;
                    r.Origin[0] = p.ro.x; r.Origin[1] = p.ro.y; r.Origin[2] = p.ro.z; r.Direction[0] = p.rd.x; r.Direction[1] = p.rd.y; r.Direction[2] = p.rd.z;
                    r.HitT = isHit ? h.t : -1.0f; r.BounceCount = (float)p.bounce;
                    rays[place + numRays] = r;
                }
                numRays++;
            }
            path_on_closest<F>(p, sc, ds, pf, isHit, h);
        } else if (p.state == ST_SHADOW) path_on_shadow<F>(p, sc, ds, pf, isHit, h);
        else path_on_sss(p, sc, pf, isHit, h, travel);
        if (p.state == ST_SCATTER) path_scatter<F>(p, pf);
    }
    if (rays) return;
    /* kernel.glsl:1910-1920 + RayGenCommon.h:704-727, as pt_stream.inc:86-95 */
    tb3 color = p.L;
    if (pf.FireflyClampValue >= EPSILON) color = tb3_min(color, tb3_splat(pf.FireflyClampValue));
    const float s0 = color.x * p.weight, s1 = color.y * p.weight, s2 = color.z * p.weight, s3 = p.weight;
    const bool ok = !(tb_isnan(s0) || tb_isnan(s1) || tb_isnan(s2) || tb_isnan(s3));
    float o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    if (ok) { o0 += s0; o1 += s1; o2 += s2; o3 += s3; }
    const float coin = rnd(p.seed, pf.Time);
    TbPathFrame out;
    out.sum[0] = o0; out.sum[1] = o1; out.sum[2] = o2; out.sum[3] = o3;
    out.frame = frame; out.first_ray = 0xffffffffu; out.num_rays = numRays;
    out.flags = ((frame == 0 || coin < 0.5f) ? TB_PATH_JITTERED : 0u) | (ok ? 0u : TB_PATH_REJECTED);
    frames[f] = out;
}

/* One workgroup: thread t owns the frames [16 t, 16 t + 16); their ray counts summed, the 256 sums scanned by thread 0, then each frame's place.
 * A frame whose rays do not all fit is marked, one none of whose rays fit (or that has none) keeps first_ray = 0xffffffff. */
__global__ __launch_bounds__(BLOCK) void vis_scan(TbPathFrame* __restrict__ frames, uint32_t numFrames, uint32_t base, uint32_t* __restrict__ rayBuffer,
    uint32_t* __restrict__ totals)
{
    static_assert(VIS_MAX_PATH_FRAMES == 16u * BLOCK, "sixteen frames a thread");
    __shared__ uint32_t part[BLOCK + 1];
    const uint32_t t = threadIdx.x, f0 = t * 16u;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 16u; i++) if (f0 + i < numFrames) sum += frames[f0 + i].num_rays;
    part[t + 1] = sum;
    __syncthreads();
    if (t == 0) { part[0] = 0; for (uint32_t i = 1; i <= BLOCK; i++) part[i] += part[i - 1]; }
    __syncthreads();
    uint64_t at = (uint64_t)base + part[t];
    for (uint32_t i = 0; i < 16u; i++) {
        if (f0 + i >= numFrames) break;
        const uint32_t n = frames[f0 + i].num_rays;
        const uint32_t room = at < TB_MAX_VISUALIZER_RAYS ? TB_MAX_VISUALIZER_RAYS - (uint32_t)at : 0u;
        if (n && room) frames[f0 + i].first_ray = (uint32_t)at;
        if (n > room) frames[f0 + i].flags |= TB_PATH_TRUNCATED;
        at += n;
    }
    if (t == 0) {
        const uint64_t all = (uint64_t)base + part[BLOCK];
        const uint32_t count = all < TB_MAX_VISUALIZER_RAYS ? (uint32_t)all : TB_MAX_VISUALIZER_RAYS;
        rayBuffer[0] = count; totals[0] = count; totals[1] = part[BLOCK];
    }
}

/* ---- the overlay ---------------------------------------------------------------------------------------------------------------------------- */
struct V3 { float x, y, z; };
TBD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
TBD V3 vsub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
TBD V3 vadd(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
TBD V3 vmul(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
TBD V3 vdiv(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
TBD float vdot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
TBD V3 vnormalize(V3 a) { return vdiv(a, tb_sqrt(vdot(a, a))); }

/* iCylinder, VisualizeRaysCS.hlsl:34-77: the distance along (ro, rd) to the capped cylinder pa..pb of radius ra, -1 without a hit (only .x is read) */
TBD float vis_cylinder(V3 ro, V3 rd, V3 pa, V3 pb, float ra)
{
    const V3 ba = vsub(pb, pa), oc = vsub(ro, pa);
    const float baba = vdot(ba, ba), bard = vdot(ba, rd), baoc = vdot(ba, oc);
    const float k2 = baba - bard * bard;
    const float k1 = baba * vdot(oc, rd) - baoc * bard;
    const float k0 = (baba * vdot(oc, oc) - baoc * baoc) - (ra * ra) * baba;
    float h = k1 * k1 - k2 * k0;
    if (h < 0.0f) return -1.0f;
    h = tb_sqrt(h);
    float t = (-k1 - h) / k2;
    const float y = baoc + t * bard;
    if (y > 0.0f && y < baba) return t;                 /* body */
    t = ((y < 0.0f ? 0.0f : baba) - baoc) / bard;       /* caps */
    if (tb_abs(k1 + k2 * t) < h) return t;
    return -1.0f;
}

/* iCappedCone, :92-131: radius ra at pa, rb at pb */
TBD float vis_cone(V3 ro, V3 rd, V3 pa, V3 pb, float ra, float rb)
{
    const V3 ba = vsub(pb, pa), oa = vsub(ro, pa), ob = vsub(ro, pb);
    const float m0 = vdot(ba, ba), m1 = vdot(oa, ba), m2 = vdot(ob, ba), m3 = vdot(rd, ba);
    if (m1 < 0.0f) { const V3 v = vsub(vmul(oa, m3), vmul(rd, m1)); if (vdot(v, v) < ((ra * ra) * m3) * m3) return -m1 / m3; }
    else if (m2 > 0.0f) { const V3 v = vsub(vmul(ob, m3), vmul(rd, m2)); if (vdot(v, v) < ((rb * rb) * m3) * m3) return -m2 / m3; }
    const float m4 = vdot(rd, oa), m5 = vdot(oa, oa), rr = ra - rb, hy = m0 + rr * rr;
    const float k2 = m0 * m0 - (m3 * m3) * hy;
    const float k1 = ((m0 * m0) * m4 - (m1 * m3) * hy) + (m0 * ra) * ((rr * m3) * 1.0f);
    const float k0 = ((m0 * m0) * m5 - (m1 * m1) * hy) + (m0 * ra) * ((rr * m1) * 2.0f - m0 * ra);
    const float h = k1 * k1 - k2 * k0;
    if (h < 0.0f) return -1.0f;
    const float t = (-k1 - tb_sqrt(h)) / k2;
    const float y = m1 + t * m3;
    if (y > 0.0f && y < m0) return t;
    return -1.0f;
}

__global__ __launch_bounds__(BLOCK) void vis_overlay(TbVisualizeConstants k, const TbVisualizerRay* __restrict__ rays, uint32_t numRays,
    const TbFloat4* __restrict__ scene, const TbFloat4* __restrict__ worldPos, const TbFloat4* __restrict__ hits, TbFloat4* __restrict__ out,
    uint32_t* __restrict__ out8)
{
    const uint32_t W = k.ResolutionX, H = k.ResolutionY, groupsX = (W + 15u) / 16u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = (blockIdx.x % groupsX) * 16u + (wave & 1u) * 8u + (lane & 7u), y = (blockIdx.x / groupsX) * 16u + (wave >> 1) * 8u + (lane >> 3);
#if TB_VIS_RAYS_IN_LDS
    __shared__ __attribute__((aligned(16))) TbVisualizerRay staged[TB_MAX_VISUALIZER_RAYS];
    for (uint32_t i = threadIdx.x; i < numRays * 2u; i += BLOCK) ((uint4*)staged)[i] = ((const uint4*)rays)[i];
    __syncthreads();
#endif
    if (x >= W || y >= H) return;
    const size_t pix = (size_t)y * W + x;
    const TbFloat4 sceneColor = scene[pix];
    /* :138-149 */
    const float resX = (float)W, resY = (float)H;
    const float u = (float)x / resX, v = 1.0f - (float)y / resY;
    const float aspect = resX / resY;
    const V3 camPos = v3(k.CameraPosition[0], k.CameraPosition[1], k.CameraPosition[2]);
    const V3 view = vnormalize(vsub(v3(k.CameraLookAt[0], k.CameraLookAt[1], k.CameraLookAt[2]), camPos));
    const V3 focal = vsub(camPos, vmul(view, k.FocalLength));
    const float lensWidth = k.LensHeight * aspect;
    V3 ro = camPos;
    ro = vadd(ro, vdiv(vmul(vmul(v3(k.CameraRight[0], k.CameraRight[1], k.CameraRight[2]), u * 2.0f - 1.0f), lensWidth), 2.0f));
    ro = vadd(ro, vdiv(vmul(vmul(v3(k.CameraUp[0], k.CameraUp[1], k.CameraUp[2]), v * 2.0f - 1.0f), k.LensHeight), 2.0f));
    const V3 rd = vnormalize(vsub(ro, focal));
    /* :151-156 */
    float occluder = -1.0f;
    if (worldPos) {
        const TbFloat4 w4 = worldPos[pix];
        V3 wp = v3(w4.x, w4.y, w4.z);
        if (hits) { const float n = hits[pix].w; wp = n > 0.0f ? vdiv(wp, n) : v3(0.0f, 0.0f, 0.0f); }
        if (tb_abs(wp.x) > 0.0001f || tb_abs(wp.y) > 0.0001f || tb_abs(wp.z) > 0.0001f) { const V3 d = vsub(wp, ro); occluder = tb_sqrt(vdot(d, d)); }
    }
    /* :158-223 */
    V3 visColor = v3(0.0f, 0.0f, 0.0f); float visAlpha = 0.0f;
    float closest = 9999999.9f;
    const uint32_t have = numRays < TB_MAX_VISUALIZER_RAYS ? numRays : TB_MAX_VISUALIZER_RAYS;
    const uint32_t count = k.RayCount < 0 ? 0u : ((uint32_t)k.RayCount < have ? (uint32_t)k.RayCount : have);
    for (uint32_t i = 0; i < count; i++) {
#if TB_VIS_RAYS_IN_LDS
        const TbVisualizerRay r = staged[i];
#else
        const TbVisualizerRay r = rays[i];
#endif
        float bounce = r.BounceCount;
        const V3 color = bounce < 0.0f ? v3(0.0f, 0.0f, 1.0f) : (bounce <= 1.1f ? v3(0.0f, 1.0f, 0.0f) : v3(1.0f, 1.0f, 0.0f));
        const V3 start = v3(r.Origin[0], r.Origin[1], r.Origin[2]), dir = v3(r.Direction[0], r.Direction[1], r.Direction[2]);
        float length = r.HitT > 0.0f ? r.HitT : 9999999.9f;
        bounce = tb_abs(bounce);
        if (bounce > k.RayDepth) continue;
        length = length * tb_min(1.0f, k.RayDepth - bounce);
        const V3 end = vadd(start, vmul(dir, length));
        float t = vis_cylinder(ro, rd, start, end, k.CylinderRadius);
        if (t > 0.0f && t < closest && (occluder < 0.0f || t < occluder)) {
            closest = t;
            /* nCylinder :80-88 */
            const V3 pa = vsub(vadd(ro, vmul(rd, t)), start), ba = vsub(end, start);
            const float baba = vdot(ba, ba), paba = vdot(pa, ba);
            const V3 n = vdiv(vsub(pa, vdiv(vmul(ba, paba), baba)), k.CylinderRadius);
            const float s = tb_abs(vdot(n, rd));
            visColor = v3(0.2f + s * (color.x - 0.2f), 0.2f + s * (color.y - 0.2f), 0.2f + s * (color.z - 0.2f));
            visAlpha = 0.75f;
        }
        if (r.HitT > 0.0f) {
            t = vis_cone(ro, rd, vadd(start, vmul(dir, length * 0.8f)), end, k.CylinderRadius * 10.0f, k.CylinderRadius);
            if (t > 0.0f && t < closest && (occluder < 0.0f || t < occluder)) { closest = t; visColor = color; visAlpha = 0.75f; }
        }
    }
    /* :225 */
    const TbFloat4 o = TbFloat4{sceneColor.x + visAlpha * (visColor.x - sceneColor.x), sceneColor.y + visAlpha * (visColor.y - sceneColor.y),
        sceneColor.z + visAlpha * (visColor.z - sceneColor.z), sceneColor.w};
    out[pix] = o;
    if (out8) { /* the output stage's R8G8B8A8_UNORM store (post_kernels.hip): clamp, scale, + 0.5, truncate */
        const uint32_t r8 = (uint32_t)(tb_saturate(o.x) * 255.0f + 0.5f), g8 = (uint32_t)(tb_saturate(o.y) * 255.0f + 0.5f),
            b8 = (uint32_t)(tb_saturate(o.z) * 255.0f + 0.5f);
        out8[pix] = r8 | (g8 << 8) | (b8 << 16) | 0xff000000u;
    }
}

bool vis_aligned(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }
size_t vis_lds(const GuidePlan& plan) { return (size_t)plan.ldsEntries * BLOCK * 4; }

template <class K> hipError_t vis_run_paths(K kernel, hipStream_t stream, const TbDeviceScene& scene, const TbPerFrameConstants& pf, const TbDeviceTargets& tg,
    uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t firstFrame, uint32_t numFrames, const GuidePlan& plan, uint32_t* rayBuffer, uint32_t base,
    TbPathFrame* frames, uint32_t* totals)
{
    const size_t lds = vis_lds(plan);
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(plan.grid), dim3(BLOCK), lds, stream, scene, pf, tg, W, H, x, y, firstFrame, numFrames, frames, (TbVisualizerRay*)nullptr);
    hipLaunchKernelGGL(vis_scan, dim3(1), dim3(BLOCK), 0, stream, frames, numFrames, base, rayBuffer, totals);
    hipLaunchKernelGGL(kernel, dim3(plan.grid), dim3(BLOCK), lds, stream, scene, pf, tg, W, H, x, y, firstFrame, numFrames, frames,
        (TbVisualizerRay*)(rayBuffer + 1));
    return hipGetLastError();
}

} // namespace

extern "C" hipError_t vis_plan_grid(GuidePlan* plan, uint32_t numFrames)
{
    if (!plan || !plan->ok || !plan->ldsEntries || !numFrames || numFrames > VIS_MAX_PATH_FRAMES) return hipErrorInvalidValue;
    plan->grid = (numFrames + BLOCK - 1u) / BLOCK;
    plan->lanes = plan->grid * BLOCK;
    return hipSuccess;
}

extern "C" hipError_t vis_launch_paths(hipStream_t stream, const TbDeviceScene* ds, const TbPerFrameConstants* pf, const TbDeviceTargets* tg, uint32_t W, uint32_t H,
    uint32_t x, uint32_t y, uint32_t firstFrame, uint32_t numFrames, const GuidePlan* plan, uint32_t* overflow, uint32_t* rayBuffer, uint32_t base,
    TbPathFrame* frames, uint32_t* totals)
{
    if (!ds || !pf || !tg || !plan || !plan->ok || !W || !H || W > 16384u || H > 16384u || x >= W || y >= H) return hipErrorInvalidValue;
    if (!numFrames || numFrames > VIS_MAX_PATH_FRAMES || plan->grid != (numFrames + BLOCK - 1u) / BLOCK || plan->lanes != plan->grid * BLOCK) return hipErrorInvalidValue;
    if (plan->ldsEntries + plan->overflowEntries < ds->stackDepth) return hipErrorInvalidValue; /* a stack shallower than the tree */
    if ((plan->overflowEntries != 0) != (overflow != nullptr)) return hipErrorInvalidValue;
    if (!rayBuffer || !vis_aligned(rayBuffer + 1) || !vis_aligned(frames) || !totals || base > TB_MAX_VISUALIZER_RAYS) return hipErrorInvalidValue;
    TbDeviceScene scene = *ds; /* the scene as this launch walks it: layout B, this launch's split of the stack */
    scene.nodesC = nullptr; scene.stackDepth = plan->ldsEntries; scene.stackOverflow = overflow; scene.stackOverflowLanes = overflow ? plan->lanes : 0u;
    if (overflow) return vis_run_paths(pt_paths<true>, stream, scene, *pf, *tg, W, H, x, y, firstFrame, numFrames, *plan, rayBuffer, base, frames, totals);
    return vis_run_paths(pt_paths<false>, stream, scene, *pf, *tg, W, H, x, y, firstFrame, numFrames, *plan, rayBuffer, base, frames, totals);
}

extern "C" hipError_t vis_launch_overlay(hipStream_t stream, const TbVisualizeConstants* k, const TbVisualizerRay* rays, uint32_t numRays, const TbFloat4* scene,
    const TbFloat4* worldPos, const TbFloat4* hits, TbFloat4* out, uint32_t* out8)
{
    if (!k || !k->ResolutionX || !k->ResolutionY || (uint64_t)k->ResolutionX * k->ResolutionY > (1ull << 24) || !scene || !out) return hipErrorInvalidValue;
    if (numRays > TB_MAX_VISUALIZER_RAYS || (numRays && !vis_aligned(rays)) || (hits && !worldPos)) return hipErrorInvalidValue;
    const uint32_t groups = ((k->ResolutionX + 15u) / 16u) * ((k->ResolutionY + 15u) / 16u);
    hipLaunchKernelGGL(vis_overlay, dim3(groups), dim3(BLOCK), 0, stream, *k, rays, numRays, scene, worldPos, hits, out, out8);
    return hipGetLastError();
}
