/* context_visualize.cpp -- the path inspector (include/tracerboy_hip.h tb_record_paths / tb_read_paths / tb_clear_paths /
 * tb_visualize_rays / tb_visualize_constants / tb_run_visualize_rays): the reference's ray visualiser.  Seeds depend on (x, y, frame) only, so the
 * paths of any pixel can be traced again after a render that ran at full speed: pt_paths (vis_kernels.hip) appends their bounce rays to the
 * reference's ray buffer, in frame and bounce order, and vis_overlay draws the buffer over the post-processed picture as VisualizeRaysCS does.
 * Writes nothing else: the accumulation, the AOVs, the guides, the post output, the frame counter and the history stay as they are. */
#include "context_internal.h"
#include "../kernels/vis_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

const size_t kRayBufferLead = 12; /* bytes in front of the count word: the records behind it are 16-B aligned */
uint32_t* rayCountWord(const tb_context* c) { return (uint32_t*)((uint8_t*)c->vis.rays.p + kRayBufferLead); }

/* TracerBoy.cpp:3216-3228 */
void makeConstants(const tb_camera& cam, uint32_t W, uint32_t H, const tb_visualize_settings& s, TbVisualizeConstants& k)
{
    memset(&k, 0, sizeof k);
    k.ResolutionX = W; k.ResolutionY = H; k.CylinderRadius = s.RayWidth; k.RayDepth = s.RayDepth; k.RayCount = s.RayCount > 0 ? s.RayCount : 999999;
    k.FocalLength = cam.FocalDistance; k.LensHeight = cam.LensHeight;
    for (int i = 0; i < 3; i++) { k.CameraPosition[i] = cam.Position[i]; k.CameraLookAt[i] = cam.LookAt[i]; k.CameraRight[i] = cam.Right[i]; k.CameraUp[i] = cam.Up[i]; }
}

} // namespace

extern "C" {

void tb_default_visualize_settings(tb_visualize_settings* o) /* TracerBoy.h:303-306 */
{
    if (!o) return;
    o->RayWidth = 0.01f; o->RayDepth = 10.0f; o->RayCount = 0;
}

int tb_visualize_constants(const tb_camera* cam, uint32_t W, uint32_t H, const tb_visualize_settings* settings, TbVisualizeConstants* out)
{
    if (!cam || !out || !W || !H) return TB_E_INVALID;
    tb_visualize_settings s; if (settings) s = *settings; else tb_default_visualize_settings(&s);
    makeConstants(*cam, W, H, s, *out);
    return TB_OK;
}

int tb_record_paths(tb_context* c, uint32_t x, uint32_t y, uint32_t firstFrame, uint32_t nFrames, TbPathFrame* frames, uint32_t* raysTotal)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_record_paths: not supported for a multi-device group: the pixel's tile may lie on another device");
    return guarded(c, [&]() {
        if (c->tiles.world > 1) return fail(c, TB_E_UNSUPPORTED, "tb_record_paths: not supported with a tile assignment of world > 1: a rank holds a part of the frame");
        if (!c->hasScene) return fail(c, TB_E_INVALID, "tb_record_paths: no scene loaded");
        if (!c->width || !c->height || !c->haveLastSettings) return fail(c, TB_E_INVALID,
            "tb_record_paths: no size yet: the frame size, settings and time seed are those of the last tb_render, tb_state_load or tb_state_begin");
        if (c->rt.lastRender || c->lastSettings.RenderModeRealTime) return fail(c, TB_E_INVALID,
            "tb_record_paths: the last render was tb_render_realtime: its surface holds one frame, not an accumulation");
        if (nFrames < 1 || nFrames > VIS_MAX_PATH_FRAMES) return fail(c, TB_E_INVALID, "tb_record_paths: n_frames is 1 to " + std::to_string(VIS_MAX_PATH_FRAMES));
        const uint32_t W = c->width, H = c->height;
        if (x >= W || y >= H) return fail(c, TB_E_INVALID, "tb_record_paths: pixel (" + std::to_string(x) + ", " + std::to_string(y) + ") is outside the " +
            std::to_string(W) + " x " + std::to_string(H) + " frame");
        GuidePlan plan = guide_stack_plan(c->ds.stackDepth, (uint32_t)std::max<int64_t>(0, opt<OPT_stack_overflow_max>(c)),
            (uint32_t)std::max<int64_t>(0, std::min<int64_t>(opt<OPT_stack_lds_cap>(c), 0xffff)));
        if (!plan.ok) return fail(c, TB_E_UNSUPPORTED, "tb_record_paths: traversal stack of depth " + std::to_string(c->ds.stackDepth) + " does not fit LDS; unsupported");
        HIP_TRY(vis_plan_grid(&plan, nFrames));
        const size_t rayBytes = kRayBufferLead + 4 + (size_t)TB_MAX_VISUALIZER_RAYS * sizeof(TbVisualizerRay);
        if (c->vis.rays.bytes != rayBytes) { ensure(c->vis.rays, rayBytes); c->vis.stored = 0; }
        if (plan.overflowEntries) ensure(c->vis.overflow, (size_t)plan.overflowEntries * plan.lanes * 4);
        const DevBuf dFrames = scratch((size_t)nFrames * sizeof(TbPathFrame)), dTotals = scratch(8);
        TbDeviceScene ds = c->ds; ds.alphaTest = opt<OPT_alpha_test>(c) ? 1u : 0u;
        TbPerFrameConstants pf;
        MakeFrameConstants(c->scene, c->camera, c->lastSettings, firstFrame, c->lastTime, 0xffffffffu, 0xffffffffu, pf);
        TbDeviceTargets tg; memset(&tg, 0, sizeof tg); /* the camera constants alone */
        if (opt<OPT_camera_constants>(c) != 0) cameraConstants(pf, W, H, tg);
        HIP_TRY(hipEventRecord(c->vis.evPaths[0].create(), c->stream));
        HIP_TRY(vis_launch_paths(c->stream, &ds, &pf, &tg, W, H, x, y, firstFrame, nFrames, &plan, plan.overflowEntries ? (uint32_t*)c->vis.overflow.p : nullptr,
            rayCountWord(c), c->vis.stored, (TbPathFrame*)dFrames.p, (uint32_t*)dTotals.p));
        HIP_TRY(hipEventRecord(c->vis.evPaths[1].create(), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (hipEventElapsedTime(&c->vis.lastPathsMs, c->vis.evPaths[0], c->vis.evPaths[1]) != hipSuccess) c->vis.lastPathsMs = 0.0f;
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        uint32_t totals[2] = {0, 0};
        HIP_TRY(hipMemcpy(totals, dTotals.p, sizeof totals, hipMemcpyDeviceToHost));
        c->vis.stored = std::min(totals[0], TB_MAX_VISUALIZER_RAYS);
        if (raysTotal) *raysTotal = totals[1];
        copyBack(frames, dFrames);
        return TB_OK;
    });
}

int tb_clear_paths(tb_context* c)
{
    if (!c) return TB_E_INVALID;
    c->vis.stored = 0;
    return TB_OK;
}

int tb_read_paths(tb_context* c, TbVisualizerRay* rays, uint32_t capacity, uint32_t* count)
{
    return guarded(c, [&]() {
        if (!count && !rays) return fail(c, TB_E_INVALID, "tb_read_paths: both pointers are null");
        const uint32_t stored = c->vis.rays.p ? c->vis.stored : 0u, n = std::min(stored, capacity);
        if (count) *count = stored;
        if (rays && n) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipMemcpy(rays, rayCountWord(c) + 1, (size_t)n * sizeof(TbVisualizerRay), hipMemcpyDeviceToHost));
        }
        return TB_OK;
    });
}

int tb_run_visualize_rays(tb_context* c, const TbVisualizeConstants* k, const TbVisualizerRay* rays, uint32_t nRays, const float* scene, const float* worldPos,
    float* out)
{
    return guarded(c, [&]() {
        if (!k || !scene || !out || (nRays && !rays)) return fail(c, TB_E_INVALID, "tb_run_visualize_rays: null pointer");
        if (const char* why = surfaceRefusal(k->ResolutionX, k->ResolutionY)) return fail(c, TB_E_INVALID, std::string("tb_run_visualize_rays: ") + why);
        if (nRays > TB_MAX_VISUALIZER_RAYS) return fail(c, TB_E_INVALID, "tb_run_visualize_rays: more than " + std::to_string(TB_MAX_VISUALIZER_RAYS) + " rays");
        const size_t bytes = (size_t)k->ResolutionX * k->ResolutionY * sizeof(TbFloat4);
        const DevBuf dScene = staged(scene, bytes), dOut = scratch(bytes);
        DevBuf dRays, dWorld;
        if (nRays) dRays = staged(rays, (size_t)nRays * sizeof(TbVisualizerRay));
        if (worldPos) dWorld = staged(worldPos, bytes);
        HIP_TRY(vis_launch_overlay(c->stream, k, (const TbVisualizerRay*)dRays.p, nRays, (const TbFloat4*)dScene.p, (const TbFloat4*)dWorld.p, nullptr,
            (TbFloat4*)dOut.p, nullptr));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_visualize_rays(tb_context* c, const tb_visualize_settings* settings, float* rgbaF32, uint8_t* rgba8)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_visualize_rays: not supported for a multi-device group: paths are not recorded across its devices");
    return guarded(c, [&]() {
        if (c->tiles.world > 1) return fail(c, TB_E_UNSUPPORTED, "tb_visualize_rays: not supported with a tile assignment of world > 1: a rank holds a part of the frame");
        const uint32_t W = c->width, H = c->height;
        const size_t px = (size_t)W * H;
        if (!px || !c->postOut.p || c->postOut.bytes != px * sizeof(TbFloat4)) return fail(c, TB_E_INVALID,
            "tb_visualize_rays: no post-processed picture of the rendered size: call tb_post_process first");
        tb_visualize_settings s; if (settings) s = *settings; else tb_default_visualize_settings(&s);
        TbVisualizeConstants k;
        makeConstants(c->camera, W, H, s, k);
        /* the occluder: the last frame's world positions where its AOVs exist (as tb_denoise judges that), else the guide pass's mean, else none */
        const TbFloat4* world = nullptr; const TbFloat4* hits = nullptr;
        c->vis.depthSource = 0;
        if (c->samplesRendered > c->firstFrame && opt<OPT_aov>(c) && c->callCount >= c->dn.aovStaleUntilCall && !c->rt.lastRender) {
            const DevBuf& positions = c->aov[TB_AOV_WORLD_POSITION0 + ((c->samplesRendered - 1u) % 2u)];
            if (positions.p && positions.bytes == px * sizeof(TbFloat4)) { world = (const TbFloat4*)positions.p; c->vis.depthSource = 1; }
        }
        if (!world && guidesCurrent(c) && c->guides.sum[2].bytes == px * sizeof(TbFloat4)) {
            world = (const TbFloat4*)c->guides.sum[2].p; hits = (const TbFloat4*)c->guides.sum[1].p; c->vis.depthSource = 2;
        }
        const uint32_t stored = c->vis.rays.p ? c->vis.stored : 0u;
        ensure(c->vis.out, px * sizeof(TbFloat4)); ensure(c->vis.out8, px * 4);
        HIP_TRY(hipEventRecord(c->vis.evOverlay[0].create(), c->stream));
        HIP_TRY(vis_launch_overlay(c->stream, &k, stored ? (const TbVisualizerRay*)(rayCountWord(c) + 1) : nullptr, stored, (const TbFloat4*)c->postOut.p, world, hits,
            (TbFloat4*)c->vis.out.p, (uint32_t*)c->vis.out8.p));
        HIP_TRY(hipEventRecord(c->vis.evOverlay[1].create(), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (hipEventElapsedTime(&c->vis.lastOverlayMs, c->vis.evOverlay[0], c->vis.evOverlay[1]) != hipSuccess) c->vis.lastOverlayMs = 0.0f;
        if (rgbaF32) HIP_TRY(hipMemcpy(rgbaF32, c->vis.out.p, px * sizeof(TbFloat4), hipMemcpyDeviceToHost));
        if (rgba8) HIP_TRY(hipMemcpy(rgba8, c->vis.out8.p, px * 4, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
