/* context_guides.cpp -- the guide pass of a still's denoise (include/tracerboy_hip.h tb_render_guides / tb_read_guide).
 * Seeds depend on (x, y, frame) only, so the first hits of any frames can be traced again after a render that ran at full speed, with AOVs off:
 * pt_guides (guide_kernels.hip) sums the effective albedo, the normals and the world positions of n_frames first hits per pixel into three
 * surfaces of their own.  tb_denoise reads them with option "denoise_guides" (context_denoise.cpp).  Writes nothing else: the accumulation, the
 * AOVs, the frame counter and the history stay as they are, and a render continued afterwards is the uninterrupted one. */
#include "context_internal.h"
#include "../kernels/guide_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {
const uint32_t kMaxGuideFrames = 256;

tb_context::GuideKey keyOf(const tb_context* c)
{
    tb_context::GuideKey k; memset(&k, 0, sizeof k);
    k.sceneGeneration = c->sceneGeneration; k.materialEdits = c->materialEdits; k.width = c->width; k.height = c->height;
    k.alphaTest = opt<OPT_alpha_test>(c) ? 1u : 0u; k.camera = c->camera; k.settings = c->lastSettings; k.time = c->lastTime;
    return k;
}
}

namespace tbctx {
/* scene, camera (by bits), size, history-relevant settings, time seed (by bits) and option alpha_test are those the guides were traced with */
bool guidesCurrent(const tb_context* c)
{
    if (!c->guides.valid || !c->haveLastSettings || !c->guides.sum[0].p) return false;
    const tb_context::GuideKey now = keyOf(c); const tb_context::GuideKey& k = c->guides.key;
    return now.sceneGeneration == k.sceneGeneration && now.materialEdits == k.materialEdits && now.width == k.width && now.height == k.height &&
        now.alphaTest == k.alphaTest && !memcmp(&now.camera, &k.camera, sizeof k.camera) && !historyRelevantChange(now.settings, k.settings) &&
        !memcmp(&now.time, &k.time, sizeof k.time);
}
}

extern "C" {

int tb_render_guides(tb_context* c, uint32_t firstFrame, uint32_t nFrames)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_render_guides: not supported for a multi-device group: guide surfaces are not gathered across its devices");
    return guarded(c, [&]() {
        if (c->tiles.world > 1) return fail(c, TB_E_UNSUPPORTED, "tb_render_guides: not supported with a tile assignment of world > 1: a rank holds a part of the frame");
        if (!c->hasScene) return fail(c, TB_E_INVALID, "tb_render_guides: no scene loaded");
        if (!c->width || !c->height || !c->haveLastSettings) return fail(c, TB_E_INVALID,
            "tb_render_guides: no size yet: the frame size, settings and time seed are those of the last tb_render, tb_state_load or tb_state_begin");
        if (c->rt.lastRender || c->lastSettings.RenderModeRealTime) return fail(c, TB_E_INVALID,
            "tb_render_guides: the last render was tb_render_realtime: its surface holds one frame, not an accumulation");
        if (c->lastSettings.OutputType == TB_OUTPUT_TYPE_HEATMAP || c->lastSettings.OutputType == TB_OUTPUT_TYPE_LIVE_PIXELS) return fail(c, TB_E_INVALID,
            "tb_render_guides: OutputType heat map / live pixels: the custom AOV of such a render is not the albedo");
        if (nFrames < 1 || nFrames > kMaxGuideFrames) return fail(c, TB_E_INVALID, "tb_render_guides: n_frames is 1 to " + std::to_string(kMaxGuideFrames));
        const uint32_t W = c->width, H = c->height;
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        c->guides.valid = false;
        GuidePlan plan = guide_stack_plan(c->ds.stackDepth, (uint32_t)std::max<int64_t>(0, opt<OPT_stack_overflow_max>(c)),
            (uint32_t)std::max<int64_t>(0, std::min<int64_t>(opt<OPT_stack_lds_cap>(c), 0xffff)));
        if (!plan.ok) return fail(c, TB_E_UNSUPPORTED, "tb_render_guides: traversal stack of depth " + std::to_string(c->ds.stackDepth) + " does not fit LDS; unsupported");
        HIP_TRY(guide_plan_grid(&plan, tb_persistent_grid(W, H, c->tiles)));
        for (DevBuf& b : c->guides.sum) ensure(b, bytes);
        if (plan.overflowEntries) ensure(c->guides.overflow, (size_t)plan.overflowEntries * plan.lanes * 4);
        TbDeviceScene ds = c->ds; ds.alphaTest = opt<OPT_alpha_test>(c) ? 1u : 0u;
        TbPerFrameConstants pf;
        MakeFrameConstants(c->scene, c->camera, c->lastSettings, firstFrame, c->lastTime, 0xffffffffu, 0xffffffffu, pf);
        TbDeviceTargets tg; memset(&tg, 0, sizeof tg); /* the camera constants alone */
        if (opt<OPT_camera_constants>(c) != 0) cameraConstants(pf, W, H, tg);
        HIP_TRY(hipEventRecord(c->guides.ev[0].create(), c->stream));
        HIP_TRY(guide_launch(c->stream, &ds, &pf, &tg, W, H, firstFrame, nFrames, &c->tiles, &plan, plan.overflowEntries ? (uint32_t*)c->guides.overflow.p : nullptr,
            (TbFloat4*)c->guides.sum[0].p, (TbFloat4*)c->guides.sum[1].p, (TbFloat4*)c->guides.sum[2].p));
        HIP_TRY(hipEventRecord(c->guides.ev[1].create(), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (hipEventElapsedTime(&c->guides.lastMs, c->guides.ev[0], c->guides.ev[1]) != hipSuccess) c->guides.lastMs = 0.0f;
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        c->guides.key = keyOf(c); c->guides.valid = true; c->guides.lastOverflow = plan.overflowEntries;
        if (c->dn.mode != 0) c->dn.valid = false; /* a denoised surface made of the guides before these */
        return TB_OK;
    });
}

int tb_read_guide(tb_context* c, int which, float* rgba)
{
    return guarded(c, [&]() {
        if (!rgba || which < 0 || which > 2) return fail(c, TB_E_INVALID, "tb_read_guide: which is 0 (albedo), 1 (normal) or 2 (position)");
        if (!guidesCurrent(c)) return fail(c, TB_E_INVALID, "tb_read_guide: no valid guide surfaces: call tb_render_guides");
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(rgba, c->guides.sum[which].p, (size_t)c->width * c->height * sizeof(TbFloat4), hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
