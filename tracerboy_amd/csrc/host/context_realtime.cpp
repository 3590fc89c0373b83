/* context_realtime.cpp -- the real-time chain (include/tracerboy_hip.h tb_render_realtime / tb_read_realtime): one path-traced frame, TAA on the
 * indirect lighting, the a-trous filter, the albedo composite, TAA (the reference's TracerBoy.cpp:3060-3160).  The a-trous pass loop is here for
 * its second caller too, tb_denoise (context_denoise.cpp); so are the test hooks that run the kernels of rt_kernels.hip on host surfaces. */
#include "context_internal.h"

using namespace tbhost;
using namespace tbctx;

int tbctx::runAtrousPasses(hipStream_t stream, uint32_t W, uint32_t H, uint32_t n, const TbFloat4* first, const TbFloat4* normals, const TbFloat4* positions,
    DevBuf (&pingPong)[2], const tb_denoiser_settings& dn, uint32_t frameCount)
{
    const TbFloat4* in = first;
    for (uint32_t i = 0; i < n; i++) {
        TbDenoiserConstants k{};
        k.ResolutionX = W; k.ResolutionY = H; k.OffsetMultiplier = 1u << i; k.GlobalFrameCount = frameCount;
        k.NormalWeightingExponential = dn.NormalWeightingExponential; k.IntersectionPositionWeightingMultiplier = dn.IntersectPositionWeightingMultiplier;
        k.LumaWeightingMultiplier = dn.LuminanceWeightingMultiplier;
        TbFloat4* out = (TbFloat4*)pingPong[i & 1u].p;
        HIP_TRY(rt_launch_denoise(stream, &k, in, normals, positions, first, out));
        in = out;
    }
    return n ? (int)((n - 1u) & 1u) : -1;
}

extern "C" {

void tb_default_denoiser_settings(tb_denoiser_settings* o) /* TracerBoy.h:338-344 */
{
    if (!o) return;
    o->Enabled = 1; o->IntersectPositionWeightingMultiplier = 1.0f; o->NormalWeightingExponential = 128.0f; o->LuminanceWeightingMultiplier = 4.0f;
        o->WaveletIterations = 5;
}

/* One frame of RenderMode::RealTime: path trace 1 spp (IsRealTime: per-frame output, demodulated albedo, AOVs), then
 * TracerBoy.cpp:3060-3160: TAA on the indirect lighting (with luminance moments), a-trous denoiser, albedo composite, TAA. */
int tb_render_realtime(tb_context* c, uint32_t W, uint32_t H, const tb_output_settings* settings, const tb_denoiser_settings* denoiser, float timeSeed)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED, "tb_render_realtime: the real-time chain runs on one device");
    return guarded(c, [&]() {
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "tb_render_realtime: no scene loaded");
        tb_output_settings s; if (settings) s = *settings; else DefaultOutputSettings(s);
        s.RenderModeRealTime = 1;
        tb_denoiser_settings dn; if (denoiser) dn = *denoiser; else tb_default_denoiser_settings(&dn);
        const int64_t savedAov = c->options.value[OPT_aov]; const bool savedSet = c->options.isSet[OPT_aov];
        c->options.value[OPT_aov] = 1; c->options.isSet[OPT_aov] = true;
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        if (c->rt.width != W || c->rt.height != H) {
            for (DevBuf* b : {&c->rt.indirect[0], &c->rt.indirect[1], &c->rt.moment[0], &c->rt.moment[1], &c->rt.finalOut[0], &c->rt.finalOut[1], &c->rt.denoise[0],
                &c->rt.denoise[1], &c->rt.composited}) {
                ensure(*b, bytes); HIP_TRY(hipMemsetAsync(b->p, 0, bytes, c->stream));
            }
            c->rt.width = W; c->rt.height = H; c->rt.active = 0; c->rt.prevCamera = c->camera;
        }
        touchAccumulation(c);
        int rc;
        { struct InChain { bool& f; explicit InChain(bool& b) : f(b) { f = true; } ~InChain() { f = false; } } inChain(c->rt.chainFrame);
            rc = renderImpl(c, W, H, 1, &s, timeSeed, false); }
        c->options.value[OPT_aov] = savedAov; c->options.isSet[OPT_aov] = savedSet;
        if (rc != TB_OK) return rc;
        const uint32_t cur = c->rt.active, prev = cur ^ 1u;
        /* AOVWorldPosition0SRV + GetPathTracerOutputIndex(), TracerBoy.cpp:3614-3622 */
        const TbFloat4* wpCur = (const TbFloat4*)c->aov[TB_AOV_WORLD_POSITION0 + cur].p;
        const TbFloat4* wpPrev = (const TbFloat4*)c->aov[TB_AOV_WORLD_POSITION0 + prev].p;
        const TbFloat4* normals = (const TbFloat4*)c->aov[TB_AOV_NORMALS].p;
        auto temporal = [&](const TbFloat4* current, DevBuf* outBuf, DevBuf* histBuf, DevBuf* momentOut, DevBuf* momentHist) {
            TbTemporalConstants k; memset(&k, 0, sizeof k); /* TemporalAccumulationPass.cpp:95-110 */
            k.ResolutionX = W; k.ResolutionY = H; k.OutputMomentInformation = momentOut ? 1u : 0u;
            /* evaluated after m_SamplesRendered++ (TracerBoy.cpp:2930,3083), i.e. never set while rendering */
            k.IgnoreHistory = c->samplesRendered == 0 ? 1u : 0u;
            k.HistoryWeight = 0.95f; k.CameraLensHeight = c->camera.LensHeight; k.CameraFocalDistance = c->camera.FocalDistance;
            memcpy(k.CameraPosition, c->camera.Position, 12); memcpy(k.CameraLookAt, c->camera.LookAt, 12); memcpy(k.CameraRight, c->camera.Right, 12);
                memcpy(k.CameraUp, c->camera.Up, 12);
            memcpy(k.PrevFrameCameraPosition, c->rt.prevCamera.Position, 12); memcpy(k.PrevFrameCameraLookAt, c->rt.prevCamera.LookAt, 12);
            memcpy(k.PrevFrameCameraRight, c->rt.prevCamera.Right, 12); memcpy(k.PrevFrameCameraUp, c->rt.prevCamera.Up, 12);
            HIP_TRY(rt_launch_temporal(c->stream, &k, (const TbFloat4*)histBuf->p, current, wpCur, wpPrev,
                momentHist ? (const TbFloat4*)momentHist->p : nullptr, normals,
                                       (TbFloat4*)outBuf->p, momentOut ? (TbFloat4*)momentOut->p : nullptr));
        };
        temporal((const TbFloat4*)c->output.p, &c->rt.indirect[cur], &c->rt.indirect[prev], &c->rt.moment[cur], &c->rt.moment[prev]);
        c->rt.last[0] = (int)cur; c->rt.last[1] = (int)cur;
        const TbFloat4* lighting = (const TbFloat4*)c->rt.indirect[cur].p;
        c->rt.last[2] = -1;
        if (dn.Enabled && s.OutputType == TB_OUTPUT_TYPE_LIT)
            c->rt.last[2] = runAtrousPasses(c->stream, W, H, dn.WaveletIterations, lighting, normals, wpCur, c->rt.denoise, dn, c->samplesRendered);
        if (c->rt.last[2] >= 0) lighting = (const TbFloat4*)c->rt.denoise[c->rt.last[2]].p;
        HIP_TRY(rt_launch_composite(c->stream, W, H, (const TbFloat4*)c->aov[TB_AOV_CUSTOM].p, lighting, (const TbFloat4*)c->aov[TB_AOV_EMISSIVE].p,
            (TbFloat4*)c->rt.composited.p));
        c->rt.last[3] = 0;
        temporal((const TbFloat4*)c->rt.composited.p, &c->rt.finalOut[cur], &c->rt.finalOut[prev], nullptr, nullptr);
        c->rt.last[4] = (int)cur;
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipEventElapsedTime(&c->lastMs, c->ev0, c->ev1); /* the path-tracing launch of this frame */
        c->rt.active = prev; c->rt.prevCamera = c->camera; c->rt.lastRender = true; /* TracerBoy.cpp:3363-3367 */
        return TB_OK;
    });
}

int tb_read_realtime(tb_context* c, int stage, float* dst)
{
    return guarded(c, [&]() {
        if (!dst || stage < 0 || stage > 4 || !c->rt.lastRender || c->rt.last[stage] < 0) return fail(c, TB_E_INVALID,
            "tb_read_realtime: stage not available (render a real-time frame first)");
        const DevBuf* b = stage == 0 ? &c->rt.indirect[c->rt.last[0]] : stage == 1 ? &c->rt.moment[c->rt.last[1]] : stage == 2 ? &c->rt.denoise[c->rt.last[2]] :
            stage == 3 ? &c->rt.composited : &c->rt.finalOut[c->rt.last[4]];
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(dst, b->p, (size_t)c->rt.width * c->rt.height * sizeof(TbFloat4), hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_run_temporal(tb_context* c, const TbTemporalConstants* k, const float* history, const float* current, const float* worldPos,
                    const float* prevWorldPos, const float* momentHistory, const float* normals, float* out, float* outMoment)
{
    return guarded(c, [&]() {
        if (!k || !history || !current || !worldPos || !prevWorldPos || !normals || !out) return fail(c, TB_E_INVALID, "tb_run_temporal: null array");
        if (const char* why = surfaceRefusal(k->ResolutionX, k->ResolutionY)) return fail(c, TB_E_INVALID, std::string("tb_run_temporal: ") + why);
        if (k->OutputMomentInformation && (!momentHistory || !outMoment)) return fail(c, TB_E_INVALID,
            "tb_run_temporal: OutputMomentInformation is set and a moment array is null");
        const size_t bytes = (size_t)k->ResolutionX * k->ResolutionY * sizeof(TbFloat4);
        const DevBuf dHist = staged(history, bytes), dCur = staged(current, bytes), dWp = staged(worldPos, bytes), dPrevWp = staged(prevWorldPos, bytes),
            dNormals = staged(normals, bytes), dOut = scratch(bytes);
        DevBuf dMomHist, dMom; /* none without moments: the kernel gets null pointers */
        if (k->OutputMomentInformation) { dMomHist = staged(momentHistory, bytes); dMom = scratch(bytes); }
        HIP_TRY(rt_launch_temporal(c->stream, k, (const TbFloat4*)dHist.p, (const TbFloat4*)dCur.p, (const TbFloat4*)dWp.p, (const TbFloat4*)dPrevWp.p,
                                   (const TbFloat4*)dMomHist.p, (const TbFloat4*)dNormals.p, (TbFloat4*)dOut.p, (TbFloat4*)dMom.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        if (dMom.p) copyBack(outMoment, dMom);
        return TB_OK;
    });
}

int tb_run_denoise_pass(tb_context* c, const TbDenoiserConstants* k, const float* input, const float* normals, const float* positions,
                        const float* undenoised, float* out)
{
    return guarded(c, [&]() {
        if (!k || !input || !normals || !positions || !undenoised || !out) return fail(c, TB_E_INVALID, "tb_run_denoise_pass: null array");
        if (const char* why = surfaceRefusal(k->ResolutionX, k->ResolutionY)) return fail(c, TB_E_INVALID, std::string("tb_run_denoise_pass: ") + why);
        if (k->OffsetMultiplier == 0) return fail(c, TB_E_INVALID, "tb_run_denoise_pass: OffsetMultiplier is 0");
        const size_t bytes = (size_t)k->ResolutionX * k->ResolutionY * sizeof(TbFloat4);
        const DevBuf dIn = staged(input, bytes), dNormals = staged(normals, bytes), dPos = staged(positions, bytes), dUnd = staged(undenoised, bytes),
            dOut = scratch(bytes);
        HIP_TRY(rt_launch_denoise(c->stream, k, (const TbFloat4*)dIn.p, (const TbFloat4*)dNormals.p, (const TbFloat4*)dPos.p, (const TbFloat4*)dUnd.p,
                                  (TbFloat4*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_run_composite(tb_context* c, uint32_t W, uint32_t H, const float* albedo, const float* lighting, const float* emissive, float* out)
{
    return guarded(c, [&]() {
        if (!albedo || !lighting || !emissive || !out) return fail(c, TB_E_INVALID, "tb_run_composite: null array");
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_composite: ") + why);
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        const DevBuf dAlbedo = staged(albedo, bytes), dLighting = staged(lighting, bytes), dEmissive = staged(emissive, bytes), dOut = scratch(bytes);
        HIP_TRY(rt_launch_composite(c->stream, W, H, (const TbFloat4*)dAlbedo.p, (const TbFloat4*)dLighting.p, (const TbFloat4*)dEmissive.p,
            (TbFloat4*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

} // extern "C"
