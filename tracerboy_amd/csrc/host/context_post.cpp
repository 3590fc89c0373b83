/* context_post.cpp -- the output stage (include/tracerboy_hip.h tb_post_process; post_kernels.hip): optional auto exposure, then the reference's
 * PostProcessCS on the surface that OutputType selects, into postOut (float) and postRgba8. */
#include "context_internal.h"

using namespace tbhost;
using namespace tbctx;

/* tb_post_process and tb_upscale (context_upscale.cpp) run it */
int tbctx::launchPostProcess(tb_context* c, const tb_post_settings* post, uint32_t outputType)
{
    if (!c->output.p || c->width == 0) return fail(c, TB_E_INVALID, "tb_post_process: nothing rendered yet");
    tb_post_settings ps; if (post) ps = *post; else tb_default_post_settings(&ps);
    const TbFloat4* in = nullptr; const float* inR32 = nullptr;
    switch (outputType) { /* GetOutputSRV, TracerBoy.cpp:2354-2383 */
    /* PostProcessInput after the real-time chain, TracerBoy.cpp:3144-3160 */
    case TB_OUTPUT_TYPE_LIT:
        if (opt<OPT_post_denoised>(c)) { /* the denoised still (tb_denoise): (rgb, 1), so that ProcessLit's division by .w is the identity */
            if (!c->dn.valid) return fail(c, TB_E_INVALID,
                "tb_post_process: option \"post_denoised\" is set and there is no valid denoised surface: call tb_denoise after the last change of the accumulation");
            in = (const TbFloat4*)c->dn.finalOut.p; break;
        }
        in = (const TbFloat4*)(c->rt.lastRender ? c->rt.finalOut[c->rt.last[4]].p : c->output.p); break;
    case TB_OUTPUT_TYPE_LUMINANCE: in = (const TbFloat4*)c->output.p; break;
    case TB_OUTPUT_TYPE_ALBEDO: case TB_OUTPUT_TYPE_LIVE_PIXELS: case TB_OUTPUT_TYPE_HEATMAP: in = (const TbFloat4*)c->aov[TB_AOV_CUSTOM].p; break;
    case TB_OUTPUT_TYPE_NORMAL: in = (const TbFloat4*)c->aov[TB_AOV_NORMALS].p; break;
    case TB_OUTPUT_TYPE_DEPTH: inR32 = (const float*)c->aov[TB_AOV_DEPTH].p; break;
    default: return fail(c, TB_E_UNSUPPORTED, "tb_post_process: this output type needs surfaces of the real-time chain (not built)");
    }
    if (!in && !inR32) return fail(c, TB_E_INVALID, "tb_post_process: the AOV for this output type was not rendered (set option \"aov\" before tb_render)");
    const size_t px = (size_t)c->width * c->height;
    ensure(c->postOut, px * 16); ensure(c->postRgba8, px * 4); ensure(c->postHistogram, 256 * 4); ensure(c->postAverage, 4);
    TbPostConstants pc; memset(&pc, 0, sizeof pc);
    pc.W = c->width; pc.H = c->height; pc.FramesRendered = c->samplesRendered; pc.ExposureMultiplier = ps.ExposureMultiplier;
    pc.TonemapType = ps.TonemapType; pc.UseGammaCorrection = ps.EnableGammaCorrection; pc.UseAutoExposure = ps.EnableAutoExposure;
    pc.OutputType = outputType; pc.VarianceMultiplier = ps.VarianceMultiplier;
    HIP_TRY(post_launch(c->stream, &pc, in, inR32, (const TbFloat4*)c->aov[TB_AOV_CUSTOM].p, (uint32_t*)c->postHistogram.p, (float*)c->postAverage.p,
                        (TbFloat4*)c->postOut.p, (uint32_t*)c->postRgba8.p));
    return TB_OK;
}

extern "C" {

void tb_default_post_settings(tb_post_settings* o) /* TracerBoy.h:298,309-313 */
{
    if (!o) return;
    o->ExposureMultiplier = 1.0f; o->EnableGammaCorrection = 1; o->EnableAutoExposure = 1; o->TonemapType = TB_TONEMAP_AGX_PUNCHY; o->VarianceMultiplier = 1.0f;
}

int tb_post_process(tb_context* c, const tb_post_settings* post, uint32_t outputType, float* rgbaF32, uint8_t* rgba8)
{
    return guarded(c, [&]() {
        if (int rc = launchPostProcess(c, post, outputType)) return rc;
        const size_t px = (size_t)c->width * c->height;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (rgbaF32) HIP_TRY(hipMemcpy(rgbaF32, c->postOut.p, px * 16, hipMemcpyDeviceToHost));
        if (rgba8) HIP_TRY(hipMemcpy(rgba8, c->postRgba8.p, px * 4, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_read_averaged_luminance(tb_context* c, float* out)
{
    return guarded(c, [&]() {
        if (!out || !c->postAverage.p) return fail(c, TB_E_INVALID, "tb_read_averaged_luminance: run tb_post_process with auto exposure first");
        HIP_TRY(hipMemcpy(out, c->postAverage.p, 4, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
