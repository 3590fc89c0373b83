/* context_denoise.cpp -- the denoise of a progressive render (include/tracerboy_hip.h tb_denoise / tb_read_denoise_stage):
 * prepare (mean + dual-buffer variance of its luminance), prefilter (3x3 Gaussian over the variance), WaveletIterations passes of the real-time
 * chain's a-trous filter guided by the first-hit normals and world positions of the last rendered frame, finish ((rgb, 1) for the output stage).
 * The reference denoises stills with OIDN on DirectML (out of scope); what is kept from it is DenoiserCS itself, run
 * unchanged.  Reads the accumulation surfaces and the AOVs, writes surfaces of its own: a render continued afterwards is the uninterrupted one.
 * Option "denoise_guides" (DESIGN.md section 13): the guides come from the guide pass (context_guides.cpp) instead of the last frame's AOVs, and with
 * 2 the chain runs on colour divided by the mean effective albedo and multiplies it back at the end. */
#include "context_internal.h"
#include "../kernels/dn_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {
const uint32_t kMaxIterations = 10; /* OffsetMultiplier = 1 << i: 2 x 512 pixels at the tenth pass, past that every tap of a 1024-pixel frame is outside */
}

extern "C" {

int tb_denoise(tb_context* c, const tb_denoiser_settings* denoiser, float* rgba)
{
    if (c && (!c->peers.empty() || c->groupOwner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_denoise: not supported for a multi-device group: AOV targets are not gathered across its devices");
    return guarded(c, [&]() {
        if (c->lastRenderRealtime) return fail(c, TB_E_INVALID,
            "tb_denoise: the last render was tb_render_realtime: its surface holds one frame, not an accumulation (the real-time chain denoises itself)");
        if (!c->output.p || !c->jittered.p || !c->width || c->samplesRendered == c->firstFrame) return fail(c, TB_E_INVALID,
            "tb_denoise: nothing rendered: the context holds no frames");
        tb_denoiser_settings dn; if (denoiser) dn = *denoiser; else tb_default_denoiser_settings(&dn);
        if (dn.WaveletIterations > kMaxIterations) return fail(c, TB_E_INVALID, "tb_denoise: WaveletIterations is at most " + std::to_string(kMaxIterations));
        const uint32_t iterations = dn.Enabled ? dn.WaveletIterations : 0u;
        const uint32_t W = c->width, H = c->height;
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        const uint32_t last = c->samplesRendered - 1u; /* the frame whose first hits the AOVs hold */
        /* option denoise_guides: 1 = the filter's normals and positions are the guide pass's (tb_render_guides), resolved
         * below -- no AOV is needed, so neither option "aov" nor a frame rendered since a state was loaded; 2 = 1 + albedo demodulation */
        const int mode = (int)opt<OPT_denoise_guides>(c);
        if (mode != 0 && !guidesCurrent(c)) return fail(c, TB_E_INVALID,
            "tb_denoise: option denoise_guides is set and the context holds no valid guide surfaces: call tb_render_guides (a history reset, a resize, "
            "a scene load or a change of camera, settings or time seed invalidates them)");
        const DevBuf& normals = mode ? c->dnNormals : c->aov[TB_AOV_NORMALS];
        const DevBuf& positions = mode ? c->dnPositions : c->aov[TB_AOV_WORLD_POSITION0 + (last % 2u)];
        if (iterations > 0 && mode == 0) {
            if (c->callCount < c->aovStaleUntilCall) return fail(c, TB_E_INVALID,
                "tb_denoise: the filter passes need the normals and world positions of the last frame, and nothing was rendered since tb_state_load / "
                "tb_state_begin (AOVs are not part of a state): render at least one more frame with option \"aov\"");
            if (!opt<OPT_aov>(c) || normals.bytes != bytes || positions.bytes != bytes) return fail(c, TB_E_INVALID,
                "tb_denoise: the filter passes need the normals and world positions of the last frame: set option \"aov\" before tb_render");
        }
        c->dnValid = false; c->dnLastPass = -1;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        ensure(c->dnPrepared, bytes); ensure(c->dnFiltered, bytes); ensure(c->dnFinal, bytes);
        if (iterations > 0) ensure(c->dnPass[0], bytes);
        if (iterations > 1) ensure(c->dnPass[1], bytes);
        if (mode != 0 && iterations > 0) { ensure(c->dnNormals, bytes); ensure(c->dnPositions, bytes); }
        const TbFloat4* const albedo = (const TbFloat4*)c->guide[0].p; /* mode 2: (sum of the effective albedo, frames) */
        HIP_TRY(hipEventRecord(c->evDn[0].create(), c->stream));
        if (mode != 0 && iterations > 0) HIP_TRY(dn_launch_resolve_guides(c->stream, (const TbFloat4*)c->guide[1].p, (const TbFloat4*)c->guide[2].p,
            (TbFloat4*)c->dnNormals.p, (TbFloat4*)c->dnPositions.p, W, H));
        if (mode == 2) HIP_TRY(dn_launch_prepare_demod(c->stream, (const TbFloat4*)c->output.p, (const TbFloat4*)c->jittered.p, albedo, (TbFloat4*)c->dnPrepared.p, W, H));
        else
        HIP_TRY(dn_launch_prepare(c->stream, (const TbFloat4*)c->output.p, (const TbFloat4*)c->jittered.p, (TbFloat4*)c->dnPrepared.p, W, H));
        HIP_TRY(dn_launch_prefilter(c->stream, (const TbFloat4*)c->dnPrepared.p, (TbFloat4*)c->dnFiltered.p, W, H));
        const TbFloat4* filtered = (const TbFloat4*)c->dnFiltered.p; const TbFloat4* in = filtered;
        for (uint32_t i = 0; i < iterations; i++) { /* DenoiserPass.cpp:61-93, as tb_render_realtime runs it */
            TbDenoiserConstants k; memset(&k, 0, sizeof k);
            k.ResolutionX = W; k.ResolutionY = H; k.OffsetMultiplier = 1u << i; k.GlobalFrameCount = c->samplesRendered;
            k.NormalWeightingExponential = dn.NormalWeightingExponential; k.IntersectionPositionWeightingMultiplier = dn.IntersectPositionWeightingMultiplier;
            k.LumaWeightingMultiplier = dn.LuminanceWeightingMultiplier;
            TbFloat4* out = (TbFloat4*)c->dnPass[i & 1u].p;
            HIP_TRY(rt_launch_denoise(c->stream, &k, in, (const TbFloat4*)normals.p, (const TbFloat4*)positions.p, filtered, out));
            in = out;
        }
        if (mode == 2) HIP_TRY(dn_launch_finish_remod(c->stream, in, albedo, (TbFloat4*)c->dnFinal.p, W, H));
        else HIP_TRY(dn_launch_finish(c->stream, in, (TbFloat4*)c->dnFinal.p, W, H));
        HIP_TRY(hipEventRecord(c->evDn[1].create(), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (hipEventElapsedTime(&c->lastDenoiseMs, c->evDn[0], c->evDn[1]) != hipSuccess) c->lastDenoiseMs = 0.0f;
        c->dnLastPass = iterations ? (int)((iterations - 1u) & 1u) : -1; c->dnValid = true; c->dnMode = mode;
        if (rgba) HIP_TRY(hipMemcpy(rgba, c->dnFinal.p, bytes, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_read_denoise_stage(tb_context* c, int stage, float* rgba)
{
    return guarded(c, [&]() {
        if (!rgba || stage < 0 || stage > 3) return fail(c, TB_E_INVALID, "tb_read_denoise_stage: stage is 0 (prepared), 1 (filtered), 2 (last filter pass) or 3 (final)");
        if (!c->dnValid) return fail(c, TB_E_INVALID,
            "tb_read_denoise_stage: no valid denoised surface: call tb_denoise after the last change of the accumulation");
        if (stage == 2 && c->dnLastPass < 0) return fail(c, TB_E_INVALID, "tb_read_denoise_stage: stage 2: the last tb_denoise ran no filter pass");
        const DevBuf& b = stage == 0 ? c->dnPrepared : stage == 1 ? c->dnFiltered : stage == 2 ? c->dnPass[c->dnLastPass] : c->dnFinal;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(rgba, b.p, (size_t)c->width * c->height * sizeof(TbFloat4), hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
