/* context_denoise.cpp -- the denoise of a progressive render (include/tracerboy_hip.h tb_denoise / tb_read_denoise_stage):
 * prepare (mean + dual-buffer variance of its luminance), prefilter (3x3 Gaussian over the variance), WaveletIterations passes of the real-time
 * chain's a-trous filter guided by the first-hit normals and world positions of the last rendered frame, finish ((rgb, 1) for the output stage).
 * The reference denoises stills with OIDN on DirectML (context_neural.cpp builds that); what is kept from it is DenoiserCS itself, run
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
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_denoise: not supported for a multi-device group: AOV targets are not gathered across its devices");
    return guarded(c, [&]() {
        if (c->rt.lastRender) return fail(c, TB_E_INVALID,
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
        const DevBuf& normals = mode ? c->dn.normals : c->aov[TB_AOV_NORMALS];
        const DevBuf& positions = mode ? c->dn.positions : c->aov[TB_AOV_WORLD_POSITION0 + (last % 2u)];
        if (iterations > 0 && mode == 0) {
            if (c->callCount < c->dn.aovStaleUntilCall) return fail(c, TB_E_INVALID,
                "tb_denoise: the filter passes need the normals and world positions of the last frame, and nothing was rendered since tb_state_load / "
                "tb_state_begin (AOVs are not part of a state): render at least one more frame with option \"aov\"");
            if (!opt<OPT_aov>(c) || normals.bytes != bytes || positions.bytes != bytes) return fail(c, TB_E_INVALID,
                "tb_denoise: the filter passes need the normals and world positions of the last frame: set option \"aov\" before tb_render");
        }
        c->dn.valid = false; c->dn.lastPass = -1;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        ensure(c->dn.prepared, bytes); ensure(c->dn.filtered, bytes); ensure(c->dn.finalOut, bytes);
        if (iterations > 0) ensure(c->dn.pass[0], bytes);
        if (iterations > 1) ensure(c->dn.pass[1], bytes);
        if (mode != 0 && iterations > 0) { ensure(c->dn.normals, bytes); ensure(c->dn.positions, bytes); }
        const TbFloat4* const albedo = (const TbFloat4*)c->guides.sum[0].p; /* mode 2: (sum of the effective albedo, frames) */
        HIP_TRY(hipEventRecord(c->dn.ev[0].create(), c->stream));
        if (mode != 0 && iterations > 0) HIP_TRY(dn_launch_resolve_guides(c->stream, (const TbFloat4*)c->guides.sum[1].p, (const TbFloat4*)c->guides.sum[2].p,
            (TbFloat4*)c->dn.normals.p, (TbFloat4*)c->dn.positions.p, W, H));
        if (mode == 2) HIP_TRY(dn_launch_prepare_demod(c->stream, (const TbFloat4*)c->output.p, (const TbFloat4*)c->jittered.p, albedo, (TbFloat4*)c->dn.prepared.p, W, H));
        else
        HIP_TRY(dn_launch_prepare(c->stream, (const TbFloat4*)c->output.p, (const TbFloat4*)c->jittered.p, (TbFloat4*)c->dn.prepared.p, W, H));
        HIP_TRY(dn_launch_prefilter(c->stream, (const TbFloat4*)c->dn.prepared.p, (TbFloat4*)c->dn.filtered.p, W, H));
        const int lastPass = runAtrousPasses(c->stream, W, H, iterations, (const TbFloat4*)c->dn.filtered.p, (const TbFloat4*)normals.p,
            (const TbFloat4*)positions.p, c->dn.pass, dn, c->samplesRendered); /* as tb_render_realtime runs them */
        const TbFloat4* in = (const TbFloat4*)(lastPass < 0 ? c->dn.filtered.p : c->dn.pass[lastPass].p);
        if (mode == 2) HIP_TRY(dn_launch_finish_remod(c->stream, in, albedo, (TbFloat4*)c->dn.finalOut.p, W, H));
        else HIP_TRY(dn_launch_finish(c->stream, in, (TbFloat4*)c->dn.finalOut.p, W, H));
        HIP_TRY(hipEventRecord(c->dn.ev[1].create(), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (hipEventElapsedTime(&c->dn.lastMs, c->dn.ev[0], c->dn.ev[1]) != hipSuccess) c->dn.lastMs = 0.0f;
        c->dn.lastPass = lastPass; c->dn.valid = true; c->dn.mode = mode;
        if (rgba) HIP_TRY(hipMemcpy(rgba, c->dn.finalOut.p, bytes, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_read_denoise_stage(tb_context* c, int stage, float* rgba)
{
    return guarded(c, [&]() {
        if (!rgba || stage < 0 || stage > 3) return fail(c, TB_E_INVALID, "tb_read_denoise_stage: stage is 0 (prepared), 1 (filtered), 2 (last filter pass) or 3 (final)");
        if (!c->dn.valid) return fail(c, TB_E_INVALID,
            "tb_read_denoise_stage: no valid denoised surface: call tb_denoise after the last change of the accumulation");
        if (stage == 2 && c->dn.lastPass < 0) return fail(c, TB_E_INVALID, "tb_read_denoise_stage: stage 2: the last tb_denoise ran no filter pass");
        const DevBuf& b = stage == 0 ? c->dn.prepared : stage == 1 ? c->dn.filtered : stage == 2 ? c->dn.pass[c->dn.lastPass] : c->dn.finalOut;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(rgba, b.p, (size_t)c->width * c->height * sizeof(TbFloat4), hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
