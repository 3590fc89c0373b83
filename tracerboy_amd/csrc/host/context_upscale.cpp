/* context_upscale.cpp -- FSR 1 upscaling of the post-processed picture (include/tracerboy_hip.h tb_fsr_constants /
 * tb_run_fsr_easu / tb_run_fsr_rcas / tb_upscale): the reference's FidelityFXSuperResolutionPass::Run (FidelityFXSuperResolution.cpp:53-111) behind
 * tb_post_process -- EASU to the display size, then RCAS.  Reads what the output stage wrote (postOut / postRgba8), writes surfaces of its own:
 * accumulation, AOVs, frame counter, history and denoised surfaces stay as they are. */
#include "context_internal.h"
#include "../kernels/fsr_launch.h"
#include "tb_math.h"

using namespace tbhost;
using namespace tbctx;

namespace {

const float kReferenceSharpness = 0.2f; /* FsrRcasCon(constants.const0, 0.2f), FidelityFXSuperResolution.cpp:102 */

/* AU1_AH1_AF1 (ffx_a.h:482-551): binary32 -> binary16 with the mantissa cut off, too small = signed zero, too large = the largest finite */
uint32_t halfTruncated(float f)
{
    const uint32_t u = tb_f2u(f), sign = (u >> 16) & 0x8000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    if (e < 103u) return sign;
    if (e < 113u) return sign | ((0x800000u | m) >> (126u - e));
    if (e > 142u) return sign | 0x7bffu;
    return sign | ((e - 112u) << 10) | (m >> 13);
}

/* bytes per texel of a surface type; 0 = no such type */
size_t texelBytes(uint32_t surface) { return surface == TB_FSR_SURFACE_UNORM8 ? 4u : surface == TB_FSR_SURFACE_F32 ? 16u : 0u; }

} // namespace

extern "C" {

int tb_fsr_constants(uint32_t inW, uint32_t inH, uint32_t outW, uint32_t outH, float sharpnessStops, TbFsrConstants* out)
{
    if (!out || !inW || !inH || !outW || !outH || !(tb_abs(sharpnessStops) < tb_u2f(0x7f800000u))) return TB_E_INVALID;
    memset(out, 0, sizeof *out);
    /* FsrEasuCon(con0..con3, viewport = in, size = in, out), ffx_fsr1.h:156-202 */
    const float vx = (float)inW, vy = (float)inH, rox = 1.0f / (float)outW, roy = 1.0f / (float)outH, rix = 1.0f / vx, riy = 1.0f / vy;
    uint32_t* k = out->easu;
    k[0] = tb_f2u(vx * rox); k[1] = tb_f2u(vy * roy);
    k[2] = tb_f2u((0.5f * vx) * rox - 0.5f); k[3] = tb_f2u((0.5f * vy) * roy - 0.5f);
    k[4] = tb_f2u(rix); k[5] = tb_f2u(riy); k[6] = tb_f2u(1.0f * rix); k[7] = tb_f2u(-1.0f * riy);
    k[8] = tb_f2u(-1.0f * rix); k[9] = tb_f2u(2.0f * riy); k[10] = tb_f2u(1.0f * rix); k[11] = tb_f2u(2.0f * riy);
    k[12] = tb_f2u(0.0f * rix); k[13] = tb_f2u(4.0f * riy); k[14] = 0; k[15] = 0;
    /* FsrRcasCon, :662-672 */
    const float sharp = tb_exp2(-sharpnessStops);
    const uint32_t h = halfTruncated(sharp);
    out->rcas[0] = tb_f2u(sharp); out->rcas[1] = h | (h << 16); out->rcas[2] = 0; out->rcas[3] = 0;
    return TB_OK;
}

int tb_run_fsr_easu(tb_context* c, const TbFsrConstants* k, uint32_t surface, uint32_t inW, uint32_t inH, uint32_t outW, uint32_t outH, const void* in,
    void* out)
{
    return guarded(c, [&]() {
        if (!k || !in || !out) return fail(c, TB_E_INVALID, "tb_run_fsr_easu: null pointer");
        const size_t texel = texelBytes(surface);
        if (!texel) return fail(c, TB_E_INVALID, "tb_run_fsr_easu: unknown surface type " + std::to_string(surface));
        if (const char* why = surfaceRefusal(inW, inH)) return fail(c, TB_E_INVALID, std::string("tb_run_fsr_easu: input: ") + why);
        if (const char* why = surfaceRefusal(outW, outH)) return fail(c, TB_E_INVALID, std::string("tb_run_fsr_easu: output: ") + why);
        if (outW < inW || outH < inH) return fail(c, TB_E_INVALID, "tb_run_fsr_easu: the output is smaller than the input: FSR 1 only upscales");
        const DevBuf dIn = staged(in, (size_t)inW * inH * texel), dOut = scratch((size_t)outW * outH * texel);
        HIP_TRY(fsr_launch_easu(c->stream, surface, k->easu, inW, inH, outW, outH, dIn.p, dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_run_fsr_rcas(tb_context* c, const TbFsrConstants* k, uint32_t surface, uint32_t W, uint32_t H, const void* in, void* out)
{
    return guarded(c, [&]() {
        if (!k || !in || !out) return fail(c, TB_E_INVALID, "tb_run_fsr_rcas: null pointer");
        const size_t texel = texelBytes(surface);
        if (!texel) return fail(c, TB_E_INVALID, "tb_run_fsr_rcas: unknown surface type " + std::to_string(surface));
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_fsr_rcas: ") + why);
        const DevBuf dIn = staged(in, (size_t)W * H * texel), dOut = scratch(dIn.bytes);
        HIP_TRY(fsr_launch_rcas(c->stream, surface, k->rcas[0], W, H, dIn.p, dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_upscale(tb_context* c, const tb_post_settings* post, uint32_t outputType, uint32_t outW, uint32_t outH, float sharpnessStops, float* rgbaF32,
    uint8_t* rgba8)
{
    return guarded(c, [&]() {
        if (!rgbaF32 && !rgba8) return fail(c, TB_E_INVALID, "tb_upscale: both output pointers are null");
        if (const char* why = surfaceRefusal(outW, outH)) return fail(c, TB_E_INVALID, std::string("tb_upscale: output: ") + why);
        if (!(tb_abs(sharpnessStops) < tb_u2f(0x7f800000u))) return fail(c, TB_E_INVALID, "tb_upscale: sharpness_stops is not finite");
        if (c->width && (outW < c->width || outH < c->height)) return fail(c, TB_E_INVALID, "tb_upscale: " + std::to_string(outW) + " x " +
            std::to_string(outH) + " is smaller than the rendered " + std::to_string(c->width) + " x " + std::to_string(c->height) + ": FSR 1 only upscales");
        if (int rc = launchPostProcess(c, post, outputType)) return rc; /* refuses what tb_post_process refuses, with its message */
        const uint32_t inW = c->width, inH = c->height;
        TbFsrConstants k;
        if (tb_fsr_constants(inW, inH, outW, outH, sharpnessStops < 0.0f ? kReferenceSharpness : sharpnessStops, &k) != TB_OK)
            return fail(c, TB_E_INVALID, "tb_upscale: no constants for these sizes");
        const size_t outPx = (size_t)outW * outH;
        const bool run[2] = {rgba8 != nullptr, rgbaF32 != nullptr}; /* by surface type: TB_FSR_SURFACE_UNORM8, TB_FSR_SURFACE_F32 */
        const void* const src[2] = {c->postRgba8.p, c->postOut.p};
        for (uint32_t t = 0; t < 2u; t++) if (run[t]) { ensure(c->fsr.mid[t], outPx * texelBytes(t)); ensure(c->fsr.out[t], outPx * texelBytes(t)); }
        for (uint32_t t = 0; t < 2u; t++) {
            if (!run[t]) continue;
            HIP_TRY(hipEventRecord(c->fsr.ev[2 * t].create(), c->stream));
            HIP_TRY(fsr_launch_easu(c->stream, t, k.easu, inW, inH, outW, outH, src[t], c->fsr.mid[t].p));
            HIP_TRY(hipEventRecord(c->fsr.ev[2 * t + 1].create(), c->stream));
            HIP_TRY(fsr_launch_rcas(c->stream, t, k.rcas[0], outW, outH, c->fsr.mid[t].p, c->fsr.out[t].p));
            HIP_TRY(hipEventRecord(c->fsr.ev[4 + t].create(), c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->fsr.lastEasuMs = 0.0f; c->fsr.lastRcasMs = 0.0f;
        for (uint32_t t = 0; t < 2u; t++) {
            if (!run[t]) continue;
            float easu = 0.0f, rcas = 0.0f;
            if (hipEventElapsedTime(&easu, c->fsr.ev[2 * t], c->fsr.ev[2 * t + 1]) != hipSuccess) easu = 0.0f;
            if (hipEventElapsedTime(&rcas, c->fsr.ev[2 * t + 1], c->fsr.ev[4 + t]) != hipSuccess) rcas = 0.0f;
            c->fsr.lastEasuMs += easu; c->fsr.lastRcasMs += rcas;
        }
        c->fsr.lastUpscaleMs = c->fsr.lastEasuMs + c->fsr.lastRcasMs;
        if (rgba8) HIP_TRY(hipMemcpy(rgba8, c->fsr.out[0].p, outPx * 4, hipMemcpyDeviceToHost));
        if (rgbaF32) HIP_TRY(hipMemcpy(rgbaF32, c->fsr.out[1].p, outPx * 16, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
