/* context_compare.cpp -- image-quality metrics on the device (include/tracerboy_hip.h tb_run_compare / tb_set_reference /
 * tb_compare): MSE, MAE, the largest error, relMSE and PSNR on linear values and SSIM on clamped ones, of the accumulation's mean or the denoised
 * still against a reference picture uploaded once.  No reference counterpart: the definitions are the standard ones.  Reads the context's
 * surfaces, writes buffers of its own: a render continued afterwards is the uninterrupted one.  The seam and the stage go through the same
 * launch (cmp_launch.h) with the same layout of partial records, so they agree bit for bit on the same two surfaces. */
#include "context_internal.h"
#include "../kernels/cmp_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

const uint32_t kKnownFlags = TB_COMPARE_SSIM | TB_COMPARE_SUMS;
bool positiveFinite(float v) { return v > 0.0f && v < std::numeric_limits<float>::infinity(); }

/* why a call refuses these settings or this size; empty: it does not */
std::string refusal(uint32_t w, uint32_t h, const tb_compare_settings& s)
{
    if (w == 0 || h == 0) return "a dimension is 0";
    if ((uint64_t)w * h > CMP_MAX_PIXELS) return "more than 2^26 pixels";
    if (!positiveFinite(s.peak)) return "peak is not a finite number above 0";
    if (!positiveFinite(s.rel_epsilon)) return "rel_epsilon is not a finite number above 0";
    if (s.flags & ~kKnownFlags) return "unknown flags " + std::to_string(s.flags & ~kKnownFlags);
    return "";
}

/* The kernels between two events on the context's stream, a wait, the record read back and turned into the result, the maps where asked for.
 * sums: test holds sums (rgb / w, a zero weight is unsampled).  The map buffers are sized here, only when a map is asked for. */
void compareSurfaces(tb_context* c, uint32_t w, uint32_t h, const void* test, const void* ref, bool sums, const tb_compare_settings& s, DevBuf& scratch,
    DevBuf& sqErr, DevBuf& ssim, DevEvent (&ev)[2], tb_compare_result* out, float* sqErrMap, float* ssimMap)
{
    const bool wantSsim = (s.flags & TB_COMPARE_SSIM) != 0, windows = wantSsim && cmp_ssim_groups(w, h) != 0;
    const size_t mapBytes = (size_t)w * h * 4, ssimBytes = windows ? (size_t)(w - 10u) * (h - 10u) * 4 : 0;
    ensure(scratch, cmp_scratch_bytes(w, h));
    if (sqErrMap) ensure(sqErr, mapBytes);
    if (ssimMap && ssimBytes) ensure(ssim, ssimBytes);
    HIP_TRY(hipEventRecord(ev[0].create(), c->stream));
    HIP_TRY(cmp_launch(c->stream, w, h, (const TbFloat4*)test, (const TbFloat4*)ref, (wantSsim ? CMP_FLAG_SSIM : 0u) | (sums ? CMP_FLAG_TEST_SUMS : 0u),
        s.peak, s.rel_epsilon, scratch.p, sqErrMap ? (float*)sqErr.p : nullptr, ssimMap && ssimBytes ? (float*)ssim.p : nullptr));
    HIP_TRY(hipEventRecord(ev[1].create(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    CmpRecord r[2];
    HIP_TRY(hipMemcpy(r, (const char*)scratch.p + cmp_result_offset(w, h), sizeof r, hipMemcpyDeviceToHost));
    if (sqErrMap) HIP_TRY(hipMemcpy(sqErrMap, sqErr.p, mapBytes, hipMemcpyDeviceToHost));
    if (ssimMap && ssimBytes) HIP_TRY(hipMemcpy(ssimMap, ssim.p, ssimBytes, hipMemcpyDeviceToHost));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) ms = 0.0f;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    memset(out, 0, sizeof *out);
    out->pixels = r[0].n[0]; out->excluded = r[0].n[1]; out->unsampled = r[0].n[2];
    const double terms = 3.0 * (double)out->pixels;
    out->mse = out->pixels ? r[0].d[0] / terms : nan;
    out->mae = out->pixels ? r[0].d[1] / terms : nan;
    out->rel_mse = out->pixels ? r[0].d[2] / terms : nan;
    out->max_abs = out->pixels ? r[0].d[3] : nan;
    out->psnr = !out->pixels ? nan : out->mse == 0.0 ? std::numeric_limits<double>::infinity() : 10.0 * std::log10(((double)s.peak * (double)s.peak) / out->mse);
    out->ssim_windows = windows ? r[1].n[0] : 0; out->ssim_windows_skipped = windows ? r[1].n[1] : 0;
    out->ssim = out->ssim_windows ? r[1].d[0] / (double)out->ssim_windows : nan;
    out->gpu_us = ms * 1000.0f;
}

} // namespace

extern "C" {

void tb_default_compare_settings(tb_compare_settings* o)
{
    if (!o) return;
    o->peak = 1.0f; o->rel_epsilon = 0.01f; o->flags = TB_COMPARE_SSIM;
}

int tb_run_compare(tb_context* c, uint32_t w, uint32_t h, const float* testRgba, const float* refRgba, const tb_compare_settings* settings,
    tb_compare_result* out, float* sqErrMap, float* ssimMap)
{
    return guarded(c, [&]() {
        if (!testRgba || !refRgba || !out) return fail(c, TB_E_INVALID, "tb_run_compare: null pointer");
        tb_compare_settings s; if (settings) s = *settings; else tb_default_compare_settings(&s);
        const std::string why = refusal(w, h, s);
        if (!why.empty()) return fail(c, TB_E_INVALID, "tb_run_compare: " + why);
        const size_t bytes = (size_t)w * h * sizeof(TbFloat4);
        const DevBuf dTest = staged(testRgba, bytes), dRef = staged(refRgba, bytes);
        DevBuf scratch, sqErr, ssim; DevEvent ev[2];
        compareSurfaces(c, w, h, dTest.p, dRef.p, (s.flags & TB_COMPARE_SUMS) != 0, s, scratch, sqErr, ssim, ev, out, sqErrMap, ssimMap);
        return TB_OK;
    });
}

int tb_set_reference(tb_context* c, uint32_t w, uint32_t h, const float* rgba)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_set_reference: not supported for a multi-device group: the comparison runs on one device");
    return guarded(c, [&]() {
        if (!rgba) { /* the reference goes, and with it what was sized for it */
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->cmp.reference.release(); c->cmp.scratch.release(); c->cmp.sqErr.release(); c->cmp.ssim.release(); c->cmp.refW = 0; c->cmp.refH = 0;
            return TB_OK;
        }
        if (w == 0 || h == 0) return fail(c, TB_E_INVALID, "tb_set_reference: a dimension is 0");
        if ((uint64_t)w * h > CMP_MAX_PIXELS) return fail(c, TB_E_INVALID, "tb_set_reference: more than 2^26 pixels");
        HIP_TRY(hipStreamSynchronize(c->stream)); /* no comparison still reads the old one */
        c->cmp.refW = 0; c->cmp.refH = 0;
        ensure(c->cmp.reference, (size_t)w * h * sizeof(TbFloat4));
        HIP_TRY(hipMemcpy(c->cmp.reference.p, rgba, c->cmp.reference.bytes, hipMemcpyHostToDevice));
        c->cmp.refW = w; c->cmp.refH = h;
        return TB_OK;
    });
}

int tb_compare(tb_context* c, uint32_t surface, const tb_compare_settings* settings, tb_compare_result* out, float* sqErrMap, float* ssimMap)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_compare: not supported for a multi-device group: the comparison runs on one device");
    return guarded(c, [&]() {
        if (!out) return fail(c, TB_E_INVALID, "tb_compare: the result pointer is null");
        if (surface != TB_COMPARE_MEAN && surface != TB_COMPARE_DENOISED) return fail(c, TB_E_INVALID, "tb_compare: unknown surface " + std::to_string(surface));
        tb_compare_settings s; if (settings) s = *settings; else tb_default_compare_settings(&s);
        if (s.flags & TB_COMPARE_SUMS) return fail(c, TB_E_INVALID, "tb_compare: TB_COMPARE_SUMS belongs to tb_run_compare: here the surface decides");
        if (!c->output.p || !c->width || c->samplesRendered == c->firstFrame) return fail(c, TB_E_INVALID, "tb_compare: nothing rendered: the context holds no frames");
        const std::string why = refusal(c->width, c->height, s);
        if (!why.empty()) return fail(c, TB_E_INVALID, "tb_compare: " + why);
        if (!c->cmp.refW) return fail(c, TB_E_INVALID, "tb_compare: no reference: call tb_set_reference");
        if (c->cmp.refW != c->width || c->cmp.refH != c->height) return fail(c, TB_E_INVALID, "tb_compare: the reference is " + std::to_string(c->cmp.refW) +
            " x " + std::to_string(c->cmp.refH) + ", the rendered surface " + std::to_string(c->width) + " x " + std::to_string(c->height));
        if (surface == TB_COMPARE_MEAN && c->rt.lastRender) return fail(c, TB_E_INVALID,
            "tb_compare: the last render was tb_render_realtime: its surface holds one frame, not an accumulation");
        if (surface == TB_COMPARE_DENOISED && !c->dn.valid) return fail(c, TB_E_INVALID,
            "tb_compare: no valid denoised surface: call tb_denoise after the last change of the accumulation");
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        const bool mean = surface == TB_COMPARE_MEAN;
        compareSurfaces(c, c->width, c->height, mean ? c->output.p : c->dn.finalOut.p, c->cmp.reference.p, mean, s, c->cmp.scratch, c->cmp.sqErr, c->cmp.ssim,
            c->cmp.ev, out, sqErrMap, ssimMap);
        return TB_OK;
    });
}

} // extern "C"
