/* context_budget.cpp -- sample budgets (include/tracerboy_hip.h tb_set_sample_budget): per pixel the global frame index at
 * which it stops receiving samples.  The budget is the second source of the adaptive launch's live list (context_render.cpp decideAdaptive,
 * pt_kernels.hip live_list_count_budget); this file holds what sets and reads it, the noise target that lowers it where a pixel's estimated error
 * is small enough (section 12's prepare and prefilter, then dn_kernels.hip budget_stop_kernel) and that kernel's seam.  None of it writes the
 * accumulation surfaces, the frame counter, the history, the guides or the denoised surfaces. */
#include "context_internal.h"
#include "../kernels/dn_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

/* prepare + prefilter of the two sums into `prepared` / `filtered`, the stop kernel on `budget`, the two counts back; waits for the stream */
void runStop(hipStream_t stream, const TbFloat4* output, const TbFloat4* jittered, TbFloat4* prepared, TbFloat4* filtered, uint32_t* budget,
    unsigned long long* counts, uint32_t W, uint32_t H, uint32_t frame, uint32_t minFrames, float relError, uint64_t* stopped, uint64_t* live,
    hipEvent_t before = nullptr, hipEvent_t after = nullptr)
{
    HIP_TRY(hipMemsetAsync(counts, 0, 16, stream));
    if (before) HIP_TRY(hipEventRecord(before, stream));
    HIP_TRY(dn_launch_prepare(stream, output, jittered, prepared, W, H));
    HIP_TRY(dn_launch_prefilter(stream, prepared, filtered, W, H));
    HIP_TRY(dn_launch_budget_stop(stream, output, jittered, filtered, budget, W, H, frame, minFrames, relError, counts));
    if (after) HIP_TRY(hipEventRecord(after, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    unsigned long long host[2] = {0, 0};
    HIP_TRY(hipMemcpy(host, counts, 16, hipMemcpyDeviceToHost));
    if (stopped) *stopped = host[0];
    if (live) *live = host[1];
}

const char* relErrorRefusal(float relError) { return std::isfinite(relError) && relError >= 0.0f ? nullptr : "rel_error must be finite and not negative"; }

} // namespace

extern "C" {

int tb_set_sample_budget(tb_context* c, uint32_t width, uint32_t height, const uint32_t* budget)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_set_sample_budget: not supported for a multi-device group: a budget belongs to one context (give each rank of a tile assignment its own)");
    return guarded(c, [&]() {
        if (!budget) { /* clear: the next call is planned and launched as if there had never been one */
            HIP_TRY(hipStreamSynchronize(c->stream)); /* (a call in flight reads it) */
            c->budget.values.release(); c->budget.set = false; c->budget.width = c->budget.height = 0;
            return TB_OK;
        }
        if (const char* why = surfaceRefusal(width, height)) return fail(c, TB_E_INVALID, std::string("tb_set_sample_budget: ") + why);
        if (opt<OPT_count_rays>(c)) return fail(c, TB_E_INVALID,
            "tb_set_sample_budget: a sample budget and option \"count_rays\" exclude each other (the counting kernels have no list-driven copy)");
        const size_t bytes = (size_t)width * height * 4u;
        HIP_TRY(hipStreamSynchronize(c->stream)); /* before the buffer a call in flight reads is replaced */
        ensure(c->budget.values, bytes);
        HIP_TRY(hipMemcpy(c->budget.values.p, budget, bytes, hipMemcpyHostToDevice));
        c->budget.set = true; c->budget.width = width; c->budget.height = height;
        return TB_OK;
    });
}

int tb_read_sample_budget(tb_context* c, uint32_t* out)
{
    return guarded(c, [&]() {
        if (!c->budget.set) return fail(c, TB_E_INVALID, "tb_read_sample_budget: no sample budget is set");
        if (!out) return fail(c, TB_E_INVALID, "tb_read_sample_budget: null array");
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out, c->budget.values.p, c->budget.values.bytes, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_budget_stop_converged(tb_context* c, float relError, uint32_t minFrames, uint64_t* stopped, uint64_t* live)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_budget_stop_converged: not supported for a multi-device group: a budget belongs to one context");
    return guarded(c, [&]() {
        if (const char* why = relErrorRefusal(relError)) return fail(c, TB_E_INVALID, std::string("tb_budget_stop_converged: ") + why);
        if (c->rt.lastRender) return fail(c, TB_E_INVALID,
            "tb_budget_stop_converged: the last render was tb_render_realtime: its surface holds one frame, not an accumulation");
        if (!c->output.p || !c->jittered.p || !c->width || c->samplesRendered == c->firstFrame) return fail(c, TB_E_INVALID,
            "tb_budget_stop_converged: nothing rendered: the context holds no frames");
        const uint32_t W = c->width, H = c->height;
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_budget_stop_converged: ") + why);
        if (c->budget.set && (c->budget.width != W || c->budget.height != H)) return fail(c, TB_E_INVALID,
            "tb_budget_stop_converged: the sample budget is " + std::to_string(c->budget.width) + " x " + std::to_string(c->budget.height) + ", the rendered frame " +
            std::to_string(W) + " x " + std::to_string(H));
        if (!c->budget.set && opt<OPT_count_rays>(c)) return fail(c, TB_E_INVALID,
            "tb_budget_stop_converged: a sample budget and option \"count_rays\" exclude each other (the counting kernels have no list-driven copy)");
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        const size_t pixels = (size_t)W * H;
        const bool fresh = !c->budget.set; /* nobody is stopped yet: an all-live budget, the context's only once the passes have run */
        if (fresh) { ensure(c->budget.values, pixels * 4u); HIP_TRY(hipMemsetAsync(c->budget.values.p, 0xff, pixels * 4u, c->stream)); }
        try {
            ensure(c->budget.prepared, pixels * sizeof(TbFloat4)); ensure(c->budget.filtered, pixels * sizeof(TbFloat4)); ensure(c->budget.counts, 16);
            runStop(c->stream, (const TbFloat4*)c->output.p, (const TbFloat4*)c->jittered.p, (TbFloat4*)c->budget.prepared.p, (TbFloat4*)c->budget.filtered.p,
                (uint32_t*)c->budget.values.p, (unsigned long long*)c->budget.counts.p, W, H, c->samplesRendered, minFrames, relError, stopped, live,
                c->budget.ev[0].create(), c->budget.ev[1].create());
        } catch (...) { if (fresh) c->budget.values.release(); throw; } /* a failure leaves no budget the caller never asked for */
        if (hipEventElapsedTime(&c->budget.lastStopMs, c->budget.ev[0], c->budget.ev[1]) != hipSuccess) c->budget.lastStopMs = 0.0f;
        if (fresh) { c->budget.set = true; c->budget.width = W; c->budget.height = H; }
        return TB_OK;
    });
}

/* the kernel seam, like tb_run_denoise_pass: host arrays, temporary buffers, nothing of the context but its stream */
int tb_run_budget_stop(tb_context* c, uint32_t width, uint32_t height, const float* output, const float* jittered, uint32_t* budget, float relError,
    uint32_t minFrames, uint32_t frame, uint64_t* stopped, uint64_t* live)
{
    return guarded(c, [&]() {
        if (!output || !jittered || !budget) return fail(c, TB_E_INVALID, "tb_run_budget_stop: null array");
        if (const char* why = surfaceRefusal(width, height)) return fail(c, TB_E_INVALID, std::string("tb_run_budget_stop: ") + why);
        if (width > 16384u || height > 16384u) return fail(c, TB_E_INVALID, "tb_run_budget_stop: a frame has at most 16384 pixels a side");
        if (const char* why = relErrorRefusal(relError)) return fail(c, TB_E_INVALID, std::string("tb_run_budget_stop: ") + why);
        const size_t pixels = (size_t)width * height, bytes = pixels * sizeof(TbFloat4);
        const DevBuf dO = staged(output, bytes), dQ = staged(jittered, bytes), dB = staged(budget, pixels * 4u), dP = scratch(bytes), dF = scratch(bytes),
            dC = scratch(16);
        runStop(c->stream, (const TbFloat4*)dO.p, (const TbFloat4*)dQ.p, (TbFloat4*)dP.p, (TbFloat4*)dF.p, (uint32_t*)dB.p, (unsigned long long*)dC.p, width,
            height, frame, minFrames, relError, stopped, live);
        copyBack(budget, dB);
        return TB_OK;
    });
}

} // extern "C"
