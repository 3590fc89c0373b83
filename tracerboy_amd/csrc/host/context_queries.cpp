/* context_queries.cpp -- tb_get_option (include/tracerboy_hip.h): the read-only names, what the library reports of its last calls and of the loaded
 * scene, as rows of one table beside the options of options.h. */
#include "context_internal.h"

using namespace tbhost;
using namespace tbctx;

namespace {

int64_t microseconds(float ms) { return (int64_t)(ms * 1000.0f + 0.5f); }
int64_t address(const DevBuf& b) { return (int64_t)(uintptr_t)b.p; }

/* hit records of the primary-visibility pre-pass that failed validation since the context was made */
int64_t prepassRejects(tb_context* c)
{
    uint32_t v = 0;
    if (c->debugCounters.p) { (void)hipStreamSynchronize(c->stream); (void)hipMemcpy(&v, c->debugCounters.p, 4, hipMemcpyDeviceToHost); }
    return v;
}
/* the owned pixels that were live at the first frame of the last call (all owned pixels of a call that did not run the adaptive launch) -- a device
 * word: reading it waits for the call; -1 when it cannot be read.  A group's owner counts its peers' too. */
int64_t lastLivePixels(tb_context* c)
{
    int64_t sum = 0;
    for (tb_context* x : members(c)) {
        if (!x->lastAdaptive || !x->liveList.p) { sum += (int64_t)x->lastOwnedPixels; continue; }
        uint32_t v = 0; DeviceScope scope(x->device);
        if (hipStreamSynchronize(x->stream) != hipSuccess || hipMemcpy(&v, (const uint8_t*)x->liveList.p + x->liveCountOffset, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        sum += v;
    }
    return sum;
}
int64_t lastVariantId(tb_context* c) /* 0 matte 1 env 2 surf 3 vol 4 full 5 sss */
{
    for (int i = 0; i < kNumVariants; i++) if (c->lastVariant == kVariants[i].name) return kVariants[i].id;
    return -1;
}

/* The read-only names.  tb_get_option searches this table first, then the options, and answers 0 to any other name.  Two rules follow:
 *  - a row shadows an option of the same name: "adaptive_min_frames" answers with its default where nobody set it, unlike every other option;
 *  - an option nobody set reads as 0, not as its default (callers rely on it; reporting the default is a change of its own). */
struct Query { const char* name; int64_t (*read)(tb_context*); };
#define Q(name, expr) {name, [](tb_context* c) -> int64_t { return (int64_t)(expr); }},
const Query kQueries[] = {
    Q("scene_in_lds_active", c->sceneInLds ? 1 : 0) Q("scene_features", c->sceneFeatures)
    Q("last_kernel_us", microseconds(c->lastKernelMs)) /* first path-tracing launch of the last synchronous render */
    Q("last_kernel_frames", c->lastKernelFrames) Q("last_primary_prepass", c->lastPrimaryPrepass) Q("last_first_bounce", c->lastFirstBounce)
    Q("last_compact_hits", c->lastCompactHits) /* 1: the last render's pre-pass wrote 16-B hit records (pt_scene.h) */
    Q("debug_slot_log_ptr", address(c->fgSlotLog[c->lastFgPar])) Q("debug_slot_log_cap", c->lastSlotLogCap)
    Q("debug_fg_samples_ptr", address(c->fgSamples[c->lastFgPar])) /* the sample buffer of the last frame-group launch (scripts/lost_item_stress.py) */
    Q("last_node_layout", c->lastNodeLayout) /* 0: layout B (64-B nodes), 1: layout C (32-B nodes on the 16-bit grid) */
    Q("debug_prepass_rejects", prepassRejects(c))
    Q("last_overlap", c->lastOverlap) /* the last frame-group render used the two side streams */
    /* best device-bound interval between call ends, overlapped / one at a time; 0 measuring overlapped, 1 measuring one at a time, 2 decided */
    Q("overlap_trial_us_overlapped", c->overlapTrial.best[0] * 1000.0f) Q("overlap_trial_us_one_at_a_time", c->overlapTrial.best[1] * 1000.0f)
    Q("overlap_trial_phase", c->overlapTrial.phase)
    Q("last_plan_rule_pipeline", c->lastPlan.rule_pipeline) /* TB_PLAN_RULE_* of the last render (tracerboy_hip.h) */
    Q("last_plan_rule_copy", c->lastPlan.rule_copy) Q("last_plan_rule_prepass", c->lastPlan.rule_prepass) Q("last_plan_frame_group", c->lastPlan.frame_group)
    Q("last_plan_guided_groups", c->lastPlan.guided_groups) Q("last_plan_costly_first", c->lastPlan.costly_first)
    Q("last_plan_stack_overflow", c->lastPlan.stack_overflow_entries)
    Q("debug_region_order_ptr", address(c->regionOrder[c->lastFgPar])) Q("debug_region_cost_ptr", address(c->regionCost))
    Q("debug_live_device_bytes", g_liveDeviceBytes.load()) /* every context of the process (DevBuf), not this one only */
    Q("last_split_waves", c->lastSplitWaves) /* traversal waves * 100 + shading waves per workgroup of the last pipeline-4 launch */
    Q("last_pipeline", c->lastPipeline) /* the pipeline the last render actually ran (2 / 3 fall back to 0 for feature sets they lack) */
    /* render states: GPU microseconds (HIP events) of the last digest of the two surfaces / of the last TB_STATE_ADD's sum; the first frame held */
    Q("last_state_digest_us", microseconds(c->lastStateDigestMs)) Q("last_state_add_us", microseconds(c->lastStateAddMs))
    Q("state_first_frame", c->firstFrame)
    Q("last_denoise_us", microseconds(c->dn.lastMs)) /* the last tb_denoise, prepare to finish (HIP events) */
    /* the last tb_upscale: its FSR passes together, its EASU passes, its RCAS passes (HIP events; both chains when both ran) */
    Q("last_upscale_us", microseconds(c->fsr.lastUpscaleMs)) Q("last_easu_us", microseconds(c->fsr.lastEasuMs))
    Q("last_rcas_us", microseconds(c->fsr.lastRcasMs))
    /* the neural still denoiser: the last network, pack to unpack (HIP events); the input channels of the loaded weights, 0 = none */
    Q("last_neural_us", microseconds(c->nn.lastMs)) Q("neural_inputs", c->nn.inputs)
    /* the neural 2 x super-resolution: the last network, pack to finish (HIP events); weights are loaded; the form its convolutions run in (the option, or
     * its default where nobody set it) */
    Q("last_sr_us", microseconds(c->sr.lastMs)) Q("sr_loaded", c->sr.loaded ? 1 : 0) Q("sr_conv_form", opt<OPT_sr_conv_form>(c))
    Q("last_guides_us", microseconds(c->guides.lastMs)) /* the last tb_render_guides, its kernel alone (HIP events) */
    Q("last_guides_stack_overflow", c->guides.lastOverflow) /* stack entries per lane the last pass kept in global memory (the HYBRID form) */
    /* the path inspector: the last tb_record_paths (both runs and the scan) and the last tb_visualize_rays (HIP events); where the last overlay took
     * its occluder from: 1 the last frame's world-position AOV, 2 the guide pass's mean position, 0 nowhere */
    Q("last_paths_us", microseconds(c->vis.lastPathsMs)) Q("last_visualize_us", microseconds(c->vis.lastOverlayMs))
    Q("visualize_depth_source", c->vis.depthSource)
    /* dynamic scenes: the kernels of the last refit (HIP events); the scene holds a dynamic state; its host geometry is stale */
    Q("last_refit_us", microseconds(c->dyn ? c->dyn->lastMs : 0.0f)) Q("dynamic_state", c->dyn ? 1 : 0) Q("host_geometry_stale", c->dyn && c->dyn->hostStale ? 1 : 0)
    /* radiance queries: the last query's launches (HIP events), its feature set (the ids of last_variant), its form (0 one ray
     * per lane, 1 the refilling grid) and how many launches it was split into */
    Q("last_radiance_us", microseconds(c->rad.lastMs)) Q("last_radiance_variant", c->rad.lastVariant) Q("last_radiance_form", c->rad.lastForm)
    Q("last_radiance_launches", c->rad.lastLaunches)
    Q("last_nearest_us", microseconds(c->pq.lastMs)) /* point queries: the last query's kernel (HIP events) */
    /* winding numbers: the last call's walk and the last moment fit (HIP events) */
    Q("last_winding_us", microseconds(c->wn ? c->wn->lastMs : 0.0f)) Q("last_winding_fit_us", microseconds(c->wn ? c->wn->lastFitMs : 0.0f))
    /* lightmap baking: the last bake's rasteriser, its query's launches, its resolve and fill passes (HIP events); the texels
     * that have a triangle */
    Q("last_bake_raster_us", microseconds(c->bake ? c->bake->lastRasterMs : 0.0f)) Q("last_bake_trace_us", microseconds(c->bake ? c->bake->lastTraceMs : 0.0f))
    Q("last_bake_finish_us", microseconds(c->bake ? c->bake->lastFinishMs : 0.0f)) Q("last_bake_covered", c->bake ? c->bake->lastCovered : 0u)
    Q("bake_width", c->bake && c->bake->held ? c->bake->width : 0u) Q("bake_height", c->bake && c->bake->held ? c->bake->height : 0u) /* of the bake held; 0: none */
    /* light probes: the last bake's four stages summed over its batches (HIP events; the trace is the radiance query's own), its
     * batches, and what is held */
    Q("last_probes_rays_us", microseconds(c->probes ? c->probes->lastRaysMs : 0.0f)) Q("last_probes_trace_us", microseconds(c->probes ? c->probes->lastTraceMs : 0.0f))
    Q("last_probes_hits_us", microseconds(c->probes ? c->probes->lastHitsMs : 0.0f)) Q("last_probes_project_us", microseconds(c->probes ? c->probes->lastProjectMs : 0.0f))
    Q("last_probes_batches", c->probes ? c->probes->lastBatches : 0u) Q("probes_held", c->probes && c->probes->held ? c->probes->n : 0u)
    Q("probes_resolution", c->probes && c->probes->held ? c->probes->resolution : 0u) Q("probes_maps_held", c->probes && c->probes->held && c->probes->mapsHeld ? 1 : 0)
    Q("last_copy_waves", c->lastCopyWaves)
    Q("last_adaptive", c->lastAdaptive ? 1 : 0) /* the adaptive launch: did the last call run it */
    /* sample budgets: one is set; the last call was planned under it (its live pixels: last_live_pixels) */
    Q("budget_set", c->budget.set ? 1 : 0) Q("last_budgeted", c->budget.lastBudgeted ? 1 : 0)
    Q("last_budget_stop_us", microseconds(c->budget.lastStopMs)) /* the last tb_budget_stop_converged: prepare, prefilter, stop (HIP events) */
    Q("adaptive_min_frames", opt<OPT_adaptive_min_frames>(c))
    Q("last_live_pixels", lastLivePixels(c)) Q("last_variant", lastVariantId(c))
};
#undef Q

} // namespace

extern "C" int64_t tb_get_option(tb_context* c, const char* name)
{
    if (!c || !name) return 0;
    for (const Query& q : kQueries) if (!strcmp(name, q.name)) return q.read(c);
    const int k = FindOption(name); return k >= 0 && c->options.isSet[k] ? c->options.value[k] : 0;
}
