/* context_radiance.cpp -- radiance queries (include/tracerboy_hip.h tb_trace_radiance / tb_make_camera_rays): the path tracer on a
 * caller's rays, per ray the sum of its samples out, on host arrays (staged by query_call.h's QueryIo, nothing kept) or on device buffers.
 * Reads the scene, the camera and the options; writes nothing of the context but the query's own work counter and overflow stacks. */
#include "query_call.h"
#include "radiance_trace.h"

#include <cstdlib>

using namespace tbhost;
using namespace tbctx;

namespace {

/* Diagnostics of scripts/radiance_rate.py and of the tests, read at every call; they change no answer.  TB_RAD_FORM: 0 one ray per lane, 1 the
 * refilling grid; TB_RAD_GRID: workgroups of the refilling grid; TB_RAD_CHUNK, TB_RAD_REFILL: the pool's size and the idle lanes at which a wave
 * draws; TB_RAD_MAX_PATHS: paths of one launch.  Unset, empty or out of range: what ships. */
int64_t diagnostic(const char* name, int64_t lo, int64_t hi, int64_t otherwise)
{
    const char* e = getenv(name);
    if (!e || !*e) return otherwise;
    char* end = nullptr;
    const long long v = strtoll(e, &end, 10);
    return end && !*end && v >= lo && v <= hi ? (int64_t)v : otherwise;
}

/* Which form runs where nobody says: the refilling grid, whatever the ray count, the samples per ray and the triangle count.  With pools of 64
 * (scripts/radiance_rate.py, DESIGN.md section 22: cornell-box and 870 k triangles, 2 M rays) it is 2 to 16 % ahead of one ray per lane on camera
 * rays and on hemispheres in pixel order, half as fast again on shuffled hemispheres, and behind in one place, by 4 %: 16 samples of cornell-box
 * camera rays.  No observable separates that case from its neighbours well enough to pay for a rule. */
uint32_t defaultForm(uint64_t, uint32_t, uint32_t) { return 1u; }

int variantIdOf(uint32_t features)
{
    for (int i = 0; i < kNumVariants; i++) if (kVariants[i].features() == features) return kVariants[i].id;
    return -1;
}

} // namespace

/* The launch of a query on device buffers, waited for: the feature set, the stack plan, the form and the grid, the frame constants, rad_launch between
 * the query's two events.  tb_trace_radiance and tb_bake_lightmap (context_bake.cpp) both end here.  who: the entry point's name, for the refusal. */
int tbctx::traceRadianceOnDevice(tb_context* c, const char* who, const tb_output_settings& s, float time, const RadCall& k, uint64_t n, const TbRadianceRay* rays,
    TbFloat4* out)
{
    /* the feature set: pickVariantAndPlan's loop over the sets the kernel is compiled for */
    uint32_t need = c->sceneFeatures | settingsFeatureMask(c, s, false);
    const bool alphaTest = opt<OPT_alpha_test>(c) != 0;
    if (alphaTest) need |= PT_FEAT_EXT;
    const int numSets = (int)(sizeof(kRadFeatureSets) / sizeof(kRadFeatureSets[0]));
    RadPlan plan{};
    plan.features = kRadFeatureSets[numSets - 1];
    for (int i = 0; i < numSets; i++) if ((need & ~kRadFeatureSets[i]) == 0) { plan.features = kRadFeatureSets[i]; break; }
    plan.stack = guide_stack_plan(c->ds.stackDepth, (uint32_t)std::max<int64_t>(0, opt<OPT_stack_overflow_max>(c)),
        (uint32_t)std::max<int64_t>(0, std::min<int64_t>(opt<OPT_stack_lds_cap>(c), 0xffff)));
    if (!plan.stack.ok) return fail(c, TB_E_UNSUPPORTED, std::string(who) + ": traversal stack of depth " + std::to_string(c->ds.stackDepth) +
        " does not fit LDS; unsupported");
    plan.form = (uint32_t)diagnostic("TB_RAD_FORM", 0, 1, defaultForm(n, k.numSamples, c->ds.numTris));
    plan.chunk = (uint32_t)diagnostic("TB_RAD_CHUNK", 16, 65536, RAD_CHUNK);
    plan.refillMin = (uint32_t)diagnostic("TB_RAD_REFILL", 1, 64, RAD_REFILL_MIN);
    plan.maxPaths = (uint32_t)diagnostic("TB_RAD_MAX_PATHS", 1, 0xffffffffll, RAD_MAX_PATHS);
    HIP_TRY(rad_plan_grid(&plan, n, (uint32_t)diagnostic("TB_RAD_GRID", 1, 65535, 0)));
    if (plan.stack.overflowEntries) ensure(c->rad.overflow, (size_t)plan.stack.overflowEntries * plan.stack.lanes * 4);
    if (plan.form && !c->rad.counter.p) ensure(c->rad.counter, 64);
    TbDeviceScene ds = c->ds; ds.alphaTest = alphaTest ? 1u : 0u;
    TbPerFrameConstants pf;
    MakeFrameConstants(c->scene, c->camera, s, k.firstSample, time, 0xffffffffu, 0xffffffffu, pf);
    if (pf.OutputMode == TB_OUTPUT_TYPE_HEATMAP) pf.OutputMode = TB_OUTPUT_TYPE_LIT; /* a query has no heatmap: the path goes on past its first hit */
    timed(c->stream, c->rad.ev, c->rad.lastMs, [&]() { return rad_launch(c->stream, &ds, &pf, &k, &plan,
        plan.stack.overflowEntries ? (uint32_t*)c->rad.overflow.p : nullptr, (uint32_t*)c->rad.counter.p, n, rays, out, &c->rad.lastLaunches); }, true);
    c->rad.lastVariant = variantIdOf(plan.features); c->rad.lastForm = (int)plan.form;
    return TB_OK;
}

extern "C" int tb_trace_radiance(tb_context* c, const tb_output_settings* settings, float time, const TbRadianceCall* call, uint64_t n,
    const TbRadianceRay* rays, TbFloat4* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_trace_radiance", "a query's rays are traced on one device")) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (tb_radiance_refusal(call, n, rays, out, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_trace_radiance: ") + why);
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        const tb_output_settings s = settingsOrDefault(settings);
        if (s.RenderModeRealTime) return fail(c, TB_E_UNSUPPORTED, "tb_trace_radiance: the real-time mode is not supported: a query has no AOVs and no history");
        if (n == 0) return TB_OK;
        const bool accumulate = (call->mode_and_flags & TB_RADIANCE_ACCUMULATE) != 0;
        QueryIo io(c, "tb_trace_radiance", (call->mode_and_flags & TB_RADIANCE_DEVICE) != 0);
        const TbRadianceRay* r = io.in("rays", rays, (size_t)n * sizeof(TbRadianceRay));
        TbFloat4* o = io.out("out", out, (size_t)n * sizeof(TbFloat4), accumulate); /* the sums start from what the caller's array holds */
        const RadCall k{call->first_sample, call->num_samples, (call->mode_and_flags & 0xffu) == TB_RADIANCE_HEMISPHERE ? 1u : 0u, accumulate ? 1u : 0u, call->seed_advance};
        const int rc = traceRadianceOnDevice(c, "tb_trace_radiance", s, time, k, n, r, o);
        if (rc != TB_OK) return rc;
        io.finish();
        return TB_OK;
    });
}

extern "C" int tb_make_camera_rays(tb_context* c, const tb_output_settings* settings, float time, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t x1,
    uint32_t y1, uint32_t frame, uint32_t flags, TbRadianceRay* out, float* seedAdvance)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_make_camera_rays", "a query's rays are traced on one device")) return rc;
    return guarded(c, [&]() {
        if (flags & ~TB_RADIANCE_DEVICE) return fail(c, TB_E_INVALID, "tb_make_camera_rays: unknown flag bits");
        if (!out || !seedAdvance) return fail(c, TB_E_INVALID, "tb_make_camera_rays: null pointer");
        if (const char* no = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_make_camera_rays: ") + no);
        if (W > 16384u || H > 16384u) return fail(c, TB_E_INVALID, "tb_make_camera_rays: a dimension above 16384");
        if (x0 >= x1 || y0 >= y1 || x1 > W || y1 > H) return fail(c, TB_E_INVALID, "tb_make_camera_rays: the window is empty or leaves the picture");
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        const tb_output_settings s = settingsOrDefault(settings);
        if (s.FilterType != TB_FILTER_TYPE_BOX) return fail(c, TB_E_UNSUPPORTED,
            "tb_make_camera_rays: a triangle or Gaussian pixel filter is not supported: its samples carry a weight and the ray record has none");
        const bool device = (flags & TB_RADIANCE_DEVICE) != 0;
        if (device && ((uintptr_t)out & 15u)) return fail(c, TB_E_INVALID, "tb_make_camera_rays: device rays are not 16-B aligned");
        QueryIo io(c, "tb_make_camera_rays", device);
        TbRadianceRay* o = io.out("out", out, (size_t)(x1 - x0) * (y1 - y0) * sizeof(TbRadianceRay));
        const DevBuf dAdvance = scratch(4);
        TbPerFrameConstants pf;
        MakeFrameConstants(c->scene, c->camera, s, frame, time, 0xffffffffu, 0xffffffffu, pf);
        TbDeviceTargets tg; memset(&tg, 0, sizeof tg); /* the camera constants alone */
        if (opt<OPT_camera_constants>(c) != 0) cameraConstants(pf, W, H, tg);
        HIP_TRY(rad_launch_camera_rays(c->stream, &c->ds, &pf, &tg, W, H, x0, y0, x1, y1, frame, o, (float*)dAdvance.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(seedAdvance, dAdvance);
        io.finish();
        return TB_OK;
    });
}
