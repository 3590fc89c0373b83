/* context.cpp -- the core of the C ABI (include/tracerboy_hip.h) on top of the host scene code and the HIP kernels: the table of feature sets,
 * create / destroy, scene loads, camera and material edits, tb_render / tb_sync, the read-backs, tb_set_option.  The other features have files
 * of their own (the index in context_internal.h).  tb_context plays the role of `class TracerBoy` (the reference's TracerBoy.h:158-398): it owns
 * every device resource, the accumulation surfaces (OutputTexture / JitteredOutputTexture) and the sample counter (m_SamplesRendered).
 * There is no CPU rendering path in this library: every entry point that produces pixels or hits launches a HIP kernel, and tb_create fails
 * when no HIP device is usable.
 */
#include "context_internal.h"

using namespace tbhost;
using namespace tbctx;

namespace tbctx {

std::string g_createError;
std::atomic<int64_t> g_liveDeviceBytes{0};
#ifndef __HIP_DEVICE_COMPILE__ /* host data: the file goes through hipcc's device pass too, which has no use for a table of host functions */
#define TB_COPY(copy) {&kPtCopies[PT_COPY_INDEX_##copy], pt_launch_persistent_##copy},
#define TB_COPY_INDEX(copy) PT_COPY_INDEX_##copy,
enum { PT_COPY_LIST(TB_COPY_INDEX) };
static const Copy kCopies[] = { PT_COPY_LIST(TB_COPY) };
static constexpr bool sameName(const char* a, const char* b) { for (; *a == *b; a++, b++) if (!*a) return true; return false; }
static const Copy* copyOf(const char* set, int role) /* the set's copy in that role, if it has one */
{
    for (const Copy& k : kCopies) if (k.row->role == role && sameName(k.row->set, set)) return &k;
    return nullptr;
}
#define TB_SET(set) .name = #set, .base = copyOf(#set, PT_ROLE_BASE), .hi = copyOf(#set, PT_ROLE_OCCUPANCY), .lds = copyOf(#set, PT_ROLE_LDS_GROUPS)
const Variant kVariants[] = {
    {TB_SET(matte), .id = 0, .wf = wf_launch_matte, .pooled = true, .split = pt_launch_split_matte},
    {TB_SET(env), .id = 1, .wf = wf_launch_env, .pooled = true, .split = pt_launch_split_env},
    {TB_SET(surf), .id = 2, .wf = wf_launch_surf, .pooled = true, .split = pt_launch_split_surf},
    {TB_SET(sss), .id = 5, .wf = wf_launch_sss, .pooled = false, .split = pt_launch_split_sss},
    {TB_SET(vol), .id = 3, .wf = wf_launch_vol, .pooled = false, .split = nullptr},
    {TB_SET(full), .id = 4, .wf = nullptr, .pooled = false, .split = nullptr},
};
const int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));
#endif

int fail(tb_context* c, int code, const std::string& msg) { if (c) c->err = msg; else g_createError = msg; return code; }

void ensure(DevBuf& b, size_t bytes)
{
    if (b.bytes == bytes && b.p) return;
    b.release();
    if (bytes == 0) return;
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    g_liveDeviceBytes += (int64_t)bytes;
}
} // namespace tbctx

extern "C" {

int tb_create(tb_context** out, int device_id)
{
    if (!out) return TB_E_INVALID;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, TB_E_NO_DEVICE,
        std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") + " (libtracerboy_hip has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return fail(nullptr, TB_E_INVALID, "tb_create: device id out of range");
    tb_context* c = new tb_context();
    c->device = device_id;
    try {
        HIP_TRY(hipSetDevice(device_id));
        c->stream.create();
        c->ev0.create(); c->ev1.create(); c->evKernel.create(); c->evKernelStart.create();
        c->evMain.create(hipEventDisableTiming);
        for (int i = 0; i < 2; i++) { c->side[i].create(); c->evPt[i].create(hipEventDisableTiming); c->evFold[i].create(hipEventDisableTiming); }
    } catch (const std::exception& ex) { g_createError = ex.what(); delete c; return TB_E_DEVICE; }
    *out = c;
    return TB_OK;
}

/* What only this function knows: the peers go first, the context's device is current for every free (and stays the calling thread's device, as it
 * always has), nothing is in flight.  The members give their resources back themselves (context_internal.h). */
void tb_destroy(tb_context* c)
{
    if (!c) return;
    for (tb_context* p : c->group.peers) { p->group.owner = nullptr; tb_destroy(p); }
    c->group.peers.clear();
    (void)hipSetDevice(c->device);
    for (hipStream_t s : {(hipStream_t)c->stream, (hipStream_t)c->side[0], (hipStream_t)c->side[1]}) if (s) (void)hipStreamSynchronize(s);
    delete c;
}

const char* tb_last_error(tb_context* c) { return c ? c->err.c_str() : g_createError.c_str(); }

int tb_load_scene(tb_context* c, const char* path)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (!path) return fail(c, TB_E_INVALID, "tb_load_scene: null path");
        std::shared_ptr<PbrtScene> ps = importScene(path);
        ConvertOptions co; /* whose defaults hold for an option nobody set */
        if (const int64_t* v = c->options.ifSet<OPT_flatten_instances>()) co.flattenInstances = *v != 0;
        if (const int64_t* v = c->options.ifSet<OPT_flip_texture_uvs>()) co.flipTextureUVs = *v != 0;
        c->hasScene = false;
        ConvertScene(*ps, c->scene, co);
        finalizeScene(c);
        return shareSceneWithPeers(c);
    });
}

int tb_load_procedural(tb_context* c, int kind, uint32_t targetTriangles, uint32_t seed)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        c->hasScene = false;
        MakeProceduralScene(c->scene, kind, targetTriangles, seed);
        finalizeScene(c);
        return shareSceneWithPeers(c);
    });
}

int tb_scene_info_get(tb_context* c, tb_scene_info* o)
{
    if (!c || !o) return TB_E_INVALID;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    return guarded(c, [&]() { refreshHostScene(c); fillSceneInfo(c->scene, o); return TB_OK; });
}

void tb_default_output_settings(tb_output_settings* o) { if (o) DefaultOutputSettings(*o); }

int tb_get_camera(tb_context* c, tb_camera* o) { if (!c || !o) return TB_E_INVALID; if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    *o = c->camera; return TB_OK; }
int tb_set_camera(tb_context* c, const tb_camera* cam)
{
    if (!c || !cam) return TB_E_INVALID;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    c->camera = *cam; c->ds.config.CameraLensHeight = cam->LensHeight; c->scene.config.CameraLensHeight = cam->LensHeight; resetHistory(c);
    for (tb_context* p : c->group.peers) { const int rc = tb_set_camera(p, cam); if (rc != TB_OK) return rc; }
    return TB_OK;
}

int tb_material_count(tb_context* c) { return (c && c->hasScene) ? (int)c->scene.materials.size() : 0; }
int tb_get_material(tb_context* c, int id, TbMaterial* o)
{
    if (!c || !o) return TB_E_INVALID;
    if (!c->hasScene || id < 0 || id >= (int)c->scene.materials.size()) return fail(c, TB_E_INVALID, "material id out of range");
    *o = c->scene.materials[(size_t)id]; return TB_OK;
}
int tb_set_material(tb_context* c, int id, const TbMaterial* in)
{
    return guarded(c, [&]() {
        if (!in || !c->hasScene || id < 0 || id >= (int)c->scene.materials.size()) return fail(c, TB_E_INVALID, "material id out of range");
        c->scene.materials[(size_t)id] = *in;
        HIP_TRY(hipMemcpy((void*)&c->ds.materials[id].m, in, sizeof *in, hipMemcpyHostToDevice));
        c->sceneFeatures = sceneFeatureMask(c->scene);
        c->ds.textureUse = sceneTextureUse(c); /* the edit may be the scene's first texture or normal map */
        resetHistory(c); c->materialEdits++; /* (c->tablesInRange stands: the edit changes no count and no index) */
        for (tb_context* p : c->group.peers) { const int rc = tb_set_material(p, id, in); if (rc != TB_OK) return rc; }
        return TB_OK;
    });
}

int tb_render(tb_context* c, uint32_t W, uint32_t H, uint32_t n, const tb_output_settings* s, float t)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) { const int rc = renderGroup(c, W, H, n, s, t); return rc != TB_OK ? rc : tb_sync(c); }
    return guarded(c, [&]() { c->rt.lastRender = false; touchAccumulation(c); return renderImpl(c, W, H, n, s, t, true); });
}
int tb_render_async(tb_context* c, uint32_t W, uint32_t H, uint32_t n, const tb_output_settings* s, float t)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return renderGroup(c, W, H, n, s, t);
    return guarded(c, [&]() { c->rt.lastRender = false; touchAccumulation(c); return renderImpl(c, W, H, n, s, t, false); });
}
int tb_sync(tb_context* c)
{
    if (c) for (tb_context* p : c->group.peers) { const int rc = tb_sync(p);
        if (rc != TB_OK) return fail(c, rc, "peer device " + std::to_string(p->device) + ": " + p->err); }
    return guarded(c, [&]() {
        HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipEventElapsedTime(&c->lastMs, c->ev0, c->ev1);
        if (hipEventElapsedTime(&c->lastKernelMs, c->evKernelStart, c->evKernel) != hipSuccess) c->lastKernelMs = c->lastMs;
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        return TB_OK;
    });
}

int tb_read_accum(tb_context* c, float* rgba, float* jit)
{
    return guarded(c, [&]() {
        if (!c->output.p) return fail(c, TB_E_INVALID, "tb_read_accum: nothing rendered yet");
        HIP_TRY(hipStreamSynchronize(c->stream));
        /* an asynchronous render of the split-role kernel that gave up leaves an incomplete frame: say so here too, not only in tb_sync */
        if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c));
        if (rgba) HIP_TRY(hipMemcpy(rgba, c->output.p, c->output.bytes, hipMemcpyDeviceToHost));
        if (jit) HIP_TRY(hipMemcpy(jit, c->jittered.p, c->jittered.bytes, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_read_aov(tb_context* c, int which, void* dst)
{
    return guarded(c, [&]() {
        if (which < 2 || which > 7 || !dst || !c->aov[which].p) return fail(c, TB_E_INVALID,
            "tb_read_aov: AOV not available (set option \"aov\" before rendering)");
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(dst, c->aov[which].p, c->aov[which].bytes, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

int tb_accum_device_ptr(tb_context* c, void** o, void** j)
{
    if (!c) return TB_E_INVALID;
    /* the abort word of the split-role kernel is host-mapped: a launch that has already given up is reported without waiting for anything --
     * and WITHOUT consuming the report (tb_sync / tb_read_accum on the same incomplete frame must still fail), with no pointer
     * handed out */
    if (c->splitAbort && *c->splitAbort) return fail(c, TB_E_DEVICE, splitAbortMessage(c, false));
    if (o) *o = c->output.p;
    if (j) *j = c->jittered.p;
    return c->output.p ? TB_OK : TB_E_INVALID;
}

int tb_read_stats(tb_context* c, tb_readback_stats* o)
{
    return guarded(c, [&]() {
        if (!o) return TB_E_INVALID;
        memset(o, 0, sizeof *o);
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->stats.p) { uint32_t raw[4]; HIP_TRY(hipMemcpy(raw, c->stats.p, 16, hipMemcpyDeviceToHost)); o->ActiveWaves = raw[0]; o->ActivePixels = raw[1];
            memcpy(&o->SelectedPixelDistance, &raw[2], 4); o->SelectedMaterialID = (int32_t)raw[3]; }
        if (c->rayStats.p) { uint64_t r[7]; HIP_TRY(hipMemcpy(r, c->rayStats.p, 56, hipMemcpyDeviceToHost)); o->rays.boxesTested = r[0];
            o->rays.trianglesTested = r[1]; o->rays.hitsShaded = r[2]; o->rays.materialFetches = r[3]; o->rays.lightSamples = r[4]; o->rays.samples = r[5];
            o->rays.rays = r[6]; }
        return TB_OK;
    });
}

int tb_read_wave_profile(tb_context* c, uint64_t* out14)
{
    return guarded(c, [&]() {
        if (!out14 || !c->rayStats.p) return fail(c, TB_E_INVALID, "tb_read_wave_profile: render with option \"count_rays\" first");
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out14, (const char*)c->rayStats.p + 56, 14 * 8, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

static const Variant* variantNamed(const char* name)
{
    if (name) for (int i = 0; i < kNumVariants; i++) if (!strcmp(kVariants[i].name, name)) return &kVariants[i];
    return nullptr;
}
int tb_variant_stash_entries(const char* name) { const Variant* v = variantNamed(name); return v ? (int)v->stashHi() : -1; }
int tb_variant_waves_hi(const char* name) { const Variant* v = variantNamed(name); return v ? (int)v->wavesHi() : -1; }
int tb_variant_waves_lds(const char* name) { const Variant* v = variantNamed(name); return v ? (int)v->wavesLds() : -1; }

int tb_read_split_profile(tb_context* c, uint64_t* out16)
{
    return guarded(c, [&]() {
        if (!out16 || !c->splitProf.p) return fail(c, TB_E_INVALID,
            "tb_read_split_profile: render with options \"pipeline\" = 4 and \"split_profile\" = 1 first");
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out16, c->splitProf.p, 16 * 8, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

void tb_invalidate_history(tb_context* c) { if (c) { resetHistory(c); for (tb_context* p : c->group.peers) resetHistory(p); } }
uint32_t tb_samples_rendered(tb_context* c) { return c ? c->samplesRendered : 0; }
/* (a group renders the selection on the device that owns the pixel's tile; ReadbackStats reads the owner's buffer) */
int tb_select_pixel(tb_context* c, uint32_t x, uint32_t y) { if (!c) return TB_E_INVALID; c->selX = x; c->selY = y; return TB_OK; }

void* tb_stream(tb_context* c) { return c ? (void*)c->stream.s : nullptr; }

int tb_set_option(tb_context* c, const char* name, int64_t v)
{
    if (!c || !name) return TB_E_INVALID;
    const int k = FindOption(name);
    if (k < 0) return fail(c, TB_E_INVALID, std::string("unknown option '") + name + "'");
    if ((kOptions[k].flags & OPT_NOT_NEGATIVE) && v < 0) return fail(c, TB_E_INVALID, std::string("tb_set_option: ") + name + " must not be negative");
    /* adaptive_test 0: the skip test runs before every frame (the reference's); 1: once per call, at its first frame */
    if ((kOptions[k].flags & OPT_ZERO_OR_ONE) && v != 0 && v != 1) return fail(c, TB_E_INVALID, std::string("tb_set_option: ") + name +
        " is 0 (before every frame) or 1 (once per call)");
    if (k == OPT_denoise_guides && (v < 0 || v > 2)) return fail(c, TB_E_INVALID,
        "tb_set_option: denoise_guides is 0 (the last frame's AOVs), 1 (the guide pass's normals and positions) or 2 (1 + albedo demodulation)");
    /* the adaptive launch has no counting copy */
    if (v && ((k == OPT_adaptive && opt<OPT_count_rays>(c)) || (k == OPT_count_rays && opt<OPT_adaptive>(c))))
        return fail(c, TB_E_INVALID, "tb_set_option: options \"adaptive\" and \"count_rays\" exclude each other (the counting kernels have no adaptive copy)");
    /* ... nor has a call under a sample budget, which runs the same launch */
    if (v && k == OPT_count_rays && c->budget.set) return fail(c, TB_E_INVALID,
        "tb_set_option: option \"count_rays\" and a sample budget exclude each other (the counting kernels have no list-driven copy): clear the budget first");
    c->options.value[k] = v; c->options.isSet[k] = true;
    if (kOptions[k].flags & OPT_RESETS_HISTORY) resetHistory(c);
    return TB_OK;
}

int tb_host_scene_view(tb_context* c, TbSceneView* v)
{
    if (!c || !v) return TB_E_INVALID;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    const int rc = guarded(c, [&]() { refreshHostScene(c); return TB_OK; }); /* a commit leaves the host geometry stale (context_dynamic.cpp) */
    if (rc != TB_OK) return rc;
    fillView(c->scene, v);
    return TB_OK;
}

int tb_make_frame_constants(tb_context* c, uint32_t, uint32_t, uint32_t frame, const tb_output_settings* settings, float t, TbPerFrameConstants* out)
{
    if (!c || !out) return TB_E_INVALID;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    tb_output_settings s; if (settings) s = *settings; else DefaultOutputSettings(s);
    MakeFrameConstants(c->scene, c->camera, s, frame, t, c->selX, c->selY, *out);
    return TB_OK;
}

float tb_last_render_ms(tb_context* c) { return c ? c->lastMs : 0.0f; }

/* The two test hooks of pt_kernels.hip, on host arrays (staged, context_internal.h) */
int tb_trace_closest(tb_context* c, uint32_t n, const float* origins, const float* dirs, float* outT, int32_t* outMat, float* outBary, uint32_t* outPrim,
                     uint32_t* outGeom, float* outNormal, float* outUV, uint32_t* outBoxes, uint32_t* outTris)
{
    return guarded(c, [&]() {
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        if (n == 0) return TB_OK;
        if (!origins || !dirs || !outT) return fail(c, TB_E_INVALID, "tb_trace_closest: null array");
        const size_t n4 = (size_t)n * 4;
        const DevBuf dO = staged(origins, n4 * 3), dD = staged(dirs, n4 * 3), dT = scratch(n4), dM = scratch(n4), dB = scratch(n4 * 2), dP = scratch(n4),
            dG = scratch(n4), dN = scratch(n4 * 3), dU = scratch(n4 * 2), dBx = scratch(n4), dTr = scratch(n4);
        if (opt<OPT_node_layout>(c) == 1) ensureCompactNodes(c);
        TbDeviceScene dsTrace = c->ds; /* option "node_layout" = 1: the batch walks the compact nodes too (one-level scenes) */
        if (opt<OPT_node_layout>(c) != 1 || dsTrace.numInstances) dsTrace.nodesC = nullptr;
        HIP_TRY(pt_launch_trace_closest(c->stream, &dsTrace, n, (const float*)dO.p, (const float*)dD.p, (float*)dT.p, (int*)dM.p, (float*)dB.p, (uint32_t*)dP.p,
                                        (uint32_t*)dG.p, (float*)dN.p, (float*)dU.p, (uint32_t*)dBx.p, (uint32_t*)dTr.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(outT, dT); copyBack(outMat, dM); copyBack(outBary, dB); copyBack(outPrim, dP); copyBack(outGeom, dG);
        copyBack(outNormal, dN); copyBack(outUV, dU); copyBack(outBoxes, dBx); copyBack(outTris, dTr);
        return TB_OK;
    });
}

int tb_device_math(tb_context* c, int fn, uint32_t n, const float* a, const float* b, float* out)
{
    return guarded(c, [&]() {
        if (!a || !out) return fail(c, TB_E_INVALID, "tb_device_math: null array");
        if (n == 0) return TB_OK;
        const DevBuf dA = staged(a, (size_t)n * 4), dB = b ? staged(b, (size_t)n * 4) : DevBuf(), dO = scratch((size_t)n * 4);
        HIP_TRY(pt_launch_device_math(c->stream, fn, n, (const float*)dA.p, (const float*)dB.p, (float*)dO.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dO);
        return TB_OK;
    });
}

} // extern "C"
