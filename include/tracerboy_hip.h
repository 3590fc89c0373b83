/* tracerboy_hip.h -- C ABI of libtracerboy_hip.so, the MI355X-native drop-in for TracerBoy's
 * path-tracing hot path.
 *
 * The reference has no FFI; the path sits behind the host seam `class TracerBoy`
 * (/root/reference/TracerBoy/TracerBoy.h:158-398, called from D3D12App.cpp:52,76,213,222,235,240).
 * Each entry point below names the member it replaces.  Conventions: plain pointers and sizes,
 * no C++/torch/D3D types; return 0 on success or a negative TB_E_* code (never abort -- the
 * reference's VERIFY -> assert(false), pch.h:45-47, becomes an error code + tb_last_error());
 * the caller owns every host buffer it passes; a context is not thread-safe and drives ONE GPU
 * (one process per GPU; multi-GPU = one context per rank, see tb_set_tile_assignment).
 * There is no CPU fallback: without a HIP device tb_create fails with TB_E_NO_DEVICE.
 */
#ifndef TRACERBOY_HIP_H
#define TRACERBOY_HIP_H

#include <stdint.h>
#include "tb_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TB_OK 0
#define TB_E_INVALID -1      /* bad argument / call order */
#define TB_E_NO_DEVICE -2    /* no usable HIP device */
#define TB_E_IO -3           /* scene / texture file could not be read */
#define TB_E_PARSE -4        /* scene parse error (std::runtime_error in the reference parser) */
#define TB_E_DEVICE -5       /* HIP runtime error */
#define TB_E_UNSUPPORTED -6  /* feature the reference also rejects (HANDLE_FAILURE paths) */
#define TB_E_NO_SCENE -7

typedef struct tb_context tb_context;

/* TracerBoy::Camera, TracerBoy.h:59-67 */
typedef struct tb_camera {
    float Position[3], LookAt[3], Right[3], Up[3];
    float LensHeight, FocalDistance;
} tb_camera;

/* TracerBoy::OutputSettings flattened (TracerBoy.h:212-288); only members that reach
 * PerFrameConstants (TracerBoy.cpp:2808-2851) are carried.  Defaults: TracerBoy.h:290-360. */
typedef struct tb_output_settings {
    uint32_t OutputType;              /* m_OutputType -> OutputMode (TB_OUTPUT_TYPE_*)        */
    uint32_t EnableNormalMaps;        /* m_EnableNormalMaps                                   */
    uint32_t RenderModeRealTime;      /* m_renderMode == RealTime -> IsRealTime               */
    float DebugValue, DebugValue2;    /* m_debugSettings                                      */
    float DOFFocalDistance, ApertureWidth; uint32_t FilterType; float FilterWidth; /* m_cameraSettings */
    float FireflyClampValue, MaxZ;    /* m_denoiserSettings                                   */
    float ConvergencePercentage;      /* m_performanceSettings... -> MinConvergence; takes effect with option "adaptive" (skip converged pixels) */
    uint32_t EnableNextEventEstimation, EnableSamplingImportanceResampling, EnableBlueNoise;
    int32_t MaxBounces;
    int32_t SampleTarget;
} tb_output_settings;

/* TracerBoy::PostProcessSettings (TracerBoy.h:222-245) + DebugSettings::m_VarianceMultiplier; defaults TracerBoy.h:298,309-313 */
typedef struct tb_post_settings {
    float ExposureMultiplier;         /* m_ExposureMultiplier, default 1                         */
    uint32_t EnableGammaCorrection;   /* m_bEnableGammaCorrection, default on                     */
    uint32_t EnableAutoExposure;      /* m_bEnableAutoExposure, default on                        */
    uint32_t TonemapType;             /* m_TonemapType (TB_TONEMAP_*), default AGX punchy          */
    float VarianceMultiplier;         /* m_debugSettings.m_VarianceMultiplier, default 1          */
} tb_post_settings;

/* TracerBoy::DenoiserSettings (TracerBoy.h:252-262), defaults TracerBoy.h:338-344 */
typedef struct tb_denoiser_settings {
    uint32_t Enabled;                               /* m_bEnabled, default on                         */
    float IntersectPositionWeightingMultiplier;     /* m_intersectPositionWeightingMultiplier, 1     */
    float NormalWeightingExponential;               /* m_normalWeightingExponential, 128             */
    float LuminanceWeightingMultiplier;             /* m_luminanceWeightingMultiplier, 4             */
    uint32_t WaveletIterations;                     /* m_waveletIterations, 5                        */
} tb_denoiser_settings;

/* TracerBoy::ReadbackStats (TracerBoy.h:362-368) + the heatmap counters summed over the render */
typedef struct tb_readback_stats {
    uint32_t ActiveWaves, ActivePixels;
    float SelectedPixelDistance;
    int32_t SelectedMaterialID;
    TbRayStats rays; /* zero unless tb_set_option("count_rays", 1) */
} tb_readback_stats;

typedef struct tb_scene_info {
    uint32_t numTriangles, numVertices, numMaterials, numLights, numGeometries, numTextures;
    uint32_t bvhBytesA, bvhNodesB, bvhMaxDepth;
    uint32_t filmWidth, filmHeight;
    float sceneMin[3], sceneMax[3];
} tb_scene_info;

/* AOV selectors for tb_read_aov (registers u2..u7 of SharedRaytracing.h:13-20) */
#define TB_AOV_NORMALS 2
#define TB_AOV_WORLD_POSITION0 3
#define TB_AOV_WORLD_POSITION1 4
#define TB_AOV_CUSTOM 5
#define TB_AOV_DEPTH 6
#define TB_AOV_EMISSIVE 7

/* <-> TracerBoy::TracerBoy(ID3D12CommandQueue*)  (TracerBoy.cpp:507-960).  device_id = HIP ordinal. */
int tb_create(tb_context** out, int device_id);
/* One context driving several devices of this process (SURVEY 8b "one context per process may drive N GPUs"; the reference's
 * TracerBoy object owns one D3D12 device).  The returned context is device_ids[0]'s and owns the frame: tb_load_scene builds once and
 * uploads to every device, tb_render deals the frame's 64x64 tiles round-robin over the devices, gathers the others' tiles with
 * peer-to-peer copies (xGMI) and un-permutes them into this context's accumulation surfaces, so tb_read_accum / tb_post_process /
 * tb_accum_device_ptr see the whole frame.  Options, camera, materials and history resets apply to all devices.  Not gathered: AOV
 * targets, the real-time chain, ray counters (TB_E_UNSUPPORTED / the owner's share).  The same id may be listed more than once. */
int tb_create_multi(tb_context** out, const int* device_ids, int n_devices);
int tb_group_size(tb_context* ctx); /* devices behind this context: 1 for tb_create */
void tb_destroy(tb_context* ctx);
const char* tb_last_error(tb_context* ctx); /* ctx may be NULL: error of a failed tb_create */

/* <-> TracerBoy::LoadScene (TracerBoy.cpp:1065-2161), blocking: parse, convert, build BVH, upload. */
int tb_load_scene(tb_context* ctx, const char* pbrt_path);
/* Deterministic procedural stand-ins for the scenes the reference tree lacks:
 * kind 0 = "dragon-class" displaced closed surface + ground (all matte, white environment),
 * kind 1 = "van-class" matte + mirror + glass + plastic mix, kind 2 = "bistro-class" (>=32 materials). */
int tb_load_procedural(tb_context* ctx, int kind, uint32_t target_triangles, uint32_t seed);
int tb_scene_info_get(tb_context* ctx, tb_scene_info* out);

/* <-> TracerBoy::GetDefaultOutputSettings (TracerBoy.h:290-360) */
void tb_default_output_settings(tb_output_settings* out);
/* <-> m_camera / TracerBoy::Update (camera part, TracerBoy.cpp:3386-3500); set invalidates history */
int tb_get_camera(tb_context* ctx, tb_camera* out);
int tb_set_camera(tb_context* ctx, const tb_camera* cam);
/* <-> TracerBoy::GetMaterial / SetMaterial / IsMaterialIDValid */
int tb_get_material(tb_context* ctx, int id, TbMaterial* out);
int tb_set_material(tb_context* ctx, int id, const TbMaterial* in);
int tb_material_count(tb_context* ctx);

/* <-> TracerBoy::Render x n_frames (TracerBoy.cpp:2677-2946): frames GlobalFrameCount =
 * samples_rendered .. +n_frames-1 are traced and accumulated into the context's accumulation
 * buffers.  time_seed <-> PerFrameConstants.Time (the reference uses wall-clock milliseconds,
 * TracerBoy.cpp:2817; callers pass 0 for reproducible output).  A change of width/height or of a
 * history-relevant setting restarts accumulation like UpdateOutputSettings (TracerBoy.cpp:2163-2185).
 * Synchronous: returns after the GPU has finished. */
int tb_render(tb_context* ctx, uint32_t width, uint32_t height, uint32_t n_frames,
              const tb_output_settings* settings, float time_seed);
/* Same, but returns after enqueueing on the context's stream; pair with tb_sync. */
int tb_render_async(tb_context* ctx, uint32_t width, uint32_t height, uint32_t n_frames,
                    const tb_output_settings* settings, float time_seed);
int tb_sync(tb_context* ctx);

/* <-> OutputTexture u0 / JitteredOutputTexture u1 (sum rgb*w, sum w), W*H*4 floats each, row 0 = top */
int tb_read_accum(tb_context* ctx, float* rgba_sum, float* jittered_or_null);
int tb_read_aov(tb_context* ctx, int which, void* dst);
/* device pointers of the accumulation buffers (for zero-copy consumers, e.g. an RCCL gather) */
int tb_accum_device_ptr(tb_context* ctx, void** output, void** jittered);
/* ---- output stage ---------------------------------------------------------------
 * <-> the tail of TracerBoy::Render (TracerBoy.cpp:2948-3030, 3165-3200): luminance histogram + averaged luminance when
 * auto exposure is on (GenerateHistogramCS.hlsl, CalculateAveragedLuminanceCS.hlsl), then PostProcessCS.hlsl on the
 * surface GetOutputSRV(output_type) selects (TracerBoy.cpp:2354-2383): the accumulated output for LIT / LUMINANCE, the
 * AOVs for ALBEDO / HEATMAP / LIVE_PIXELS / NORMAL / DEPTH (render with option "aov").  Writes the post-processed RGBA32F
 * image and/or the R8G8B8A8_UNORM back-buffer value (either pointer may be NULL), W*H pixels, row 0 = top.
 * Output types that need surfaces of the real-time chain (motion vectors, variance, live waves) return
 * TB_E_UNSUPPORTED. */
void tb_default_post_settings(tb_post_settings* out);
int tb_post_process(tb_context* ctx, const tb_post_settings* post, uint32_t output_type, float* rgba_f32_or_null, uint8_t* rgba8_or_null);
/* averaged luminance of the last auto-exposed tb_post_process (AveragedLuminance buffer) */
int tb_read_averaged_luminance(tb_context* ctx, float* out);
/* Image files for the headless CLI (the reference presents to a swap chain): ".png" (8-bit RGBA, stored deflate blocks),
 * ".pfm" (RGB float, bottom-up per the format) or ".exr" (OpenEXR scan lines, four uncompressed FLOAT channels) chosen by
 * extension; host-only, no context needed. */
int tb_write_image_rgba8(const char* path, uint32_t width, uint32_t height, const uint8_t* rgba8);
int tb_write_image_f32(const char* path, uint32_t width, uint32_t height, const float* rgba);
/* The texture decoders of tb_load_scene on their own (<-> DirectX::LoadFromHDRFile / LoadFromTGAFile / LoadFromWICFile +
 * the typed load of the resulting DXGI format, TracerBoy.cpp:2188-2232): .hdr .pfm .png .tga -> RGBA32F, row 0 = top.
 * rgba may be NULL to query the size; normalized <-> IsNormalizedFormat, has_alpha <-> !IsAlphaAllOpaque. */
int tb_decode_image(const char* path, uint32_t* width, uint32_t* height, int* normalized, int* has_alpha, float* rgba_or_null);

/* ---- real-time chain ------------------------------------------------------------
 * <-> TracerBoy::Render with RenderMode::RealTime (TracerBoy.cpp:2677-3160), one displayed frame per call: one sample per
 * pixel with IsRealTime (per-frame output, albedo demodulated into the custom AOV), TemporalAccumulationCS on the indirect
 * lighting with luminance moments, DenoiserCS x WaveletIterations, CompositeAlbedoCS, TemporalAccumulationCS again.  History
 * buffers and the previous camera live in the context.  tb_post_process(LIT) afterwards tonemaps the chain's output.
 * tb_read_realtime stages: 0 first TAA output (rgb, variance), 1 moments, 2 denoised, 3 composited, 4 final TAA output. */
void tb_default_denoiser_settings(tb_denoiser_settings* out);
int tb_render_realtime(tb_context* ctx, uint32_t width, uint32_t height, const tb_output_settings* settings, const tb_denoiser_settings* denoiser,
    float time_seed);
int tb_read_realtime(tb_context* ctx, int stage, float* rgba);

/* ---- denoised stills ---------------------------------------------------------
 * The reference denoises a still with OIDN on DirectML (the neural section below); here the progressive render's own two surfaces
 * feed the real-time chain's a-trous filter.  The jittered surface holds an independent half of every pixel's samples (RayGenCommon.h:721-727),
 * so the difference of the two halves' mean luminances estimates the variance of the mean's luminance.  The chain, all IEEE fp32:
 *   prepare    (sum rgb / sum w, that variance; 0 where a half is empty or the estimate is not finite)
 *   prefilter  3x3 Gaussian over the variance, coordinates clamped to the frame
 *   filter     WaveletIterations passes of DenoiserCS (OffsetMultiplier 1 << i) guided by the normals (TB_AOV_NORMALS) and the world positions
 *              of the last rendered frame L = tb_samples_rendered - 1 (TB_AOV_WORLD_POSITION0 + L % 2): render with option "aov", from the
 *              first frame on (setting the option resets the history)
 *   finish     (rgb, 1)
 * Pixels whose normal AOV is zero -- camera rays that missed, pixels the adaptive launch retired -- keep their mean and weigh nothing as a
 * neighbour's tap.  dn_or_null: NULL = tb_default_denoiser_settings; Enabled == 0 or WaveletIterations == 0: no filter pass, final is the mean
 * and no AOV is needed; more than 10 iterations: TB_E_INVALID.  rgba_or_null receives final (W*H*4 floats, row 0 = top).  Synchronous.
 * TB_E_INVALID (the message names the cause): nothing rendered; the last render was tb_render_realtime; filter passes asked for without the AOVs
 * of frame L (option "aov" off, or nothing rendered since tb_state_load / tb_state_begin: AOVs are not part of a state).  TB_E_UNSUPPORTED: a
 * context of a tb_create_multi group (AOVs are not gathered).
 * Writes neither the accumulation surfaces nor the AOVs, the frame counter or the history: tb_accum_digest is the same before and after, and a
 * render continued after the call is the uninterrupted render, bit for bit.  Whatever changes the accumulation surfaces (a render, tb_state_load,
 * tb_state_begin, a history reset) invalidates the denoised surfaces.
 * Option "post_denoised" = 1: tb_post_process(TB_OUTPUT_TYPE_LIT) and its auto exposure read final instead of the accumulated output
 * (TB_E_INVALID while no valid denoised surface exists); other output types ignore it.  tb_get_option "last_denoise_us": GPU microseconds of the
 * last chain, prepare to finish (HIP events).
 * tb_read_denoise_stage: 0 prepared, 1 filtered (both rgb, variance), 2 the last filter pass's output (rgb, variance; unavailable when no pass
 * ran), 3 final. */
int tb_denoise(tb_context* ctx, const tb_denoiser_settings* dn_or_null, float* rgba_or_null);
int tb_read_denoise_stage(tb_context* ctx, int stage, float* rgba);

/* ---- the guide pass of a denoised still ---------------------------------------
 * Seeds depend on (x, y, frame) only, so the first hits of any frames can be traced again at any time -- after a render that ran with option "aov"
 * off, at full speed, or after tb_state_load / tb_state_begin.  tb_render_guides traces the first bounce of the frames [first_frame, first_frame +
 * n_frames) with the context's current size, settings, time seed and camera (those of the last tb_render, tb_state_load or tb_state_begin; any
 * frame range, inside the rendered one or not; 1 <= n_frames <= 256; every pixel, adaptive retirement is ignored) and replaces the three guide
 * surfaces, RGBA32F, W x H, fp32 sums acc = acc + v from 0 in frame order:
 *   0 albedo    (sum of e_f, frames)                   e_f = the frame's albedo AOV, or (1, 1, 1) where it is all zero (a miss, a light, a path
 *                                                      that ended before it stored one): a pixel half on a light blends towards "not demodulated"
 *   1 normal    (sum of the normal AOV over the frames that hit, their number)      a frame hits where its normal AOV is not all zero
 *   2 position  (sum of the world position over the frames that hit, sum of the distance to the neighbour's hit over them)
 * With n_frames = 1 these are the AOVs a render with option "aov" leaves of that frame (TB_AOV_CUSTOM with zeros as ones, TB_AOV_NORMALS,
 * TB_AOV_WORLD_POSITION0 + frame % 2).  Synchronous.  Writes nothing else: accumulation, AOVs, frame counter, history and tb_accum_digest are what
 * they were, and a render continued afterwards is the uninterrupted one, bit for bit.
 * TB_E_INVALID (the message names the cause): no scene; no size yet; the last render was tb_render_realtime; an OutputType whose custom AOV is not
 * the albedo (heat map, live pixels); n_frames out of range.  TB_E_UNSUPPORTED: a tb_create_multi group; a tile assignment with world > 1.
 * The guides stay valid while scene, camera, size, history-relevant settings, time seed and option "alpha_test" are those they were traced with:
 * whatever resets the history, a resize or a scene load invalidates them; further rendering, tb_state_load(TB_STATE_ADD) and a TB_STATE_REPLACE
 * that leaves all of those equal do not.  tb_read_guide reads surface `which` (0..2; W*H*4 floats, row 0 = top; TB_E_INVALID without valid
 * guides).  tb_get_option "last_guides_us": GPU microseconds of the last pass's kernel (HIP events).
 * "last_guides_stack_overflow": stack entries per lane that pass kept in global memory (0: the whole traversal stack in LDS).
 * Option "denoise_guides" (does not reset the history) selects what tb_denoise reads:
 *   0 (default)  section 12 as it stands, bit for bit
 *   1            the filter's normals = sum / hits (brought back to length 1 where hits > 1: a mean of unequal normals is shorter than 1 and the
 *                filter raises dot products to NormalWeightingExponential), (0, 0, 0) where no frame hit; positions = sum / hits, all four
 *                components.  No AOV is needed: neither option "aov" nor a frame rendered since a state was loaded.  With guides of the one frame
 *                tb_samples_rendered - 1 the result is mode 0's of a render with option "aov", bit for bit.
 *   2            mode 1, and the chain runs on demodulated colour: d = max(albedo.xyz / albedo.w, 0.01) per channel, prepare divides the mean and
 *                both halves' means by d (the variance is that of the demodulated luminance), finish multiplies by d.  tb_read_denoise_stage
 *                0-2 are in the demodulated domain, 3 is remodulated.
 * With 1 or 2 and no valid guides tb_denoise returns TB_E_INVALID and says to call tb_render_guides. */
#define TB_GUIDE_ALBEDO 0
#define TB_GUIDE_NORMAL 1
#define TB_GUIDE_POSITION 2
int tb_render_guides(tb_context* ctx, uint32_t first_frame, uint32_t n_frames);
int tb_read_guide(tb_context* ctx, int which, float* rgba);

/* ---- sample budgets (no reference counterpart: its only control is the frame-rate target) -------------------
 * budget[y * width + x] is the global frame index at which pixel (x, y) stops receiving samples.  The context keeps a device copy; NULL clears it,
 * and without a budget every call is planned and launched as it always was, bit for bit.  Setting, changing or clearing a budget resets no
 * history, and a budget is not part of a render state.  While one is set, a tb_render / tb_render_async of n frames that starts at frame
 * F0 = tb_samples_rendered is a per-call adaptive call (tb_plan_input::adaptive = 2, plan rules 8 / 7, the call from frame 0 included):
 *   pixel p receives ALL n samples of the call -- the samples a plain call adds, in frame order -- iff F0 < budget[p], and none otherwise;
 *   with options "adaptive" = 1 and "adaptive_test" = 1 and F0 > adaptive_min_frames the skip test must be false as well.
 * So a pixel's sums are, bit for bit, the plain render's at some call boundary; a budget is exact where the calls are cut at its values.  A budget
 * need not be monotone in time: raise a pixel's later and it resumes.  A budgeted call from frame 0 first clears both accumulation surfaces: a
 * pixel that was never sampled holds (0, 0, 0, 0) on both -- 0 / 0 = NaN in tb_post_process's float picture, 0 in its 8-bit one.  The AOVs of a
 * pixel that is not live in a call are those of a pixel the adaptive launch skips (normal (0, 0, 0, 1), custom (0, 0, 0, 1) or the LIVE_PIXELS
 * tint); tb_denoise passes such pixels through.  tb_render_realtime ignores the budget, as it ignores "adaptive".  A tile assignment with
 * world > 1 works: only owned pixels are listed.  tb_get_option: "budget_set"; "last_budgeted" (the last call was planned under a budget);
 * "last_adaptive" is 1 and "last_live_pixels" the pixels listed for such a call.
 * TB_E_INVALID (the message names the cause): tb_set_sample_budget with a zero size or more than 2^24 pixels, or while option "count_rays" is set
 * (and "count_rays" while a budget is set); tb_render with a budget whose size is not the render's, or with "adaptive" = 1 and "adaptive_test" = 0
 * (the per-frame test would need a budget test inside the kernels); tb_read_sample_budget without a budget.  TB_E_UNSUPPORTED: a tb_create_multi
 * group. */
int tb_set_sample_budget(tb_context* ctx, uint32_t width, uint32_t height, const uint32_t* budget_or_null);
int tb_read_sample_budget(tb_context* ctx, uint32_t* out);
/* The noise target: with F = tb_samples_rendered, every pixel that is still live (budget > F) stops -- budget = F -- iff F >= min_frames, it holds
 * samples (n = output.w > 0) and either its mean c = output.xyz / n is black (every channel <= 0) or m > 0, n - m > 0 (m = jittered.w) and
 * V < rel_error^2 (luma(c)^2 + 0.01), V being section 12's dual-buffer variance of the mean's luminance, prepared and 3x3-prefiltered from the current
 * sums into scratch of this call's own (tb_denoise's surfaces stay as valid or invalid as they were); IEEE fp32, NaN compares false (such a pixel
 * stays live).  Creates an all-0xffffffff budget if none is set.  stopped_or_null: the pixels stopped by this call; live_or_null: the pixels with
 * budget > F afterwards.  Synchronous.  Writes nothing but the budget: tb_accum_digest, frame counter, history and guides are unchanged.
 * A failure leaves no budget the caller did not set.  tb_get_option "last_budget_stop_us": GPU microseconds of the last call's three passes (HIP
 * events).  With a tile assignment (world > 1) the call judges the whole surface: pixels of other ranks' tiles hold zeros, never stop and count
 * as live unless the budget is 0 there (set it so), and along tile borders their zero variance enters the owned neighbours' prefiltered estimate,
 * which is then lower than a one-context render's -- such pixels may stop a call earlier.
 * TB_E_INVALID: rel_error negative or not finite; nothing rendered; the last render was tb_render_realtime; a budget of another size than the
 * rendered frame; more than 2^24 pixels; option "count_rays" where the call would create the budget.  TB_E_UNSUPPORTED: a tb_create_multi group.
 * tb_run_budget_stop: the kernel seam, like tb_run_denoise_pass -- host arrays of the two sums (width*height*4 floats each) and the budget (in and
 * out), temporary buffers, nothing of the context but its stream; `frame` stands for F. */
int tb_budget_stop_converged(tb_context* ctx, float rel_error, uint32_t min_frames, uint64_t* stopped_or_null, uint64_t* live_or_null);
int tb_run_budget_stop(tb_context* ctx, uint32_t width, uint32_t height, const float* output, const float* jittered, uint32_t* budget, float rel_error,
                       uint32_t min_frames, uint32_t frame, uint64_t* stopped_or_null, uint64_t* live_or_null);

/* <-> ReadbackStats copy (TracerBoy.cpp:2946, D3D12App.cpp:195-201) */
int tb_read_stats(tb_context* ctx, tb_readback_stats* out);
/* Wave-occupancy profile of the last counting render (option "count_rays"): 7 pairs (active lane-executions,
 * wave trips) for: BVH inner-node step, leaf step, closest-hit shading, shadow-ray slot, scatter, regeneration,
 * main-loop iteration.  occupancy of a phase = active / (64 * trips). */
int tb_read_wave_profile(tb_context* ctx, uint64_t* out14);
/* Counters of the split-role kernel (option "pipeline" = 4 rendered with option "split_profile" = 1; no reference counterpart, an
 * instrument like the one above).  Traversal waves: [0] inner-node steps, [1] lanes in them, [2] triangle steps, [3] lanes in them,
 * [4] ticket draws, [5] rays taken, [6] sleeps with nothing to walk, [7] wave cycles.  Shading waves: [8] rounds, [9] lanes in them,
 * [10] sleeps waiting for hits, [11] wave cycles, [12] rays queued, [13] samples finished.  [14] / [15] traversal / shading waves. */
int tb_read_split_profile(tb_context* ctx, uint64_t* out16);
/* <-> InvalidateHistory (TracerBoy.cpp:3569-3575) / GetNumberOfSamplesSinceLastInvalidate */
void tb_invalidate_history(tb_context* ctx);
uint32_t tb_samples_rendered(tb_context* ctx);
/* <-> TracerBoy::SelectPixel */
int tb_select_pixel(tb_context* ctx, uint32_t x, uint32_t y);

/* Multi-GPU tile split: the frame is cut into tile_w x tile_h tiles numbered row-major;
 * this context renders tile t iff t % world == rank.  Pixels of other tiles are left untouched.
 * With world == 1 (default) the whole frame is rendered. */
int tb_set_tile_assignment(tb_context* ctx, uint32_t rank, uint32_t world, uint32_t tile_w, uint32_t tile_h);
/* Compact per-rank buffer: the owned tiles' pixels in tile order (tile-major, then row-major inside
 * the tile), RGBA32F.  count = number of pixels written; buffer must hold tb_owned_pixels(). */
uint64_t tb_owned_pixels(tb_context* ctx, uint32_t width, uint32_t height);
int tb_pack_owned_device(tb_context* ctx, void* device_dst);   /* device-to-device pack on the context stream */
int tb_pack_owned_device_async(tb_context* ctx, void* device_dst);   /* same, returns after enqueueing (pair with tb_sync or order through tb_stream) */
/* The context's HIP stream (a hipStream_t), for callers that order their own device work against the library's without
 * blocking the host -- e.g. an RCCL gather of the packed tiles after tb_render_async + tb_pack_owned_device_async
 * (torch.cuda.ExternalStream(tb_stream(ctx)) on the Python side).  Owned by the context. */
void* tb_stream(tb_context* ctx);
/* Rank 0, device side: un-permute the gathered buffers (world x capacity_pixels RGBA32F, rank r's packed tiles at
 * r * capacity_pixels -- the layout one RCCL gather into a contiguous buffer gives) into the full W x H frame, both in HBM.
 * Enqueued on `stream` (a hipStream_t, e.g. the stream the gather was ordered on; NULL = the context stream); returns at once. */
int tb_unpack_gathered_device(tb_context* ctx, void* stream, const void* gathered, uint64_t capacity_pixels, uint32_t width, uint32_t height,
                              uint32_t world, uint32_t tile_w, uint32_t tile_h, void* full_frame);
int tb_unpack_gathered_host(uint32_t width, uint32_t height, uint32_t world, uint32_t tile_w, uint32_t tile_h,
                            const float* const* per_rank_packed, float* full_rgba);

/* ---- render states (no reference counterpart: the reference's accumulation dies with its process) ----------
 * A render state is what a progressive render IS: the two accumulation surfaces and the range [first_frame, next_frame) of the frames
 * whose samples they hold, together with everything a later process must agree on to go on with the same bits.  Seeds depend on
 * (x, y, frame) only, so a render that is saved, loaded into a new context and continued is bit-identical to the uninterrupted one; states
 * of adjacent frame ranges add up (TB_STATE_ADD) to the fp32 sum of the partial sums.  AOVs, the real-time history, ray counters and region
 * costs are not part of a state: none of them changes a bit of the picture.
 * File: TB_STATE_HEADER_BYTES of header ("TBSTATE1", tb_state_info, zeros), then the output surface, then the jittered one, each
 * width x height RGBA32F, row 0 = top.  The digests (include/tb_state.h) are taken on the device from the surfaces as they lie in HBM. */
#define TB_STATE_VERSION 1u
#define TB_STATE_HEADER_BYTES 256u
typedef struct tb_state_info {
    uint32_t version;                         /* TB_STATE_VERSION */
    uint32_t width, height;
    uint32_t first_frame, next_frame;         /* the surfaces hold the samples of frames [first_frame, next_frame) */
    float time_seed;                          /* as passed to tb_render */
    tb_output_settings settings;              /* the settings the surfaces were accumulated under */
    tb_camera camera;
    uint32_t tile_rank, tile_world, tile_w, tile_h; /* tb_set_tile_assignment; tile_world == 1: a complete frame */
    uint32_t alpha_test, adaptive, adaptive_test;   /* the options that change the result, with adaptive_min_frames below */
    int64_t adaptive_min_frames;
    uint64_t scene_digest;                    /* tb_scene_digest of the scene the frames were rendered of */
    uint64_t output_digest, jittered_digest;  /* tb_accum_digest at the time of the save */
} tb_state_info;
enum { TB_STATE_REPLACE = 0, TB_STATE_ADD = 1, TB_STATE_ANY_SCENE = 16 };
/* The context holds the empty state [first_frame, first_frame): surfaces sized and zeroed.  A following tb_render with the same size,
 * time seed and history-relevant settings renders frames first_frame, first_frame + 1, ...; whatever resets the history (a change of any
 * of those, tb_set_camera, tb_set_material, tb_invalidate_history, tb_set_tile_assignment, an option that resets it) returns to frame 0. */
int tb_state_begin(tb_context* ctx, uint32_t width, uint32_t height, const tb_output_settings* settings, float time_seed, uint32_t first_frame);
/* Waits for the context's stream like tb_read_accum.  Atomic: the file is written beside `path` and renamed.  Refused (TB_E_INVALID) when
 * nothing is rendered or the last render was tb_render_realtime. */
int tb_state_save(tb_context* ctx, const char* path);
/* flags: TB_STATE_REPLACE or TB_STATE_ADD, optionally | TB_STATE_ANY_SCENE (do not compare the scene digests).  A scene must be loaded.
 * REPLACE: the context adopts size, settings, time seed, camera (without a history reset) and frame range; the options alpha_test, adaptive,
 * adaptive_min_frames and adaptive_test must have the file's values.  A complete frame (tile_world == 1) loads into any context -- every device
 * of a tb_create_multi group receives it --, a rank's partial frame only into a context with the same tile assignment.
 * ADD: context += file, per float, on the device; size, history-relevant settings, time seed, camera (by bits), scene and completeness must be
 * equal and the frame ranges adjacent (the file's appends or prepends).  The result is the fp32 sum of the two partial sums, NOT the bits of
 * one straight render.
 * TB_E_IO: the file cannot be read; TB_E_PARSE: bad magic, version, sizes, length or digest; TB_E_INVALID: a mismatch (the message names it). */
int tb_state_load(tb_context* ctx, const char* path, uint32_t flags);
/* digests of the output / jittered surface, computed on the device from HBM (waits for the context's stream) */
int tb_accum_digest(tb_context* ctx, uint64_t out2[2]);
/* digest of the loaded scene: every array of TbSceneView, each prefixed by its length (layout-A BVH, hit groups, indices, vertices,
 * materials, texture data, lights, images + texels, environment map, config constants without the camera's lens height, top level) */
int tb_scene_digest(tb_context* ctx, uint64_t* out);
/* host only, no device, no context.  tb_state_info_read validates the header and the file's length; tb_state_read_host also returns the
 * surfaces (each width x height x 4 floats; either may be NULL) and checks them against the stored digests; tb_state_write_host computes
 * the surface digests itself (the two digest fields and the version of `in` are ignored). */
int tb_state_info_read(const char* path, tb_state_info* out, char* err, uint32_t err_len);
int tb_state_read_host(const char* path, tb_state_info* out, float* output, float* jittered, char* err, uint32_t err_len);
int tb_state_write_host(const char* path, const tb_state_info* in, const float* output, const float* jittered);
uint64_t tb_state_digest_host(const void* words, uint64_t n_words);

/* Tunables / instrumentation: "pipeline" (0 = lock-step-bounce persistent kernel [default, fastest measured],
 * 1 = streaming persistent kernel with a resumable BVH walk),
 * "count_rays" (0/1), "bvh_builder" (0 = LBVH, 1 = binned SAH + reinsertion passes, 2 = LBVH built on the GPU, 3 = LBVH + the fallback layer's
 * three treelet passes = the tree the reference's PREFER_FAST_TRACE build traverses, 4 = the same built on the GPU), "flatten_instances".
 * Builder 1: "reinsertion_passes" (-1 = the library's choice), "reinsertion_share" (percent of the subtrees a pass tries, largest first),
 * "presplit" (percent of extra references from cutting the triangles with the largest, emptiest boxes before the build; 0 = off, the default:
 * measured to raise box tests), "wave_tree" (-1 = the library's choice: on where reinsertion passes run, 0 = off, 1 = on: for a scene that will be LDS-resident the tree is then
 * optimised for what a 64-lane wave pays, host/wave_cost.h; every other scene's tree is untouched), "wave_tree_threads" (the workers of that
 * search: 0 = min(16, the CPUs the process may run on), 1 = serial; the tree is the same bytes for every count).  Launch policy: "frame_group", "guided_groups" (0 never, 1 = calls that wait [default], 2 always: the frame
 * groups of a region shrink over the last groups of a launch), "primary_prepass", "overlap_launches", "costly_first" (+ "costly_late_samples"), "high_occupancy", "stack_lds_cap",
 * "compact_hits", "camera_constants", "texture_use_hint", "node_layout", "node_order" -- each described where launch_plan.h / context_render.cpp use it.
 * Adaptive sampling: "adaptive" (0/1), "adaptive_min_frames", "adaptive_test" (0 = the skip test runs before every frame
 * [default], 1 = once per call, at its first frame: a live pixel gets all the call's frames, a converged one none; any other value is refused).
 * An unknown name is an error. */
int tb_set_option(tb_context* ctx, const char* name, int64_t value);
/* tb_get_option also reads what the last render did ("last_*") and "debug_live_device_bytes": the device bytes the library holds for all
 * contexts of the process together (a context that is destroyed gives back all it took).  Render states: "state_first_frame" (the first
 * frame the surfaces hold; tb_samples_rendered is the one after the last), "last_state_digest_us" / "last_state_add_us" (GPU microseconds of
 * the last surface digest / TB_STATE_ADD sum, HIP events). */
int64_t tb_get_option(tb_context* ctx, const char* name);

/* The launch policy of tb_render as a pure function (no device, no context): which pipeline, which copy of the feature set (and how
 * much of the traversal stack stays in LDS), compact nodes, the primary-visibility pre-pass (off / on / tried both ways), whether
 * consecutive launches overlap, and the batch and frame-group sizes -- from statistics of the scene, the size of the call and the
 * options.  tb_render fills the input from its context and executes the plan; tests walk every branch on the CPU
 * (tests/test_launch_plan.py).  No reference counterpart: TracerBoy::Render has one shader and one dispatch shape (TracerBoy.cpp:2677-2946). */
enum { TB_PLAN_FEAT_SSS = 8, TB_PLAN_FEAT_EXT = 32 }; /* bits of variant_features the policy looks at (PT_FEAT_SSS / PT_FEAT_EXT) */
enum { TB_PLAN_PREPASS_OFF = 0, TB_PLAN_PREPASS_ON = 1, TB_PLAN_PREPASS_TRIAL = 2 };
/* rule_pipeline */
enum { TB_PLAN_RULE_ONE_PIXEL_PER_LANE = 1, TB_PLAN_RULE_FRAME_GROUPS, TB_PLAN_RULE_WAVEFRONT, TB_PLAN_RULE_POOLED, TB_PLAN_RULE_SPLIT,
    TB_PLAN_RULE_SPLIT_NO_ROOM, TB_PLAN_RULE_ADAPTIVE /* = 7: the adaptive launch (option "adaptive", frames past adaptive_min_frames) */,
    TB_PLAN_RULE_ADAPTIVE_GROUPS /* = 8: the adaptive launch tested per call (option "adaptive_test" = 1) through the frame-group kernels */,
       /* rule_copy */
       TB_PLAN_RULE_COPY_NONE = 10, TB_PLAN_RULE_COPY_FITS, TB_PLAN_RULE_COPY_SPLIT_STACK, TB_PLAN_RULE_COPY_TOO_DEEP, TB_PLAN_RULE_COPY_NO_ROOM,
           TB_PLAN_RULE_COPY_FULL_FOR_INSTANCES,
       TB_PLAN_RULE_PREPASS_NO_KERNEL = 20, TB_PLAN_RULE_PREPASS_OPTION_OFF, TB_PLAN_RULE_PREPASS_FORCED, TB_PLAN_RULE_PREPASS_SMALL_CALL,
           TB_PLAN_RULE_PREPASS_ENV_LIT,
       /* rule_prepass */
       TB_PLAN_RULE_PREPASS_GLASS_AMONG_OTHERS, TB_PLAN_RULE_PREPASS_TRIAL };
typedef struct tb_plan_input {
    /* the feature set the scene and the settings select (context.cpp kVariants) */
    uint32_t variant_features;        /* PT_FEAT_* mask of the set */
    uint32_t variant_waves_hi;        /* waves per SIMD of its higher-occupancy copy, 0 = it has none */
    uint32_t variant_prepass_in_base; /* its only copy carries the pre-pass (surf) */
    uint32_t variant_has_wavefront, variant_has_pooled, variant_has_split; /* pipelines 2 / 3 / 4 exist for it */
    uint32_t variant_stash_entries;   /* LDS entries per lane the higher-occupancy copy's frame-group kernels keep behind the stacks (scenes fetched from memory) */
    /* the loaded scene */
    uint32_t scene_in_lds, lds_blob_bytes, stack_depth, two_level, has_lights, has_compact_nodes;
    float interior_walk_triangle_share; /* share of the triangles whose material starts an interior walk */
    /* the call */
    uint32_t width, height, frames; int32_t max_bounces;
    uint64_t owned_regions;           /* 16x16 regions this context renders (the whole frame, or its tiles of a split) */
    uint32_t count_rays, aov, realtime, selected_pixel;
    /* options (tb_set_option), with their defaults where 0 is not one */
    int64_t pipeline, frame_group, high_occupancy /* 1 */, stack_lds_cap, stack_overflow_max /* 24 */, node_layout, primary_prepass /* 1 */,
            overlap_launches /* 1 */, pooled_samples /* 2^28 */;
    /* pipeline 4 (split-role kernel): its workgroup shape, so that the plan knows whether a workgroup's LDS and the frame's work items fit
     * and says "the lock-step kernel" itself where they do not (rule TB_PLAN_RULE_SPLIT_NO_ROOM) instead of leaving the launcher to refuse */
    int64_t split_trav /* 4 */, split_shade /* 0 = 4 with the scene in LDS, 6 otherwise */, split_stack_cap /* 0 = the whole stack in LDS */;
    /* frame groups that shrink towards the end of a launch (option guided_groups: 0 never, 1 = calls that wait for their result, 2 always) and
     * whether this call waits (tb_render, not tb_render_async) */
    int64_t guided_groups /* 1 */; uint32_t sync_call;
    /* the regions where paths were long in the launches before are handed out first (option costly_first: 0 never, 1 = feature sets with interior walks, calls
     * below 3 x 2^24 samples [default], 2 = those feature sets at any size) */
    uint32_t costly_first /* 1 */;
    /* 1: the call runs the adaptive launch: option "adaptive" on, not real-time, and its last frame past option adaptive_min_frames (renderImpl).
     * 2: the same tested once per call (option "adaptive_test" = 1; the call's FIRST frame is past adaptive_min_frames): the pixels live at the
     * call's first frame get every frame of the call, through the frame-group kernels where a plain call would take them (rule
     * TB_PLAN_RULE_ADAPTIVE_GROUPS), else through the one-pixel-per-lane adaptive kernel with its per-frame test switched off (TB_PLAN_RULE_ADAPTIVE) */
    uint32_t adaptive;
} tb_plan_input;
typedef struct tb_launch_plan {
    int32_t pipeline;                 /* 0 lock-step, 1 streaming, 2 wavefront, 3 pooled, 4 split-role: what will run */
    uint32_t groups;                  /* frame-group mode (resident grid, ordered sample buffer) */
    uint32_t high_occupancy_copy, full_variant;
    uint32_t stack_lds_entries, stack_overflow_entries; /* split stack when the second is not 0 */
    uint32_t compact_nodes;
    uint32_t prepass;                 /* TB_PLAN_PREPASS_* */
    uint32_t overlap_launches;
    uint32_t batch_frames, frame_group; /* frame-group mode only */
    uint32_t rule_pipeline, rule_copy, rule_prepass; /* TB_PLAN_RULE_*: which branch decided */
    uint32_t guided_groups;           /* frame-group mode: the groups of a region halve in size towards the end of a launch (frame_group = the largest) */
    uint32_t costly_first;            /* frame-group mode: the launch hands its regions out in the order of TbDeviceTargets::regionOrder (pt_scene.h) */
} tb_launch_plan;
void tb_plan_defaults(tb_plan_input* in);  /* zeroes, then the option defaults */
/* waves per SIMD the higher-occupancy copy of a feature set ("matte", "env", "surf", "vol", "full", "sss") is compiled for -- what
 * renderImpl puts into tb_plan_input::variant_waves_hi; 0 = the set has no such copy, -1 = no such set.  Needs no context. */
int tb_variant_waves_hi(const char* variant_name);
/* waves per SIMD of the feature set's copy for scenes in LDS (frame-group launches with the whole stack in LDS, where that many workgroups per CU fit;
 * option last_copy_waves tells which copy a launch ran); 0 = the set has no such copy, -1 = no such set.  Needs no context. */
int tb_variant_waves_lds(const char* variant_name);
/* LDS entries per lane (1 KB per workgroup each) the frame-group kernels of that copy keep behind the traversal stacks for a path's cold state --
 * tb_plan_input::variant_stash_entries; 0 = none, -1 = no such set */
int tb_variant_stash_entries(const char* variant_name);
int tb_plan_launch(const tb_plan_input* in, tb_launch_plan* out);
/* The frame groups of a region in a frame-group launch of `frames` frames whose (largest) group holds frame_group frames (a power of two): returns
 * their number; with group < that number also the group's first frame and its frame count.  guided = 0: equal groups; 1: the sizes halve towards
 * the end of the launch (tb_launch_plan::guided_groups; pt_scene.h tb_fg_groups -- the same function the kernels run).  Needs no context. */
uint32_t tb_frame_groups(uint32_t frames, uint32_t frame_group, uint32_t guided, uint32_t group, uint32_t* first_frame, uint32_t* num_frames);

/* The kernel seam, exported so the checker can run on exactly the arrays the kernels read:
 * fills `view` with HOST pointers owned by the context (valid until the next load/destroy). */
int tb_host_scene_view(tb_context* ctx, TbSceneView* view);
/* PerFrameConstants the next tb_render would push for frame `frame` (TracerBoy.cpp:2808-2851). */
int tb_make_frame_constants(tb_context* ctx, uint32_t width, uint32_t height, uint32_t frame,
                            const tb_output_settings* settings, float time_seed, TbPerFrameConstants* out);
/* Last timed render: GPU milliseconds measured with HIP events on the context's stream. */
float tb_last_render_ms(tb_context* ctx);
/* Closest-hit query through the device BVH (IntersectWithMaxDistance, RayGenCommon.h:365-414): n rays,
 * host arrays; out_t = -1 on miss. Used by the parity tests of the traversal kernel. */
int tb_trace_closest(tb_context* ctx, uint32_t n, const float* origins, const float* dirs, float* out_t,
                     int32_t* out_material, float* out_bary, uint32_t* out_prim, uint32_t* out_geom,
                     float* out_normal, float* out_uv, uint32_t* out_boxes, uint32_t* out_tris);
/* Device-side evaluation of tb_math.h (fn codes as oracle tbo_math) for host/device bit-equality tests. */
int tb_device_math(tb_context* ctx, int fn, uint32_t n, const float* a, const float* b, float* out);
/* The three kernels of the real-time chain (rt_kernels.hip) on host surfaces of ResolutionX * ResolutionY * 4 floats (width * height * 4 for
 * the composite), arguments as the oracle's tbo_temporal / tbo_denoise / tbo_composite: uploaded into temporary buffers, launched on the
 * context's stream, waited for and copied back.  Need no scene; read and write nothing the context holds (no history, no ping-pong state, no
 * accumulation, no denoised surface).  moment_history and out_moment may be null unless OutputMomentInformation is set.
 * TB_E_INVALID (the message names the cause): a required array is null; a dimension is 0; more than 2^24 pixels; OffsetMultiplier 0;
 * OutputMomentInformation set and one of the moment arrays null. */
int tb_run_temporal(tb_context* ctx, const TbTemporalConstants* constants, const float* history, const float* current, const float* world_pos,
                    const float* prev_world_pos, const float* moment_history, const float* normals, float* out, float* out_moment);
int tb_run_denoise_pass(tb_context* ctx, const TbDenoiserConstants* constants, const float* input, const float* normals, const float* positions,
                        const float* undenoised, float* out);
int tb_run_composite(tb_context* ctx, uint32_t width, uint32_t height, const float* albedo, const float* lighting, const float* emissive, float* out);

/* ---- FSR 1 upscaling -----------------------------------------------------------
 * <-> the reference's display path below full size: m_downscaleFactor < 1 or PostProcessSettings::m_bEnableFSR shrink the render surfaces,
 * GetSelectedUpscaler picks TAAUpscaler::FSR (TracerBoy.cpp:2520-2567) and the tail of Render runs FidelityFXSuperResolutionPass::Run
 * (TracerBoy.cpp:3324-3336; FidelityFXSuperResolution.cpp:53-111): EASU on the post-processed image, then RCAS at 0.2 stops.
 * Surface types (tb_abi.h): TB_FSR_SURFACE_UNORM8 -- input, intermediate and output are R8G8B8A8_UNORM as in the reference, so the picture
 * is quantised between the passes; TB_FSR_SURFACE_F32 -- RGBA32F throughout, alpha 1, no clamp (values outside [0, 1] and non-finite values go
 * through the same arithmetic).  All arithmetic is the fp32 contract of tb_math.h; tests/fsr_ref.py restates it in numpy.
 *
 * tb_fsr_constants: host only, no context.  easu = FsrEasuCon(in, in, out) (ffx_fsr1.h:156-202; all sixteen words, although the kernel reads
 * the first four only), rcas = FsrRcasCon(sharpness_stops) (:662-672): rcas[0] = bits of exp2(-stops) by tb_math.h's exp2, rcas[1] = that value
 * twice as truncated binary16.  TB_E_INVALID: a null pointer, a zero size, sharpness_stops not finite.
 * tb_run_fsr_easu / tb_run_fsr_rcas: the kernel seam, like tb_run_denoise_pass: host surfaces (4 B or 16 B per texel by surface type, row 0 =
 * top), temporary device buffers, no scene, nothing the context holds is read or written.  EASU: in is in_w x in_h, out is out_w x out_h.
 * RCAS: both w x h.
 * tb_upscale: the stage.  Runs exactly what tb_post_process(post, output_type) runs at the rendered size (option "post_denoised" included;
 * after tb_render as well as after tb_render_realtime), then EASU -> RCAS to out_w x out_h: the UNORM8 chain on the 8-bit back-buffer value
 * into rgba8_or_null (out_w * out_h * 4 bytes) when that is given, the F32 chain on the float image into rgba_f32_or_null (out_w * out_h * 4
 * floats) when that is given, both when both are.  sharpness_stops < 0: the reference's 0.2.  Synchronous.  Like tb_denoise it writes neither
 * the accumulation surfaces nor the AOVs, frame counter, history or denoised surfaces: tb_accum_digest is the same before and after.  Its
 * scratch surfaces belong to the context.  tb_get_option "last_upscale_us" / "last_easu_us" / "last_rcas_us": GPU microseconds of the last call's
 * FSR passes together / its EASU passes / its RCAS passes (HIP events; both chains when both ran).
 * TB_E_INVALID (the message names the cause): a null required pointer or a zero size; out_w < in_w or out_h < in_h (FSR 1 only upscales; 1:1
 * is allowed, as the reference allows it with m_bEnableFSR); more than 2^24 output pixels; an unknown surface type; sharpness_stops not finite;
 * both output pointers null; whatever tb_post_process itself refuses. */
int tb_fsr_constants(uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h, float sharpness_stops, TbFsrConstants* out);
int tb_run_fsr_easu(tb_context* ctx, const TbFsrConstants* constants, uint32_t surface, uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h,
                    const void* in, void* out);
int tb_run_fsr_rcas(tb_context* ctx, const TbFsrConstants* constants, uint32_t surface, uint32_t w, uint32_t h, const void* in, void* out);
int tb_upscale(tb_context* ctx, const tb_post_settings* post, uint32_t output_type, uint32_t out_w, uint32_t out_h, float sharpness_stops,
               float* rgba_f32_or_null, uint8_t* rgba8_or_null);

/* ---- the path inspector --------------------------------------------------------
 * <-> the reference's ray visualiser: TracerBoy::SelectPixel arms a buffer of MAX_VISUALIZER_RAYS rays, the path tracer appends the selected
 * pixel's bounce rays to it (RayGenCommon.h:600-630, kernel.glsl:1337-1351) and VisualizeRaysCS.hlsl draws them over the post-processed picture
 * (m_bVisualizeRays, TracerBoy.cpp:3201-3244).  Here nothing is recorded while rendering: a sample's seed depends on (x, y, frame) alone, so
 * tb_record_paths traces the complete paths of pixel (x, y) again for the frames [first_frame, first_frame + n_frames), 1 <= n_frames <= 4096,
 * with the context's current size, settings, time seed, camera and option "alpha_test" (what tb_render_guides uses; any frame range, rendered or
 * not; adaptive retirement and budgets are ignored).  Synchronous.  It writes nothing of the context but the ray buffer: tb_accum_digest, AOVs,
 * guides, frame counter and history are what they were.
 *   The ray buffer (tb_abi.h TbVisualizerRay; a count and up to TB_MAX_VISUALIZER_RAYS records): the closest-hit ray of every bounce i > 0 that
 *   the throughput early-out (kernel.glsl:1319-1326) did not end first -- origin, direction, HitT (the hit distance, -1 for a miss), BounceCount =
 *   (float)i.  The primary ray, feelers and interior-walk steps are not recorded.  Order: frame ascending, then bounce ascending, whatever the
 *   scheduling.  Calls append; when the buffer is full further rays are dropped and the count stays at the cap (the reference's counter runs on
 *   past the end).  rays_total_or_null: the rays this call would have stored without the cap.  tb_clear_paths empties the buffer, and so does
 *   whatever resets the history (tb_set_camera, a scene load, a resize, a change of history-relevant settings or time seed ...; the reference clears
 *   on a camera move, TracerBoy.cpp:2771).  tb_read_paths: the count, and min(capacity, count) records where rays_or_null is given.
 *   frames_or_null: n_frames records (TbPathFrame) for the caller, not kept.  sum: exactly what the render adds to the output surface for that
 *   sample -- colour after the firefly clamp times the filter weight, then the weight; zeros where the NaN filter rejected it (TB_PATH_REJECTED).
 *   TB_PATH_JITTERED: it also went to the jittered surface.  first_ray: where the frame's rays begin in the buffer, 0xffffffff when none was stored;
 *   num_rays: the rays its path produced; TB_PATH_TRUNCATED: the buffer held fewer of them.  Summed in frame order from frame 0 in fp32
 *   (acc = sum + acc) the records give the output surface's pixel, the flagged ones the jittered surface's, bit for bit.
 * TB_E_INVALID (the message names the cause): no scene; no size yet; the last render was tb_render_realtime; n_frames out of range; a pixel
 * outside the frame.  TB_E_UNSUPPORTED: a tb_create_multi group; a tile assignment with world > 1; a traversal stack that does not fit LDS.
 *
 * tb_visualize_rays: the overlay.  Needs a tb_post_process result in the context (TB_E_INVALID otherwise) and draws the stored rays over its float
 * picture into surfaces of its own -- the post output is not modified, a second call does not draw twice; the 8-bit picture is the output stage's
 * R8G8B8A8_UNORM store of the float one.  Settings (tb_default_visualize_settings: TracerBoy.h:303-306): RayWidth 0.01 the cylinders' radius,
 * RayDepth 10 -- rays of a bounce above it are skipped, the last one below it is drawn at the fraction RayDepth - bounce of its length --, RayCount 0
 * = all (the first RayCount rays of the buffer otherwise).  A ray is hidden where the pixel's world position (any |xyz| > 0.0001) is nearer.  That
 * position comes from TB_AOV_WORLD_POSITION0 + L % 2 of the last frame L where the render had option "aov", else from the guide pass's mean
 * (position sum / frames that hit, where any hit) while the guides are valid, else there is none and every ray draws on top; tb_get_option
 * "visualize_depth_source" says which applied to the last call: 1, 2 or 0.  Per pixel: VisualizeRaysCS.hlsl:133-226 in IEEE fp32, unfused, dot =
 * (x x' + y y') + z z', normalize = v / sqrt(dot), lerp = a + s (b - a); the reference's divisions by zero are kept (tests/visualize_ref.py is the
 * numpy restatement).  TB_E_UNSUPPORTED: a group, a tile assignment with world > 1.
 * tb_visualize_constants: host only, no context: VisualizationRaysConstants as TracerBoy.cpp:3216-3228 fills them (RayCount 0 -> 999999).
 * tb_run_visualize_rays: the kernel seam, like tb_run_fsr_easu: host arrays (rays: n_rays <= TB_MAX_VISUALIZER_RAYS records; scene_rgba, out_rgba and
 * world_pos_or_null: ResolutionX * ResolutionY * 4 floats, row 0 = top, of the position .xyz is read), temporary buffers, nothing of the context.
 * tb_get_option "last_paths_us" / "last_visualize_us": GPU microseconds of the last tb_record_paths / tb_visualize_rays (HIP events). */
typedef struct tb_visualize_settings { float RayWidth, RayDepth; int32_t RayCount; } tb_visualize_settings;
void tb_default_visualize_settings(tb_visualize_settings* out);
int tb_record_paths(tb_context* ctx, uint32_t x, uint32_t y, uint32_t first_frame, uint32_t n_frames, TbPathFrame* frames_or_null, uint32_t* rays_total_or_null);
int tb_clear_paths(tb_context* ctx);
int tb_read_paths(tb_context* ctx, TbVisualizerRay* rays_or_null, uint32_t capacity, uint32_t* count);
int tb_visualize_rays(tb_context* ctx, const tb_visualize_settings* settings_or_null, float* rgba_f32_or_null, uint8_t* rgba8_or_null);
int tb_visualize_constants(const tb_camera* camera, uint32_t width, uint32_t height, const tb_visualize_settings* settings_or_null, TbVisualizeConstants* out);
int tb_run_visualize_rays(tb_context* ctx, const TbVisualizeConstants* constants, const TbVisualizerRay* rays, uint32_t n_rays, const float* scene_rgba,
                          const float* world_pos_or_null, float* out_rgba);

/* ---- ray queries -----------------------------------------------------------------
 * The traversal the renderer uses, as a service: n rays in (tb_abi.h TbQueryRay), closest-hit records (TbQueryHit[n], TB_RAYS_CLOSEST) or
 * occlusion flags (uint8_t[n], 1 or 0, TB_RAYS_OCCLUDED) out.  Synchronous: runs on the context's stream and returns after the stream has
 * finished.  Without TB_RAYS_DEVICE both arrays are host arrays, staged in temporary device buffers like tb_trace_closest's; with it they are
 * device pointers of the context's device (rays and hit records 16-B aligned; the caller orders its own work on them before the call), and the
 * call allocates nothing -- the context keeps one small buffer, the work counter of the any-hit walk's refilling form, until tb_destroy.
 *   What a ray means.  MIN_T = 0.001 and MAX_T = 999999 are the renderer's constants.  A candidate counts iff MIN_T < t < min(TMax, MAX_T); TMax
 *   = +inf, or any value >= MAX_T, is the renderer's ray; a TMax that is a NaN or <= MIN_T gives a miss.  There is no per-ray tmin: move the
 *   origin instead.  A ray with TB_QUERY_RAY_DISABLED in Flags (only bit 0 is read) is not traced and reads as a miss / not occluded.  Option
 *   "alpha_test" applies as it does to tb_trace_closest on the same context.
 *   TB_RAYS_CLOSEST: the closest-hit walk of tb_trace_closest, unchanged; the hit is kept iff t < TMax (the closest hit inside the range exists
 *   iff the overall closest hit lies inside it), so every field has tb_trace_closest's bits.  A miss: T = -1, U = V = 0, Prim = Geom = 0xffffffff,
 *   Material = -1, UV = 0, Normal = 0.
 *   TB_RAYS_OCCLUDED: 1 iff some triangle passes the renderer's triangle test with its closest distance held at min(TMax, MAX_T).  One-level
 *   scenes run an any-hit walk that ends a ray at its first accepted candidate -- one ray per lane, or from 32 768 triangles a persistent grid
 *   whose waves refill their idle lanes; which triangle is found, and how rays are scheduled, does not change the answer.  Two-level scenes (option "flatten_instances" = 0) are answered by the closest-hit walk and the comparison t < TMax.
 * TB_E_NO_SCENE: no scene loaded.  TB_E_INVALID: a null pointer with n > 0; an unknown mode or flag bit; n > 2^31; a misaligned device pointer,
 * or one that is not memory of the context's device or is too short; a peer handle.  TB_E_UNSUPPORTED: the context of a tb_create_multi group.
 * n = 0: TB_OK, nothing is launched.  tb_trace_closest stays as it is. */
#define TB_RAYS_CLOSEST  0u
#define TB_RAYS_OCCLUDED 1u
#define TB_RAYS_DEVICE   0x100u       /* rays and out are device pointers of the context's device */
int tb_trace_rays(tb_context* ctx, uint32_t mode_and_flags, uint64_t n, const TbQueryRay* rays, void* out);

/* ---- radiance queries ------------------------------------------------------------
 * The path tracer on the caller's rays: the light arriving along n rays (tb_abi.h TbRadianceRay), num_samples paths each, summed per ray.
 * Synchronous like tb_trace_rays, on host arrays (staged, nothing kept) or, with TB_RADIANCE_DEVICE, on device pointers of the context's device
 * (16-B aligned; the context keeps one work counter and, on trees deeper than the LDS share, the overflow half of the stacks).
 *   Sample k of ray i has the number s = first_sample + k and starts with the seed hash13(SeedX, SeedY, (float)s) + seed_advance, the sum taken
 *   the way rand() moves a seed: floor(seed_advance) fp32 additions of 1 (at most 1024 of them), then one addition of the rest (a negative
 *   advance: one addition of all of it).  hash13 carries bits below the ulp of the sum, so the steps are not the one addition, and only the steps
 *   land where the renderer lands: for a camera ray of pixel (x, y) that is the seed of frame s once path_begin has drawn its pixel jitter
 *   (tb_make_camera_rays reports that distance).  The path starts at Origin along Direction with throughput 1, radiance 0, bounce 0, and runs the renderer's loop -- closest hit,
 *   shading, next-event estimation, the feeler, scattering, the interior walk, Russian roulette -- under the frame constants of `settings`
 *   (null: the defaults), `time`, the scene's lights and the current camera; MaxBounces 0 ends it at once.  AOVs, the heatmap, pixel picking and
 *   the real-time mode are not part of a query (RenderModeRealTime: TB_E_UNSUPPORTED).  Option "alpha_test" applies.
 *   A sample's result is the path's radiance, min(., FireflyClampValue) where that is >= EPSILON; a result with a NaN is rejected.
 *   out[i] = (sum r, sum g, sum b, number of accepted samples), summed in fp32 in sample order from 0 -- from out[i] as it stands with
 *   TB_RADIANCE_ACCUMULATE, so a call over [a, c) equals the calls over [a, b) and [b, c) accumulated, bit for bit.
 *   TB_RADIANCE_HEMISPHERE: Direction is a unit surface normal; every sample first draws two random numbers r0, r1 and starts along
 *   GenerateCosineWeightedDirection(normal, r0, r1) (kernel.glsl:1025-1046), its seed two further.  pi * sum / count is the irradiance; the library
 *   does not multiply.
 *   A ray whose direction is all zero or not finite, or whose origin is not finite, is not traced: out[i] is zeros, or stays under accumulate.
 * tb_make_camera_rays: the renderer's camera rays of frame `frame` for the pixels [x0, x1) x [y0, y1) of a W x H picture, row-major in the window:
 * origin and direction as path_begin leaves them (pixel jitter, depth of field), SeedX = x, SeedY = y.  *seed_advance_out: how far path_begin
 * moved the seed (16 without blue noise, 0 with it).  flags: 0 or TB_RADIANCE_DEVICE (out is a device pointer).  A filter whose weight is not 1
 * (triangle, Gaussian) is TB_E_UNSUPPORTED: the record has no weight.  So tb_trace_radiance(samples 1, first_sample f, that advance) on the rays of
 * frame f adds to out what tb_render adds to the accumulation surface in frame f.
 * TB_E_NO_SCENE: no scene.  TB_E_INVALID: a null pointer with n > 0; an unknown mode or flag bit; num_samples 0 or above 2^24; n > 2^31;
 * first_sample + num_samples past 2^32; a seed_advance that is not finite; an empty or outside window; a misaligned or foreign device pointer; a peer handle.  TB_E_UNSUPPORTED:
 * a tb_create_multi group; real-time settings; a stack deeper than LDS.  n = 0: TB_OK, nothing is launched.
 * tb_get_option "last_radiance_us" (GPU microseconds of the last query's launches), "last_radiance_variant" (the feature set's id, as
 * "last_variant"), "last_radiance_form" (0 one ray per lane, 1 the refilling grid). */
#define TB_RADIANCE_RAY        0u
#define TB_RADIANCE_HEMISPHERE 1u
#define TB_RADIANCE_DEVICE     0x100u   /* rays and out are device pointers of the context's device (the value and meaning of TB_RAYS_DEVICE) */
#define TB_RADIANCE_ACCUMULATE 0x200u   /* the sums start from out[i] */
int tb_trace_radiance(tb_context* ctx, const tb_output_settings* settings_or_null, float time, const TbRadianceCall* call, uint64_t n,
                      const TbRadianceRay* rays, TbFloat4* out);
/* host only, no context: why tb_trace_radiance refuses these arguments before it looks at its context -- TB_OK, or TB_E_INVALID with the reason in
 * why (why_bytes of room; may be null) */
int tb_radiance_refusal(const TbRadianceCall* call, uint64_t n, const void* rays, const void* out, char* why_or_null, uint32_t why_bytes);
int tb_make_camera_rays(tb_context* ctx, const tb_output_settings* settings_or_null, float time, uint32_t width, uint32_t height,
                        uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t frame, uint32_t flags, TbRadianceRay* out, float* seed_advance_out);

/* ---- lightmap baking -----------------------------------------------------------
 * One call from lightmap UVs to an RGBA32F atlas, all of it on the device: the triangles of a one-level scene are rasterised into a width x height
 * atlas by their lightmap UVs (texel (x, y) has its centre at u * width = x + 0.5, v * height = y + 0.5; row 0 is v = 0; no wrap), every texel that
 * a triangle owns becomes a ray record of the radiance query -- origin on the triangle, direction the interpolated unit normal, seed (x, y) --, the
 * atlas in row-major order is traced by tb_trace_radiance's kernels in TB_RADIANCE_HEMISPHERE mode with seed_advance 0 over the samples
 * [first_sample, first_sample + num_samples), and the sums are resolved (rgb = PI * sum / accepted count, alpha 1; texels without a triangle
 * (0, 0, 0, 0)) and dilated: dilate_passes times every texel with alpha 0 that has a 3 x 3 neighbour with alpha > 0 becomes the mean of those
 * neighbours, with alpha 2^-pass (1/2 in the first pass, 1/4 in the second ...), so a reader can tell rasterised texels from filled ones.
 * kernels/bake_launch.h states every rule operation by operation; tests/bake_cases.py restates them in numpy, and the two agree on bits.
 *   A texel whose centre a triangle covers (class 0) belongs to the lowest-numbered such triangle; a texel whose square a triangle only touches
 *   (class 1, the conservative half-texel offset) belongs to the lowest-numbered such triangle unless some triangle covers its centre; there its
 *   ray starts at the point of the triangle nearest to the centre in barycentric terms (negative weights clamped to 0, the rest renormalised).
 *   The origin is not offset along the normal: MIN_T keeps a path off the surface it starts on.
 *   Triangles are numbered as tb_host_scene_triangles numbers them (the scene's geometries back to back), vertices as section 21 numbers them.
 * uv_or_null: 2 floats per vertex of the scene; null: the UV field of the scene's vertex records as loaded -- loads flip V (FlipTextureUVs), so a
 * file's (u, v) arrives as (u, 1 - v).  rgba_out: width x height x 4 floats, row 0 first.  Positions and normals are what the last
 * tb_commit_geometry left.  Synchronous.  The context keeps the atlas's rays, texel records and sums until the next bake, a scene load or a
 * rebuild (tb_read_bake); they are allocated at the first bake, reused while the size holds, and freed with the scene.
 * flags: TB_BAKE_DEVICE -- uv_or_null and rgba_out are device pointers of the context's device, uv 4-B and rgba_out 16-B aligned.
 * TB_BAKE_ACCUMULATE -- nothing is rasterised (uv_or_null is not read): the samples are added to the sums the last bake of the same size left,
 * which are then resolved and dilated again; by section 22's contract bakes of 3 and then 5 samples equal one of 8, bit for bit.  Refused
 * (TB_E_INVALID) when no bake of that size is held or a tb_commit_geometry has changed the scene since it was rasterised.
 * Refusals, in this order, each leaving the last bake as it was: tb_bake_refusal's (TB_E_INVALID: a null call, a side of 0 or above 8192, unknown
 * flag bits, num_samples 0 or above 2^24, first_sample + num_samples above 2^32, more than 16 passes, a null rgba_out, misaligned device
 * pointers); TB_E_NO_SCENE; TB_E_UNSUPPORTED for a tb_create_multi group, a two-level scene (section 21 refuses vertex access there for the same
 * reason) and real-time settings; pointers that are not memory of the context's device; TB_BAKE_ACCUMULATE's two.
 * tb_get_option: "last_bake_raster_us", "last_bake_trace_us", "last_bake_finish_us" (GPU microseconds of the rasteriser, the query and resolve +
 * dilate; HIP events), "last_bake_covered" (texels with a triangle).
 * tb_read_bake: what the last bake rasterised and summed, each width x height records in row-major order, to the host pointers that are not null.
 * tb_run_bake_raster / tb_run_bake_dilate: the kernel seam, like tb_run_fsr_easu: host arrays, temporary device buffers, no scene -- the
 * rasteriser on n_vertices positions, normals (3 floats each) and uvs (2 floats each) and n_triangles x 3 vertex numbers (one at or past
 * n_vertices is TB_E_INVALID); `passes` fill passes on a width x height RGBA32F picture. */
#define TB_BAKE_DEVICE     0x100u   /* the value and meaning of TB_RAYS_DEVICE */
#define TB_BAKE_ACCUMULATE 0x200u
typedef struct tb_bake_call { uint32_t width, height, first_sample, num_samples, dilate_passes, flags; } tb_bake_call;
int tb_bake_lightmap(tb_context* ctx, const tb_output_settings* settings_or_null, float time, const tb_bake_call* call, const float* uv_or_null,
                     float* rgba_out);
/* host only, no context: why tb_bake_lightmap refuses these arguments before it looks at its context -- TB_OK, or TB_E_INVALID with the reason in why */
int tb_bake_refusal(const tb_bake_call* call, const void* uv_or_null, const void* rgba_out, char* why_or_null, uint32_t why_bytes);
int tb_read_bake(tb_context* ctx, TbRadianceRay* rays_or_null, TbBakeTexel* texels_or_null, float* sums_or_null);
int tb_run_bake_raster(tb_context* ctx, uint32_t width, uint32_t height, uint32_t n_vertices, const float* positions, const float* normals,
                       const float* uvs, uint32_t n_triangles, const uint32_t* tri_vertex_index, TbRadianceRay* rays_out, TbBakeTexel* texels_out);
int tb_run_bake_dilate(tb_context* ctx, uint32_t width, uint32_t height, uint32_t passes, const float* rgba_in, float* rgba_out);

/* ---- light probes ---------------------------------------------------------------
 * The other half of a baker: lightmaps light the static surfaces, probes light what moves between them.  tb_bake_probes takes n positions and
 * returns n TbProbe records (tb_abi.h), all of it on the device: every probe looks along the texel centres of a resolution x resolution octahedral
 * map (2 .. 64; the directions are fixed, samples vary the paths), each direction is a ray of the radiance query -- ray mode, seed_advance 0, seed
 * (first_probe_number + i, texel), the samples [first_sample, first_sample + num_samples) -- and a ray of tb_trace_rays in TB_RAYS_CLOSEST mode
 * with TMax +inf; the mean radiance per direction, weighted by the texel's solid angle, is projected onto the nine real SH basis functions of
 * orders 0 to 2 and normalised by the sum of the weights, so a constant radiance L gives SH[0] = 2 sqrt(pi) L whatever the resolution; the hits
 * give the statistics a sampler needs to leave out probes inside geometry.  kernels/probe_launch.h states every rule operation by operation;
 * tests/probe_cases.py restates them in numpy, and the two agree on bits.  A probe with a coordinate that is not finite is not traced: its record
 * is zeros with both distances -1.  One-level and two-level scenes.  Synchronous.
 * positions_xyz: 3 floats per probe; probes_out: n records.  flags: TB_PROBES_DEVICE -- both are device pointers of the context's device,
 * positions 4-B and probes_out 16-B aligned.  TB_PROBES_KEEP_MAPS -- the context keeps every ray's sums and hit record for tb_read_probe_maps
 * (64 B a ray); without it it keeps the records and the buffers of one batch.  TB_PROBES_ACCUMULATE -- the samples are added to the sums the last
 * bake kept: bakes of 3 and then 5 samples equal one of 8, bit for bit.  It needs a bake held with its maps, of the same n and resolution, traced
 * of the scene as it is now (no load, rebuild or tb_commit_geometry since): else TB_E_INVALID; the maps stay kept.
 * A bake runs in batches of whole probes of at most TB_PROBE_MAX_RAYS rays (environment, read at every call; default 2^20, that is 128 MB for
 * the four per-ray buffers); the split does not change a byte of the answer.  The buffers are made at the first bake and released with the scene.
 * Refusals, in this order, each leaving the last bake as it was: tb_probes_refusal's (TB_E_INVALID: a null call; a resolution outside [2, 64];
 * n x resolution^2 above 2^31; n, or first_probe_number + n, above 2^24 -- the seed must be an exact float; num_samples 0 or above 2^24;
 * first_sample + num_samples above 2^32; unknown flag bits; with n > 0 a null pointer or a misaligned device pointer); TB_E_NO_SCENE;
 * TB_E_UNSUPPORTED for a tb_create_multi group and real-time settings; n = 0: TB_OK, nothing is launched; pointers that are not memory of the
 * context's device; TB_PROBES_ACCUMULATE's three.
 * tb_get_option: "last_probes_rays_us", "last_probes_trace_us", "last_probes_hits_us", "last_probes_project_us" (GPU microseconds of the four
 * stages, summed over the batches; HIP events), "last_probes_batches", "probes_held" (the probes of the bake held; 0: none), "probes_resolution",
 * "probes_maps_held".
 * tb_read_probe_maps: what the last bake with TB_PROBES_KEEP_MAPS summed and hit, n x resolution^2 records each in probe-major order (4 floats;
 * TbQueryHit), to the host pointers that are not null.
 * tb_sample_probes: the consumer's half.  n points with unit normals against a grid of probes (tb_abi.h tb_probe_grid; probes in the grid's
 * numbering, count[0] x count[1] x count[2] <= 2^24 of them): trilinear weights over the eight probes around the point (clamped to the grid), a
 * probe counting iff its Weight > 0 and its Backfaces <= backface_limit x resolution^2, the weights renormalised over those that count;
 * rgba_out[i] = (irradiance r, g, b at the normal, the sum of the counting weights) -- zeros where none counts.  flags: 0 (host arrays, staged)
 * or TB_PROBES_DEVICE (probes and rgba_out 16-B, points and normals 4-B aligned).  Needs no scene.
 * tb_sh9_irradiance (host, pure): the irradiance of one record at a unit normal, the sampler's own text.  tb_probe_directions (host, pure): the
 * M x M directions (3 floats each) and solid angles of a map, to the pointers that are not null; TB_E_INVALID for M outside [2, 64].
 * tb_run_probe_rays / tb_run_probe_project: the kernel seam, like tb_run_bake_raster: host arrays, temporary device buffers, no scene; at most
 * 2^24 rays. */
#define TB_PROBES_DEVICE     0x100u   /* the value and meaning of TB_RAYS_DEVICE */
#define TB_PROBES_ACCUMULATE 0x200u
#define TB_PROBES_KEEP_MAPS  0x400u
typedef struct tb_probe_call { uint32_t n, first_probe_number, resolution, first_sample, num_samples, flags; } tb_probe_call;
int tb_bake_probes(tb_context* ctx, const tb_output_settings* settings_or_null, float time, const tb_probe_call* call, const float* positions_xyz,
                   TbProbe* probes_out);
/* host only, no context: why tb_bake_probes refuses these arguments before it looks at its context -- TB_OK, or TB_E_INVALID with the reason in why */
int tb_probes_refusal(const tb_probe_call* call, const void* positions_xyz, const void* probes_out, char* why_or_null, uint32_t why_bytes);
int tb_read_probe_maps(tb_context* ctx, float* sums_or_null, TbQueryHit* hits_or_null);
int tb_sample_probes(tb_context* ctx, uint32_t flags, const tb_probe_grid* grid, uint32_t resolution, float backface_limit, const TbProbe* probes,
                     uint64_t n, const float* points_xyz, const float* normals_xyz, float* rgba_out);
int tb_sh9_irradiance(const TbProbe* probe, const float* normal_xyz, float* rgb_out);
int tb_probe_directions(uint32_t resolution, float* dirs_out_or_null, float* weights_out_or_null);
int tb_run_probe_rays(tb_context* ctx, uint32_t n, uint32_t resolution, uint32_t first_probe_number, const float* positions_xyz,
                      TbRadianceRay* radiance_rays_out, TbQueryRay* query_rays_out);
int tb_run_probe_project(tb_context* ctx, uint32_t n, uint32_t resolution, const float* positions_xyz, const float* sums, const TbQueryHit* hits,
                         TbProbe* probes_out);

/* ---- point queries (no reference counterpart) ---------------------------------------------------------------------
 * The tree as a service for POINTS: for each of n points (tb_abi.h TbQueryPoint) the nearest point of the scene's triangles, a TbNearest record.
 * include/tb_nearest.h states the rule operation by operation -- the nearest point of one triangle, which triangles count (Distance <=
 * MaxDistance), the tie-break (smaller Geom, then smaller Prim) and the pruning slack of the walk -- and host and device give the same bits; the
 * answer is a function of the triangle set and the point alone, whatever the tree.  Synchronous like tb_trace_rays, on host arrays (staged,
 * nothing kept) or, with TB_NEAREST_DEVICE, on device pointers of the context's device (16-B aligned; nothing is allocated).  The kernel is a
 * nearest-first walk of the layout-B tree in memory, one point per lane; layout C and LDS-resident scenes change nothing, option "alpha_test" does
 * not apply (the query is geometry alone), positions are what the last tb_commit_geometry left.  A position that is not finite is a miss.
 * TB_NEAREST_SIGNED: Distance is negated where the point lies behind the NEAREST TRIANGLE (dot(p - Point, face vector) < 0; the face vector is
 * tb_normals.h's).  That is exact where the nearest point is interior to a triangle; wrong for about one point in twenty near edges or vertices
 * whose faces meet at an acute angle, a regular tetrahedron included; see section 28 (tb_nearest_points_winding has the robust sign).
 * tb_bake_distance_field: the same walk over the cells of a grid (tb_abi.h tb_probe_grid: cell (i, j, k) at origin + (i, j, k) * spacing, one
 * rounded product and one rounded sum per axis, number (k * count[1] + j) * count[0] + i), positions made in the kernel and never stored; out is
 * one float per cell, the Distance of the cell's record (signed under the flag, +inf on a miss), every cell with MaxDistance = max_distance.
 * out is a host array or, with TB_NEAREST_DEVICE, a 4-B aligned device pointer.
 * Refusals, in this order: a peer handle (TB_E_INVALID); TB_E_UNSUPPORTED for a tb_create_multi group ("multi-device group"); tb_nearest_refusal's
 * (TB_E_INVALID: unknown flag bits; n > 2^31; a null pointer with n > 0; misaligned device pointers; a null grid, a count of 0, more than 2^31
 * cells, an origin or a spacing that is not finite); TB_E_NO_SCENE; TB_E_UNSUPPORTED for a two-level scene ("two-level": a transform with
 * non-uniform scale does not keep nearest points; load with option "flatten_instances" = 1); n = 0: TB_OK, nothing is launched; pointers that are
 * not memory of the context's device, or too short (TB_E_INVALID).
 * tb_get_option "last_nearest_us": GPU microseconds of the last query's kernel (HIP events).
 * tb_nearest_refusal (host only, pure, like tb_bake_refusal): grid_or_null = null judges a tb_nearest_points call, else a tb_bake_distance_field
 * call (n and points are not read).
 * tb_host_scene_nearest: the rule on the host, over a one-level host scene's layout-B arrays (TB_E_UNSUPPORTED for a two-level one).  flags:
 * TB_NEAREST_SIGNED and exactly one of TB_NEAREST_HOST_BRUTE -- every triangle, in order, through the header's rule -- and TB_NEAREST_HOST_WALK
 * -- the kernel's walk and pruning rule as scalar C++.  tb_host_scene_nearest_excess: the measurement behind TB_NEAREST_SLACK_ULPS
 * (scripts/nearest_slack.py): over the n points, the largest sqrt(tb_box_d2) - sqrt(D2) of a box above the brute-force winner's leaf (the root's
 * box included), in units of 2^-23 x tb_nearest_scale; 0 where every such box is nearer than its triangle. */
#define TB_NEAREST_SIGNED     0x1u
#define TB_NEAREST_DEVICE     0x100u    /* the value and meaning of TB_RAYS_DEVICE */
#define TB_NEAREST_HOST_BRUTE 0x1000u   /* tb_host_scene_nearest only */
#define TB_NEAREST_HOST_WALK  0x2000u   /* tb_host_scene_nearest only */
int tb_nearest_points(tb_context* ctx, uint32_t flags, uint64_t n, const TbQueryPoint* points, TbNearest* out);
int tb_bake_distance_field(tb_context* ctx, uint32_t flags, const tb_probe_grid* grid, float max_distance, float* out);
int tb_nearest_refusal(uint32_t flags, uint64_t n, const void* points, const void* out, const tb_probe_grid* grid_or_null, char* why_or_null,
                       uint32_t why_bytes);

/* ---- winding numbers (no reference counterpart) -------------------------------------------------------------------
 * Robust inside / outside: for each of n points (tb_abi.h TbQueryPoint; MaxDistance is not read) the generalized winding number of the scene's
 * triangles, w = (sum of the triangles' signed solid angles) / 4 pi, one float per point: 1 inside a closed mesh whose face vectors point outward,
 * 0 outside, -1 inside an inward-facing one, 2 inside two shells, and a graceful in-between on open meshes and soups.  include/tb_winding.h states
 * the rule operation by operation -- the solid angle of one triangle, the moments of a subtree, the far-field test L2 > (beta r)^2 under which a
 * subtree is replaced by its dipole, and the order of the sum -- and host and device give the same bits; w is a function of (tree topology,
 * triangles, point, beta).  beta >= 1; larger is more exact and slower, +inf sums every triangle (the exact form); 3 is the default of the Python
 * layer.  tb_winding_inside (tb_winding.h; api.winding_inside) is |w| >= 0.5.  A position that is not finite gives the NaN 0x7fc00000.
 * Synchronous like tb_nearest_points, on host arrays (staged, nothing kept) or, with TB_WINDING_DEVICE, on device pointers of the context's device
 * (points 16-B aligned, numbers 4-B).  The subtree moments (64 B per node) are made on the device at the first call of a scene and again at the
 * first call after a tb_commit_geometry; a rebuild or a new scene drops them; beyond them nothing is allocated per call on the device path.
 * tb_bake_winding_field: the same walk over the cells of a grid, tb_bake_distance_field's cell rule, one float per cell.
 * tb_nearest_points_winding, tb_bake_distance_field_winding: the UNSIGNED point query of section 27, unchanged, then a pass of the walk that sets
 * the sign bit of Distance where the record is a hit and tb_winding_inside(w): every byte is the unsigned answer's but that bit; a miss stays
 * +inf.  TB_NEAREST_SIGNED is refused here (TB_E_INVALID): the two signs are different rules.
 * TB_WINDING_HOST_WALK (tb_winding_numbers only, host arrays only): the kernel's walk as scalar C++ over the context's own host copies of the tree
 * as the device holds it now -- what the device must give on bits, whatever built or refitted the tree.
 * Refusals, in tb_nearest_points's order: a peer handle (TB_E_INVALID); TB_E_UNSUPPORTED for a tb_create_multi group ("multi-device group");
 * tb_winding_refusal's (TB_E_INVALID: unknown flag bits; n > 2^31; a null pointer with n > 0; misaligned device pointers; the grid's, as
 * tb_nearest_refusal's; a beta that is a NaN or < 1); TB_E_NO_SCENE; TB_E_UNSUPPORTED for a two-level scene ("two-level") and for a tree of pre-split
 * references ("pre-split": under option "presplit" a cut triangle lies in the tree once per reference, and a sum over the leaves would count it
 * as often -- the refit refuses the same trees; tb_host_scene_winding refuses them too); n = 0: TB_OK, nothing is launched; pointers that are not
 * memory of the context's device, or too short (TB_E_INVALID).
 * tb_get_option "last_winding_us": GPU microseconds of the last call's walk; "last_winding_fit_us": of the last moment fit (HIP events).
 * tb_winding_refusal (host only, pure): grid_or_null = null judges a tb_winding_numbers call, else a tb_bake_winding_field call.
 * tb_host_scene_winding: the rule on the host over a one-level host scene's layout-B arrays (TB_E_UNSUPPORTED for a two-level one and for a tree of
 * pre-split references).  flags: exactly
 * one of TB_WINDING_HOST_BRUTE -- every triangle of the array in order, the exact form; beta is checked, not used -- and TB_WINDING_HOST_WALK. */
#define TB_WINDING_DEVICE     0x100u    /* the value and meaning of TB_RAYS_DEVICE */
#define TB_WINDING_HOST_BRUTE 0x1000u   /* tb_host_scene_winding only */
#define TB_WINDING_HOST_WALK  0x2000u   /* tb_host_scene_winding and tb_winding_numbers */
int tb_winding_numbers(tb_context* ctx, uint32_t flags, uint64_t n, const TbQueryPoint* points, float beta, float* out);
int tb_bake_winding_field(tb_context* ctx, uint32_t flags, const tb_probe_grid* grid, float beta, float* out);
int tb_nearest_points_winding(tb_context* ctx, uint32_t flags, uint64_t n, const TbQueryPoint* points, float beta, TbNearest* out);
int tb_bake_distance_field_winding(tb_context* ctx, uint32_t flags, const tb_probe_grid* grid, float max_distance, float beta, float* out);
int tb_winding_refusal(uint32_t flags, uint64_t n, const void* points, const void* out, const tb_probe_grid* grid_or_null, float beta, char* why_or_null,
                       uint32_t why_bytes);

/* ---- dynamic scenes (no reference counterpart: its scene is frozen once LoadScene returns) -------------------------
 * Vertices and instance transforms are STAGED by the three calls below; nothing a render or a trace reads changes until tb_commit_geometry, which
 * waits for the context's stream and then applies everything staged.  A commit with nothing staged is TB_OK and does nothing.
 * Vertex numbering: that of the scene's position / vertex arrays, all geometries back to back; tb_scene_info::numVertices bounds it and
 * tb_geometry_vertex_range gives the range of one geometry (hit-group record).  Coordinates are in the space those arrays hold (world space for a
 * one-level scene).  xyz: n_vertices triples.  Without TB_UPDATE_DEVICE a host array: it is checked for finite values (TB_E_INVALID otherwise) and
 * copied before the call returns.  With it a device pointer of the context's device, read where it lies on the context's stream (tb_stream,
 * tb_sync) without a staging copy; its VALUES ARE NOT CHECKED -- a position that is not finite gives boxes no ray enters, that is misses, never an
 * access out of range, because the topology does not change.
 * tb_update_normals writes the Normal field of the 32-B vertex records (TbVertex); UVs and tangents stay.  Nothing is recomputed: the caller
 * brings the normals that go with its positions.
 * tb_commit_geometry(0), the refit: the tree keeps its topology -- every child reference, the sorted order of the triangles, their metadata -- and
 * every stored box becomes what the builder's fit pass gives for that topology and the new positions, bit for bit:
 *   leaf    mn = min(v0, v1, v2), mx = max(v0, v1, v2); mn = min(mn, mx - 0.001f); c = (mn + mx) * 0.5f, h = mx - c
 *   parent  from the children's STORED boxes: mn = min(lc - lh, rc - rh), mx = max(lc + lh, rc + rh), then the same c, h
 * so a refit from the positions a scene was loaded with gives back the loaded tree.  On the device it runs as one launch over the triangles and one
 * per level of a schedule made once; the only value the host reads is the 24-byte root box.  The compact nodes (option "node_layout") and the LDS
 * image of an LDS-resident scene are made again from the new tree.  The host copies (tb_host_scene_view, tb_scene_digest, tb_scene_info_get) are
 * brought up from the device when they are next asked for, not at the commit.
 * tb_commit_geometry(TB_GEOMETRY_REBUILD): the refit, then the tree a fresh load of the moved scene would build (option "bvh_builder"), slow; for
 * meshes that have deformed past what a refit tree serves well.  It also rebuilds, with nothing staged, a tree that has been refit.
 * tb_set_instance_transforms (two-level scenes: option "flatten_instances" = 0 with instances): object_to_world_3x4 holds n_instances row-major 3 x 4
 * matrices (host memory).  The commit derives worldToObject as the loader does and builds the top level again (same bytes as a load of the scene
 * with those transforms); the bottom levels are untouched.
 * After a commit that changed something: the history is reset (tb_samples_rendered is 0), tb_scene_digest differs -- a render state saved before
 * cannot be resumed onto the moved scene --, tb_scene_info's sceneMin / sceneMax follow.  The dynamic state (a device copy of the positions, per
 * triangle its vertex numbers, per node its parent, the level schedule) is made at the first of these calls and released with the scene; a context
 * that never calls them allocates and launches nothing for it.  tb_get_option "last_refit_us": GPU microseconds of the last refit's kernels.
 * Refusals; each leaves the scene and the staged data as they were (the message names the cause).  TB_E_NO_SCENE: no scene.  TB_E_INVALID: a range
 * past the end; a null pointer with n > 0; unknown flag bits; a host value that is not finite; a transform whose 3 x 3 part is singular or not finite.
 * TB_E_UNSUPPORTED: a tb_create_multi group (ranks that are separate processes each call the update themselves); tb_update_positions /
 * tb_update_normals on a two-level scene; tb_set_instance_transforms on a scene without instances; TB_GEOMETRY_REBUILD of a two-level scene; a tree
 * of pre-split references (option "presplit"); at the commit, staged vertices of a geometry whose material is emissive that differ from the scene's
 * (each emissive triangle has a TbLight that carries its positions, normals and area, and the light table is not made again): the message names the
 * geometry.  Not offered: adding or removing triangles, motion blur. */
#define TB_UPDATE_DEVICE    0x100u   /* xyz is a device pointer of the context's device (the value and meaning of TB_RAYS_DEVICE) */
#define TB_GEOMETRY_REBUILD 1u       /* tb_commit_geometry: build a new topology */
int tb_update_positions(tb_context* ctx, uint32_t flags, uint32_t first_vertex, uint32_t n_vertices, const float* xyz);
int tb_update_normals(tb_context* ctx, uint32_t flags, uint32_t first_vertex, uint32_t n_vertices, const float* xyz);
int tb_set_instance_transforms(tb_context* ctx, uint32_t first_instance, uint32_t n_instances, const float* object_to_world_3x4);
int tb_commit_geometry(tb_context* ctx, uint32_t flags);
int tb_geometry_vertex_range(tb_context* ctx, uint32_t geometry, uint32_t* first_vertex, uint32_t* n_vertices);

/* ---- scenes from caller arrays; smooth normals recomputed on the device (no reference counterpart) -----------------
 * tb_load_meshes: a scene from vertices and faces in memory instead of a .pbrt / .pbf file (tb_abi.h tb_mesh_desc, tb_scene_desc).  Every mesh becomes
 * one geometry (hit-group record) in the order given, its vertices numbered back to back -- section 21's numbering: tb_geometry_vertex_range(g) is
 * mesh g.  Positions, indices, the per-triangle arrays and the hit-group records come out of the functions the PBRT conversion uses, with positions,
 * normals and UVs stored as given.  A vertex record is Normal (given, flat or smooth), UV (given or 0) and Tangent (0, 0, 1).  A mesh whose material
 * carries TB_MAT_LIGHT gets one area TbLight per triangle (LightColor the material's emissive; N0..N2 the vertex records' normals where normals were
 * given or smooth, the loader's face normal in flat mode); the library sets no flag on the caller's behalf and makes no directional lights.  The scene
 * is one-level; materials are copied as given, FlipTextureUVs is 0, the environment (host memory, also under TB_MESH_DEVICE) gets the identity
 * transform and env_scale; without one the scene has none, as a file without one.  camera_or_null: taken as it stands; null: the procedural scenes'
 * look-at camera with eye = c + (0, 0.35 d, d), target c, 35 degrees, c the centre of the vertices' bounds and d twice their diagonal (1 where that
 * is 0).  Then the scene is built and uploaded as a loaded one is: every option a file load honours applies ("bvh_builder", "scene_in_lds",
 * "node_order" ...), and renders, queries, bakes, updates, render states and the scene digest work as on a loaded scene.
 * TB_MESH_DEVICE: positions, indices, normals and UVs of every mesh are device pointers of the context's device, checked as section 20 checks its
 * pointers (device memory, this device, long enough).  They are read to the host ONCE, by copies on the context's stream, and then pass the host
 * checks below: the tree build and every host consumer work from the host copy.  A build that never leaves the device is not offered.
 * Refusals, in this order, the message naming the mesh and the element where there is one; a refused call leaves the context's scene as it was.
 * tb_meshes_refusal's (TB_E_INVALID): a null desc; no meshes or no materials; a null positions or indices pointer; 0 vertices or 0 triangles; a
 * material index at or past n_materials; an unknown normals mode or flag bit; an environment with a side of 0 or above 16384; more than 2^24 - 1
 * triangles or 2^27 - 1 vertices in total, index bytes past 2^32.  TB_E_UNSUPPORTED: a tb_create_multi group; a material that names a texture.
 * TB_E_INVALID: under TB_MESH_DEVICE a pointer that is not memory of the context's device.  TB_E_INVALID: an index at or past its mesh's n_vertices;
 * a position, normal, UV or environment value that is not finite.
 * tb_host_scene_from_meshes: the host half (host arrays only; TB_MESH_DEVICE is TB_E_INVALID), for tb_host_scene_* and the oracle.
 * tb_host_smooth_normals: include/tb_normals.h's rule over one mesh, 3 floats per vertex into normals_out; a vertex that no triangle names keeps
 * what normals_out holds.  TB_E_INVALID: a null pointer, an index at or past n_vertices.
 * tb_recompute_normals: staged like tb_update_normals -- a MARK on the vertices first_vertex .. first_vertex + n_vertices.  The next
 * tb_commit_geometry makes their normals again by that rule, on the device, per mesh, from the positions as that commit leaves them, and writes them
 * into the Normal field of the vertex records; UVs and tangents stay.  A face vector is taken over all three of its vertices, marked or not.  Order
 * inside one commit: staged positions, the refit, staged explicit normals, marked ranges -- a recomputation wins over tb_update_normals for the same
 * vertex.  A commit with only marks staged counts as a change.  Vertices of a geometry whose material carries TB_MAT_LIGHT are skipped and stay as
 * they are (section 21 does not let them move, and their TbLights carry their normals), so a whole-scene call works on a scene with a light.
 * Refusals as for tb_update_normals: no scene, a range past the end, a group, a two-level scene, a pre-split tree; n_vertices 0 is TB_OK.  The
 * tables (per triangle its vertex numbers in geometry order, per vertex the face-vector slots of its corners) are made at the first call and
 * released with the scene; "last_refit_us" includes the two launches. */
int tb_load_meshes(tb_context* ctx, const tb_scene_desc* desc);
int tb_meshes_refusal(const tb_scene_desc* desc, char* why_or_null, uint32_t why_bytes);   /* host only, pure, like tb_bake_refusal */
int tb_host_smooth_normals(const float* positions, uint32_t n_vertices, const uint32_t* indices, uint32_t n_triangles, float* normals_out);
int tb_recompute_normals(tb_context* ctx, uint32_t first_vertex, uint32_t n_vertices);

/* ---- neural still denoiser -----------------------------------------------------
 * <-> the reference's TAAUpscaler::OIDN path (TracerBoy.cpp:3306-3322; OpenImageDenoise.cpp:855-1039): the OIDN U-Net -- 16 convolutions of 3 x 3,
 * four 2 x 2 max-pools on the way down, four nearest upsamples x 2 on the way up, each concatenated in front of the skip tensor of its size, ReLU
 * after every layer -- on the post-processed LDR picture, the mean albedo and the mean normals (9 input channels) or the picture alone (3).
 * The library ships no weights: the caller names a TZA file (OIDN's rt_ldr_alb_nrm.tza / rt_ldr.tza, or any file of that graph).
 * Layer arithmetic, the contract (tests/neural_ref.py restates it in torch): activations and weights are binary16; products are summed in fp32, in
 * any order; then + bias, then max(., 0) where the layer has ReLU, then one rounding to binary16 (nearest even; overflow gives infinity, NaN is
 * propagated).  Padding is zero; the max-pool takes the rounded values; the network runs on the picture zero-extended at the right and bottom to
 * multiples of 16 and its result is cropped.
 *
 * tb_nn_weights_info: host only, no context.  Reads the file's tensors `<layer>.weight` (oihw, 3 x 3) and `<layer>.bias` (x) for the layers
 * enc_conv0, enc_conv1, enc_conv2, enc_conv3, enc_conv4, enc_conv5a, enc_conv5b, dec_conv4a, dec_conv4b, dec_conv3a, dec_conv3b, dec_conv2a,
 * dec_conv2b, dec_conv1a, dec_conv1b, dec_conv0 (the order of out_channels / in_channels_of); binary32 tensors are rounded to binary16.  Channel
 * counts are the file's, each 1 ... 256, as long as the graph closes (3 or 9 inputs, 3 outputs).  weight_bytes: the binary16 bytes of all weights
 * and biases.  TB_E_IO: the file cannot be read.  TB_E_PARSE (err names the tensor and the cause): bad magic or version, anything that runs past
 * the end of the file, a missing tensor, a wrong layout or kernel size, a graph that does not close.
 * tb_neural_load: the same read, then the repack for the kernel and the upload; replaces weights loaded before.
 * tb_run_conv3x3: the layer seam, like tb_run_denoise_pass: host arrays of binary16 bits in unpadded NHWC order, temporary device buffers, no
 * scene, no loaded weights, nothing the context holds is read or written.  in_a is width x height x c_a -- (width / 2) x (height / 2) x c_a with
 * upsample_a, read nearest-upsampled -- in_b_or_null width x height x c_b, concatenated behind A; weight_oihw is c_out x (c_a + c_b) x 3 x 3, bias c_out;
 * out is height x width x c_out, (height / 2) x (width / 2) x c_out with pool.  TB_E_INVALID (the message names the cause): a null required
 * pointer, a zero size, an odd width or height with pool or upsample_a, more than 512 channels in a tensor, more than 2^24 pixels.
 * tb_run_neural: the network on host surfaces (width x height RGBA32F, .xyz read; out gets (r, g, b, 1)).  Needs tb_neural_load; albedo and
 * normal are given exactly when the weights have 9 inputs.  Bit for bit the chain of tb_run_conv3x3 calls on the packed input (channels colour,
 * albedo, normal).  Reads and writes nothing else the context holds.  At most 2^24 pixels after the extension to multiples of 16.
 * tb_denoise_neural: the stage. Colour is what the reference's network reads: the 8-bit picture tb_post_process(post, TB_OUTPUT_TYPE_LIT) writes at the
 * rendered size (option "post_denoised" included), each channel k / 255 in fp32 -- the reference's post-process surface has the back buffer's format,
 * R8G8B8A8_UNORM (TracerBoy.cpp:3817-3829, D3D12App.cpp:3), its view is OpenImageDenoise::Run's input (TracerBoy.cpp:3309-3318) and
 * ImageToTensorCS.hlsl:22-32 loads it as float3 -- so the colour is clamped to [0, 1], quantised, and a NaN of the float picture (the default AgX
 * punchy tonemapper gives one for a black pixel) goes in as 0.  The quantisation happens inside the pack (no extra pass, no 8-bit surface).  With
 * 9-input weights albedo is sum.xyz / sum.w of guide surface TB_GUIDE_ALBEDO and the normals are those option
 * "denoise_guides" = 1 gives the a-trous filter (the mean over the frames that hit, several brought to length 1, zero where nothing was hit), both of
 * valid guide surfaces (tb_render_guides), neither clamped. The float result goes to rgba_f32_or_null (width * height * 4 floats), its 8-bit conversion
 * as the output stage does it (clamp with NaN -> 0, scale, + 0.5, truncate) to rgba8_or_null. Synchronous. Like tb_denoise it writes neither the
 * accumulation surfaces nor AOVs, frame counter, history, guides or denoised surfaces: tb_accum_digest is the same before and after. Its activation
 * buffers belong to the context (sized at the first use, kept while the size holds, released by tb_destroy). TB_E_UNSUPPORTED: a tb_create_multi
 * group. TB_E_INVALID: no weights, nothing rendered, both pointers null, no valid guides with 9-input weights (call tb_render_guides), whatever
 * tb_post_process refuses. tb_run_neural takes its floats as they are: a non-finite value given there spreads over the network's receptive field
 * (about 95 pixels each way) and no further. tb_get_option "last_neural_us": GPU microseconds of the last network, pack to unpack (HIP events);
 * "neural_inputs": 0, 3 or 9.
 * tb_run_nn_pack / tb_run_nn_unpack / tb_run_nn_resolve_aux / tb_run_nn_to_rgba8: the four helper kernels around the layers, like tb_run_composite:
 * host arrays, temporary device buffers, no scene, no weights, nothing the context holds is read or written.  Surfaces are width x height RGBA32F,
 * row 0 = top; a tensor is padded_h x padded_w x 32 binary16 (as bits), padded sizes >= the picture's (the network uses the next multiples of 16).
 *   pack: channels 0-2 colour.xyz, and with albedo and normal (both or neither) 3-5 albedo.xyz, 6-8 normal.xyz, each rounded once to binary16 (nearest
 *     even); every other channel and every pixel outside width x height is zero.  unorm_color != 0: the colour first goes through the 8-bit store,
 *     k = (uint32)(saturate(x) * 255 + 0.5) with NaN -> 0, then (float)k / 255 -- the stage's form; 0 is tb_run_neural's.
 *   unpack: out = (channels 0-2 of the tensor at (y, x) as fp32, 1).
 *   resolve aux: albedo = (sum.xyz / sum.w, 1); normals = (sum.xyz / hits, 1) with hits = sum.w > 0, brought to length 1 when hits > 1 (zero when
 *     that length is 0), (0, 0, 0, 1) when hits is 0.
 *   to rgba8: (uint32)(saturate(x) * 255 + 0.5) per channel with NaN -> 0, alpha 255.
 *   TB_E_INVALID (the message names the cause): a null required array, albedo without normal or the reverse, a zero dimension, more than 2^24
 *   pixels (padded ones included), a padded size below the picture's. */
typedef struct tb_nn_info { uint32_t in_channels; uint32_t out_channels[16]; uint32_t in_channels_of[16]; uint64_t weight_bytes; } tb_nn_info;
typedef struct tb_conv3x3_desc { uint32_t width, height;      /* of the convolution's output before pooling */
                                 uint32_t c_a, c_b, c_out;    /* channels of source A, source B (0 = none), output */
                                 uint32_t upsample_a;         /* A is (width/2 x height/2), read nearest-upsampled */
                                 uint32_t pool, relu; } tb_conv3x3_desc;
int tb_nn_weights_info(const char* tza_path, tb_nn_info* out, char* err, uint32_t err_len);
int tb_neural_load(tb_context* ctx, const char* tza_path);
int tb_run_conv3x3(tb_context* ctx, const tb_conv3x3_desc* d, const uint16_t* in_a, const uint16_t* in_b_or_null,
                   const uint16_t* weight_oihw, const uint16_t* bias, uint16_t* out);
int tb_run_neural(tb_context* ctx, uint32_t width, uint32_t height, const float* color_rgba,
                  const float* albedo_rgba_or_null, const float* normal_rgba_or_null, float* out_rgba);
int tb_denoise_neural(tb_context* ctx, const tb_post_settings* post, float* rgba_f32_or_null, uint8_t* rgba8_or_null);
int tb_run_nn_pack(tb_context* ctx, uint32_t width, uint32_t height, uint32_t padded_w, uint32_t padded_h, uint32_t unorm_color, const float* color_rgba,
                   const float* albedo_rgba_or_null, const float* normal_rgba_or_null, uint16_t* out_tensor);
int tb_run_nn_unpack(tb_context* ctx, uint32_t width, uint32_t height, uint32_t padded_w, uint32_t padded_h, const uint16_t* tensor, float* out_rgba);
int tb_run_nn_resolve_aux(tb_context* ctx, uint32_t width, uint32_t height, const float* albedo_sum, const float* normal_sum, float* out_albedo,
                          float* out_normal);
int tb_run_nn_to_rgba8(tb_context* ctx, uint32_t width, uint32_t height, const float* rgba, uint8_t* out_rgba8);

/* ---- neural 2 x super-resolution ------------------------------------------------
 * <-> the reference's DirectMLSuperResolutionPass (DirectMLSuperResolution.cpp:304-409 the graph, :986-1091 the run, :1128-1219 the weights;
 * ImageToTensorCS.hlsl, TensorToImageCS.hlsl), what it upscales with when built with PREFER_OIDN 0 (pch.h:10-14, TracerBoy.cpp:3289-3303): the frame
 * is rendered at half size and the network gives the full-size picture.  Seven convolutions, zero padding (K - 1) / 2, stride 1:
 *   conv1 3 -> 32, 5 x 5; conv2 32 -> 64, 3 x 3; conv3 64 -> 64, 3 x 3, at width x height; nearest upsample x 2; conv_up1/conv 64 -> 32, 5 x 5;
 *   conv4 32 -> 32; conv5 32 -> 32; conv6 32 -> 3, all 3 x 3, at 2 width x 2 height; bias + ReLU after every layer but conv6, which has neither.
 * The result is |half(conv6 + the input nearest-upsampled x 2)| with alpha 1 (the abs: TensorToImageCS.hlsl:50).  The library ships no weights: the
 * caller names a file of the reference's container (TracerBoy/ML/weights.bin).  The layer arithmetic is the neural section's contract
 * (tests/sr_ref.py restates it in torch); the residual add is the exact sum of two binary16 values, rounded once.
 *
 * tb_sr_weights_info: host only, no context.  The container: int32 tensor count, then per tensor u32 name length (at most 255), the name, u32 element
 * count and that many binary32 values (DirectMLSuperResolution.cpp:94-160).  A layer's filter is `<name>/weights` (oihw), and every layer but conv6
 * has `<name>/BatchNorm/scale` and `/shift`.  The file holds no shapes: kernel[] is the graph's (5, 3, 3, 5, 3, 3, 3), out_channels the scale
 * tensor's length (3 for conv6), in_channels the filter's count / (out * K * K); each 1 ... 256, and the chain closes (3 in, 3 out, a layer reads what
 * its predecessor wrote).  weight_bytes: the binary16 bytes of all folded filters and biases.  TB_E_IO: the file cannot be read.  TB_E_PARSE (err
 * names the tensor and the cause): a negative count, a name longer than 255, anything that runs past the end of the file, a missing tensor, a count
 * that does not divide, a chain that does not close.
 * tb_sr_read_layer: host only.  The folded binary16 values of one layer (0 ... 6): filter * scale[o] as one fp32 multiply, then the reference's
 * Float16Compressor::compress (DirectMLSuperResolution.cpp:47-63), restated bit for bit -- it truncates where a rounding would round, and gives
 * infinity for everything above 65504; the bias is compress(shift[o]).  weight_oihw holds out * in * K * K values, bias_or_null out (untouched for
 * layer 6, which has none).
 * tb_sr_load: the same read, then the repack for the kernel and the upload; replaces weights loaded before.
 * tb_run_conv: the layer seam, like tb_run_conv3x3 (host arrays of binary16 bits in unpadded NHWC order, temporary device buffers, nothing the
 * context holds is read or written) with a kernel of 3 or 5 and an optional bias.  form: 0, the plain form, a wave per 16 pixels of a row with every
 * fragment from memory; 1, the staged form, a workgroup per 32 x 8 pixels with its input tile and halo in LDS; the results are the same bits.  The
 * staged form holds at most 64 input channels, each source padded to a multiple of 32.  TB_E_INVALID (the message names the cause): a null required
 * pointer, a zero size, an odd width or height with upsample_a, more than 512 channels in a tensor, more than 2^24 pixels, a kernel other than 3 or
 * 5, a form above 1, form 1 with more input channels than it holds.
 * tb_run_sr_finish: the residual add on host arrays: residual (2 in_h) x (2 in_w) x 3 and input in_h x in_w x 3, binary16 bits; out_rgba gets
 * (|half(residual + input at (y >> 1, x >> 1))|, 1) as fp32, (2 in_w) * (2 in_h) * 4 floats.
 * tb_run_sr: the network on a host surface (width x height RGBA32F, .xyz read as they are); out_rgba is 2 width x 2 height.  Needs tb_sr_load.
 * Bit for bit the pack, seven tb_run_conv calls and tb_run_sr_finish.  tb_set_option "sr_conv_form" (0 or 1; default 1, the staged form, which
 * takes half the time) picks the form of its convolutions; a layer with more input channels than the staged form holds runs in the plain form.
 * tb_upscale_neural: the stage.  The network's input is what the reference's reads: the 8-bit picture tb_post_process(post, TB_OUTPUT_TYPE_LIT)
 * writes at the rendered size (option "post_denoised" included), each channel k / 255 (the neural section argues the surface's format).  The float
 * result goes to rgba_f32_or_null (2 width * 2 height * 4 floats), its 8-bit conversion as the output stage does it to rgba8_or_null.  Synchronous.
 * It writes neither the accumulation surfaces nor anything another stage reads: tb_accum_digest is the same before and after.  Its weights and
 * activation buffers belong to the context (sized at the first use, kept while the size holds, released by tb_destroy).  TB_E_UNSUPPORTED: a
 * tb_create_multi group.  TB_E_INVALID: no weights, nothing rendered, both pointers null, more than 2^24 output pixels, whatever tb_post_process
 * refuses.  tb_get_option "last_sr_us": GPU microseconds of the last network, pack to finish (HIP events); "sr_loaded": 0 or 1; "sr_conv_form":
 * the form the network's convolutions run in. */
typedef struct tb_sr_info { uint32_t in_channels[7], out_channels[7], kernel[7]; uint64_t weight_bytes; } tb_sr_info;
typedef struct tb_conv_desc { uint32_t width, height;       /* of the convolution's output */
                              uint32_t c_a, c_b, c_out;     /* channels of source A, source B (0 = none), output */
                              uint32_t kernel;              /* 3 | 5 */
                              uint32_t upsample_a, relu;
                              uint32_t form;                /* 0 plain, 1 staged */ } tb_conv_desc;
int tb_sr_weights_info(const char* path, tb_sr_info* out, char* err, uint32_t err_len);
int tb_sr_read_layer(const char* path, uint32_t layer, uint16_t* weight_oihw, uint16_t* bias_or_null, char* err, uint32_t err_len);
int tb_sr_load(tb_context* ctx, const char* path);
int tb_run_conv(tb_context* ctx, const tb_conv_desc* d, const uint16_t* in_a, const uint16_t* in_b_or_null, const uint16_t* weight_oihw,
                const uint16_t* bias_or_null, uint16_t* out);
int tb_run_sr_finish(tb_context* ctx, uint32_t in_w, uint32_t in_h, const uint16_t* residual_2w2h3, const uint16_t* input_wh3, float* out_rgba);
int tb_run_sr(tb_context* ctx, uint32_t width, uint32_t height, const float* color_rgba, float* out_rgba);
int tb_upscale_neural(tb_context* ctx, const tb_post_settings* post, float* rgba_f32_or_null, uint8_t* rgba8_or_null);

/* ---- image-quality metrics (no reference counterpart: the definitions are the standard ones) -------------------
 * A test picture A against a reference picture R, both RGBA32F of one size w x h, row 0 = top.  RGB is compared, alpha is ignored (a NaN alpha
 * excludes nothing).  Where A is an accumulation surface, A.rgb = sum.rgb / sum.w, one fp32 division per channel, and a pixel with sum.w == 0 is
 * UNSAMPLED (outside a crop window, a zero budget).  A pixel is EXCLUDED if it is unsampled or one of its six RGB values is not finite: it is
 * counted and contributes to nothing.
 * Pointwise, in fp64 per included pixel and channel: d = (double)A - (double)R, se = d d, ae = |d|, re = se / ((double)R (double)R + rel_epsilon);
 * per pixel the three channels are added in the order r, g, b; mse, mae, rel_mse = the sums over the included pixels / (3 pixels); max_abs = the
 * largest ae; psnr = 10 log10(peak^2 / mse) on the host, +inf for mse == 0; pixels == 0: all of them NaN.  The squared-error map holds
 * (float)((se_r + se_g + se_b) / 3.0) per pixel, 0 at an excluded one.
 * SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03), in fp32 on x < 0 ? 0 : x > peak ? peak : x per channel, an
 * excluded pixel as 0; valid region only: (w - 10) x (h - 10) windows, none if w < 11 or h < 11.  The eleven weights are the binary32 values
 * 3a86cab6 3bf8ff01 3d13758c 3ddff87f 3e5a1e20 3e8832b0 and back.  A plane is filtered along rows, then along columns, each as acc = 0; acc = acc +
 * w[i] x[i] for i = 0..10 (separate multiply and add); five planes per channel: a, r, a a, r r, a r (fp32 products).  Per window
 * va = Eaa - ma ma, vr = Err - mr mr, c = Ear - ma mr, C1 = (float)((0.01 (double)peak)^2), C2 = (float)((0.03 (double)peak)^2),
 * s = (((2 ma) mr + C1) (2 c + C2)) / ((ma ma + mr mr + C1) (va + vr + C2)); the window's value is ((double)s_r + s_g + s_b) / 3.0; a window that
 * holds an excluded pixel is skipped and counted.  The map holds the value rounded to fp32, 0 for a skipped window; ssim is the fp64 mean over
 * the windows that count, NaN without one.  A == R bit for bit gives exactly 1 in every window.
 * Sums: every workgroup writes one partial record at its own index and a last kernel adds them in index order -- no floating-point atomic, so
 * for a given w x h the result is the same bits on every call; the order is not part of the contract, tests/metrics_ref.py holds the sums to the
 * any-order bound and the maps bit for bit.
 *
 * tb_run_compare: the kernel seam, like tb_run_fsr_easu: host arrays (w * h * 4 floats each), temporary device buffers, no scene, nothing the
 * context holds is read or written.  Flag TB_COMPARE_SUMS: test_rgba holds sums (rgb / w, unsampled pixels), as the accumulation does.
 * tb_set_reference: uploads the reference the stage compares with; it belongs to the context, is kept until it is replaced or released (NULL)
 * and goes with tb_destroy.
 * tb_compare: the stage.  surface TB_COMPARE_MEAN: the accumulation (sums / .w, unsampled pixels excluded); TB_COMPARE_DENOISED: the final
 * surface of tb_denoise, read as (rgb, 1).  Runs on the context's stream after whatever was enqueued; synchronous; its only read-back is the result
 * record, and the maps where asked for.  It writes neither the accumulation nor the AOVs, frame counter, history, denoised or guide surfaces:
 * tb_accum_digest is the same before and after and a render continued afterwards is the uninterrupted one.  Its scratch buffers belong to the
 * context and are kept while the size holds.  It equals tb_run_compare on host copies of the same two surfaces, field for field, bit for bit.
 * settings NULL: the defaults.  sq_err_map_or_null: w * h floats; ssim_map_or_null: (w - 10) * (h - 10) floats, untouched without a window.
 * TB_E_INVALID (the message names the cause): a null required pointer; a zero size or w * h > 2^26; peak or rel_epsilon not finite or <= 0;
 * unknown flags (TB_COMPARE_SUMS in tb_compare among them) or an unknown surface; no reference set, or one of another size than the rendered
 * surface; nothing rendered yet; TB_COMPARE_MEAN after tb_render_realtime; TB_COMPARE_DENOISED without a valid denoised surface (the rule of
 * tb_post_process with option "post_denoised").  TB_E_UNSUPPORTED: tb_set_reference / tb_compare on a tb_create_multi group or a peer handle. */
#define TB_COMPARE_SSIM 1u /* tb_compare_settings::flags: compute SSIM */
#define TB_COMPARE_SUMS 2u /* tb_run_compare only: the test picture holds sums */
#define TB_COMPARE_MEAN 0u
#define TB_COMPARE_DENOISED 1u
typedef struct tb_compare_settings { float peak; float rel_epsilon; uint32_t flags; } tb_compare_settings;
typedef struct tb_compare_result {
    uint64_t pixels, excluded, unsampled;          /* included pixels; excluded ones; unsampled ones, which are part of the excluded */
    uint64_t ssim_windows, ssim_windows_skipped;   /* both 0 without TB_COMPARE_SSIM */
    double mse, mae, rel_mse, max_abs, psnr, ssim; /* ssim NaN without TB_COMPARE_SSIM */
    float gpu_us;                                  /* HIP events around the kernels of this call */
} tb_compare_result;
void tb_default_compare_settings(tb_compare_settings* out); /* peak 1, rel_epsilon 0.01, flags TB_COMPARE_SSIM */
int tb_run_compare(tb_context* ctx, uint32_t w, uint32_t h, const float* test_rgba, const float* ref_rgba, const tb_compare_settings* settings_or_null,
                   tb_compare_result* out, float* sq_err_map_or_null, float* ssim_map_or_null);
int tb_set_reference(tb_context* ctx, uint32_t w, uint32_t h, const float* rgba_or_null);
int tb_compare(tb_context* ctx, uint32_t surface, const tb_compare_settings* settings_or_null, tb_compare_result* out, float* sq_err_map_or_null,
               float* ssim_map_or_null);

/* ---- host-only half of LoadScene (no device needed) ------------------------------------------------
 * The same parse / convert / BVH-build code tb_load_scene runs, exposed separately so that the
 * scene conversion and the BVH can be inspected and checked on machines without a GPU.  Nothing here
 * renders. */
typedef struct tb_host_scene tb_host_scene;
/* load_flags: bit 0 = flatten instanced shapes (option "flatten_instances"), bit 1 = do NOT flip texture v (the Assimp
 * convention; .pbrt / .pbf loads flip: m_flipTextureUVs, TracerBoy.cpp:1208,1222; option "flip_texture_uvs" = 0).
 * bvh_builder: option "bvh_builder" in bits 0-5; for builder 1 optionally (wave_tree + 1) << 6 -- option "wave_tree": 1 = off, 2 = on --,
 * (reinsertion passes + 1) << 8 and (share of the subtrees a
 * pass tries, percent) << 16 -- options "reinsertion_passes" / "reinsertion_share" -- and (percent of extra references from pre-splitting the
 * triangles with the emptiest boxes, <= 127) << 24 -- option "presplit"; a zero field leaves the library's own choice. */
int tb_host_scene_load(const char* pbrt_path, int bvh_builder, int load_flags, tb_host_scene** out, char* err, uint32_t err_len);
int tb_host_scene_procedural(int kind, uint32_t target_triangles, uint32_t seed, int bvh_builder, tb_host_scene** out, char* err, uint32_t err_len);
/* the host half of tb_load_meshes (above): host arrays only */
int tb_host_scene_from_meshes(const tb_scene_desc* desc, int bvh_builder, tb_host_scene** out, char* err, uint32_t err_len);
void tb_host_scene_free(tb_host_scene* s);
int tb_host_scene_view_get(tb_host_scene* s, TbSceneView* view);          /* pointers owned by s */
int tb_host_scene_camera(tb_host_scene* s, tb_camera* cam);
int tb_host_scene_info(tb_host_scene* s, tb_scene_info* info);
int tb_host_scene_digest(tb_host_scene* s, uint64_t* out);                /* what tb_scene_digest gives for the same scene and builder */
int tb_host_scene_frame_constants(tb_host_scene* s, const tb_output_settings* settings, uint32_t frame, float time_seed, TbPerFrameConstants* out);
/* layout-B arrays (what the kernels fetch) and the per-triangle builder inputs */
int tb_host_scene_layout_b(tb_host_scene* s, const TbNodeB** nodes, uint32_t* num_nodes, const TbTriB** tris, uint32_t* num_tris, uint32_t* root_ref);
/* The LDS image of the walk as a context uploads it for a scene that is LDS-resident (the same pure function builds both): node records
 * node_stride bytes apart from off_nodes, tri_copies axis-permuted copies of every layout-B triangle from off_tris (copy = kz * 2 + (d[kz] < 0)).
 * Child refs are offsets in 16-B units -- an inner ref from off_nodes, a leaf ref (leaf flag in the sign bit) from off_tris to the triangle's
 * first copy; root_ref is 0 or LEAF | 0.  stack_depth: entries per lane of the traversal stack, one more than a walk can hold.  out = null: sizes only
 * (off_nodes / off_tris are filled with the image). */
typedef struct tb_lds_image_info { uint32_t bytes, off_nodes, off_tris, num_nodes, num_tris, node_stride, tri_copies, root_ref, stack_depth; } tb_lds_image_info;
int tb_host_scene_lds_image(tb_host_scene* s, uint8_t* out, uint32_t capacity, tb_lds_image_info* info);
/* Whether every index the kernels can form into the shading tables is in range (host/lds_image.h SceneTablesInRange, what a context asks of a scene
 * before it launches the copy that fetches those tables unguarded): 1 or 0, TB_E_INVALID for a null table with a count.  hit_groups: 4 words per
 * record -- MaterialIndex, first vertex float, first index, unused. */
int tb_host_scene_tables_in_range(const TbTriB* tris, uint32_t num_tris, const uint32_t* hit_groups, uint32_t num_hit_groups, const uint32_t* indices,
    uint32_t num_indices, uint32_t num_vertex_floats, uint32_t num_materials);
/* What a 64-lane wave pays to walk a tree (host/wave_cost.h; builder 1's wave stage, option "wave_tree").  Trips of a wave through the inner loop's
 * body and leaf passes under the schedule of the LDS-resident walk, the lanes active in them, passes whose leaf step no lane takes, and
 * cost = inner_trips x inner_insts + leaf_trips x leaf_insts of tb_wave_stage_info. */
typedef struct tb_wave_trips { uint64_t inner_trips, leaf_trips, idle_passes, inner_active, leaf_active; double cost; } tb_wave_trips;
/* what the wave stage did when the scene was built: ran = 0 where it did not run (option off, another builder, a scene that is not LDS-resident);
 * before / after: its model rays over the tree it was given and the tree it returned (trips and cost only); depth_limit in nodes */
typedef struct tb_wave_stage_info { uint32_t ran, rays, seed, park_min, depth_limit, moves, evaluations, inner_insts, leaf_insts, reserved;
    tb_wave_trips before, after; double milliseconds;
    /* the search (docs/experiments/r13.md): places whose rays were priced, those of them abandoned because the partial sum had passed the best price,
     * rays walked again for them (the others kept their steps), workers, passes run, places per cut subtree (0 = every legal one), winners refused
     * because they raised the price of the validation rays, and that price before and after.  With more than one worker `abandoned` and
     * `rays_rewalked` depend on which worker finished first; the tree does not. */
    uint64_t places_priced, abandoned, rays_checked, rays_rewalked, places_screened;
    uint32_t threads, passes, places, validation_rejects, cuts_skipped, screen_waves, screen_keep, reserved2;
    double validation_before, validation_after;
    } tb_wave_stage_info;
/* up to 64 step strings of 'I' (inner node visited) and 'L' (triangle tested), each ended by a 0, replayed in lock step */
int tb_wave_replay(const char* const* steps, uint32_t lanes, uint32_t park_min, tb_wave_trips* out);
/* n rays over the tree of a one-level host scene with the kernels' rule: steps per ray and, where steps != null, the step strings back to back, each
 * ended by a 0 (TB_E_INVALID where steps_capacity is short).  t_max = null: the closest-hit walk's */
int tb_host_scene_wave_walk(tb_host_scene* s, uint32_t n, const float* origins, const float* dirs, const float* t_max, uint32_t* inner_steps,
    uint32_t* leaf_steps, char* steps, uint64_t steps_capacity);
/* the wave stage's model rays of a scene, `waves` waves of 64 (0 / 0 / -1: the stage's own seed, size and share of feeler waves); returns their number */
int tb_host_scene_wave_rays(tb_host_scene* s, uint32_t seed, uint32_t waves, int feeler_percent, float* origins, float* dirs, float* t_max, uint32_t capacity);
/* ... and what they cost over the scene's tree (park_min 0: that of a scene in LDS) */
int tb_host_scene_wave_cost(tb_host_scene* s, uint32_t seed, uint32_t waves, int feeler_percent, uint32_t park_min, tb_wave_trips* out);
int tb_host_scene_wave_stage(tb_host_scene* s, tb_wave_stage_info* out);
/* Builds the tree of a one-level host scene again with builder 1 and the wave stage on, for comparisons: the stage's model rays from `seed`, `waves`
 * and `feeler_percent` (0 / 0 / -1: its own); `places` per cut subtree: 0 = every legal place (the stage as it runs), K > 0 = the stage as it was
 * before it priced them all -- the K best by induced area, four passes, no validation rays; 3 gives that stage's tree byte for byte; `keep`: how
 * many places of a cut go on from the screen (the first 8 waves) to all waves, 0 = the stage's own 4, a number no cut reaches = no screen; `threads`:
 * option "wave_tree_threads" (0 = min(16, the CPUs the process may run on), 1 = serial; the same tree for every count).  out may be null. */
int tb_host_scene_wave_search(tb_host_scene* s, uint32_t seed, uint32_t waves, int feeler_percent, uint32_t places, uint32_t keep, int threads,
    tb_wave_stage_info* out);
/* Diagnostic: the build's own parse of a PBRT file in the record format of oracle/ref_dump.cpp. */
int tb_host_pbrt_dump(const char* pbrt_path, const char* out_path, char* err, uint32_t err_len);
int tb_host_scene_triangles(tb_host_scene* s, const float** positions, uint32_t* num_vertices, const uint32_t** tri_vertex_index,
                            const uint32_t** tri_geometry, const uint32_t** tri_primitive, const uint32_t** tri_flags, uint32_t* num_triangles);
/* point queries on the host (section 27 above): the rule of tb_nearest.h by brute force or by the kernel's walk, and the pruning slack's measurement */
int tb_host_scene_nearest(tb_host_scene* scene, uint32_t flags, uint64_t n, const TbQueryPoint* points, TbNearest* out);
int tb_host_scene_nearest_excess(tb_host_scene* scene, uint64_t n, const TbQueryPoint* points, float* worst_out);
/* winding numbers on the host (section 28 above): the rule of tb_winding.h by brute force or by the kernel's walk */
int tb_host_scene_winding(tb_host_scene* scene, uint32_t flags, uint64_t n, const TbQueryPoint* points, float beta, float* out);

#ifdef __cplusplus
}
#endif
#endif /* TRACERBOY_HIP_H */
