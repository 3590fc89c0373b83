/* context_internal.h -- what the translation units of the context share: the kernel launchers' C interface, the table of feature
 * sets, the owners of device resources, struct tb_context (the role of the reference's `class TracerBoy`, TracerBoy.h:158-398) and a few helpers.
 *   context.cpp         the C ABI (include/tracerboy_hip.h): kVariants, create / destroy, scene loads, edits, tb_render / tb_sync, read-backs, tb_set_option
 *   context_queries.cpp tb_get_option: the table of read-only names, then the options
 *   context_scene.cpp   finalizeScene: BVH builds on the GPU, node orders, layout C, uploads, the LDS scene image
 *   context_render.cpp  renderImpl, a sequence of named steps, and the pipelines it dispatches to
 *   context_group.cpp   multi-device groups: tb_create_multi, the group's render and gather, tile assignments, pack / unpack of owned tiles
 *   context_realtime.cpp the real-time chain (tb_render_realtime), the a-trous pass loop, the test hooks of rt_kernels.hip
 *   context_post.cpp    the output stage: tb_post_process, launchPostProcess
 *   render_state.cpp    render states: begin at a frame, save, load, merge
 *   context_denoise.cpp the denoise of a progressive render: dual-buffer variance + the a-trous filter
 *   context_guides.cpp  the guide pass of that denoise: first hits traced again and summed over frames
 *   context_upscale.cpp FSR 1 upscaling of the post-processed picture: EASU + RCAS
 *   context_neural.cpp  the neural still denoiser: the OIDN U-Net on the matrix cores, its layer seam and its stage
 *   context_sr.cpp      the neural 2 x super-resolution: the reference's DirectML network on the matrix cores, its seams and its stage
 *   context_budget.cpp  sample budgets: set / read, the noise target that stops converged pixels, its kernel seam
 *   context_compare.cpp image-quality metrics against a reference image: the kernel seam, the reference, the stage
 *   context_visualize.cpp the path inspector: a pixel's paths recorded again, the ray buffer, the overlay and its kernel seam
 *   context_dynamic.cpp dynamic scenes: staged vertices and instance transforms, the refit commit, the host copies' refresh
 *   context_rays.cpp    ray queries: tb_trace_rays, closest hits and any-hit occlusion of a caller's rays, host arrays or device buffers
 *   context_radiance.cpp radiance queries: tb_trace_radiance, the path tracer on a caller's rays, and tb_make_camera_rays
 *   context_bake.cpp    lightmap baking: tb_bake_lightmap, a UV atlas rasterised, its texels traced by the radiance query, resolved and dilated
 *   context_probes.cpp  light probes: tb_bake_probes, SH9 records of the radiance and the distances around points, and tb_sample_probes
 *   context_nearest.cpp point queries: tb_nearest_points and tb_bake_distance_field, the nearest surface point by a distance-ordered walk
 *   context_winding.cpp winding numbers: tb_winding_numbers, tb_bake_winding_field and the winding-signed point queries; the subtree moments
 *   context_meshes.cpp  scenes from caller arrays: tb_load_meshes, device arrays read to the host once, the swap into the context
 *   query_call.h        what the query entry points above share: a caller's arrays checked or staged, the timed launch, the common refusals
 *   host_api.cpp        every entry point that needs no device (host scenes, images, the plan); shares host_shared.h with the above, not this header
 *   options.h           the table of options      launch_plan.h  WHAT a call launches      launch_trials.h  the two trials (pure, like the plan)
 */
#pragma once
#include "host_shared.h"
#include "../kernels/pt_launch.h"
#include "../kernels/pt_device_features.h"
#include "launch_plan.h"
#include "launch_trials.h"
#include "options.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>
#include <memory>
#include <cmath>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

using namespace tbhost;

/* the kernel launchers of the feature sets: the lock-step copies' come with pt_launch.h (one per row of pt_copies.h); pipeline 4, the
 * split-role kernel (pt_split.inc): shading waves + traversal waves over an LDS ray queue */
#define TB_SPLIT_ARGS hipStream_t, const TbDeviceScene*, const TbPerFrameConstants*, const TbDeviceTargets*, const TbSplitParams*, uint32_t, uint32_t, \
    uint32_t, uint32_t, const TbTileMap*, int, int*
#define TB_SPLIT(name) hipError_t name(TB_SPLIT_ARGS);
extern "C" {
typedef hipError_t (*pt_split_fn)(TB_SPLIT_ARGS);
TB_SPLIT(pt_launch_split_matte) TB_SPLIT(pt_launch_split_env) TB_SPLIT(pt_launch_split_surf) TB_SPLIT(pt_launch_split_sss)
}

#include "../kernels/wf_types.h"
#define TB_WAVEFRONT_ARGS hipStream_t, int, const TbDeviceScene*, const TbPerFrameConstants*, const WfParams*, const WfQueue*, const WfQueue*, const WfQueue*, \
    const WfHits*, int, TbFloat4*, TbFloat4*, uint32_t
#define TB_WAVEFRONT(name) hipError_t name(TB_WAVEFRONT_ARGS);
extern "C" {
typedef hipError_t (*wf_variant_fn)(TB_WAVEFRONT_ARGS);
TB_WAVEFRONT(wf_launch_matte) TB_WAVEFRONT(wf_launch_env) TB_WAVEFRONT(wf_launch_surf) TB_WAVEFRONT(wf_launch_sss) TB_WAVEFRONT(wf_launch_vol)
}

namespace tbnn { struct PackedLayer; } /* nn_weights.h */

namespace tbctx {
using namespace tbhost;

/* A lock-step copy: its row of pt_copies.h and its launcher. */
struct Copy { const PtCopy* row; pt_variant_fn launch; };
/* A feature set.  Searched in order: the first one that covers what scene + settings need.  id: what option "last_variant" reports (stable across
 * insertions).  base / hi / lds: its copies by role (pt_copies.h) -- hi is used when LDS has room for hi->row->waves workgroups per CU (otherwise
 * its spills would buy no residency), lds in place of hi where the plan picks hi for a frame-group launch of a scene in LDS and lds->row->waves
 * workgroups fit (launch_plan.h LdsCopyFits); null for the sets without one.
 * wf: the wavefront pipeline's launcher of the feature set (pipeline 2; none for the full set); pooled: pipeline 3 exists. */
struct Variant { const char* name; const Copy* base; const Copy* hi; const Copy* lds; int id; wf_variant_fn wf; bool pooled; pt_split_fn split;
    uint32_t features() const { return base->row->features; }
    uint32_t wavesHi() const { return hi ? hi->row->waves : 0u; }
    uint32_t wavesLds() const { return lds ? lds->row->waves : 0u; }
    uint32_t stashHi() const { return hi ? hi->row->stash : 0u; } /* LDS entries per lane behind the stacks: frame groups, scenes from memory, one level */
};
extern const Variant kVariants[];
extern const int kNumVariants;

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

/* Owners of what the library takes from HIP: device memory, streams, events, host-mapped words.  None can be copied; each destructor gives its
 * handle back, on the device that is current then -- a context's members go in tb_destroy, after its hipSetDevice; a function's locals go inside
 * guarded()'s DeviceScope.  Nothing else in the host code frees or destroys.
 * g_liveDeviceBytes: device bytes the library holds, all contexts of the process together (option "debug_live_device_bytes"): added where ensure
 * allocates, subtracted where DevBuf::release frees -- a context that is destroyed leaves the count where it found it. */
extern std::atomic<int64_t> g_liveDeviceBytes;
struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); g_liveDeviceBytes -= (int64_t)bytes; } p = nullptr; bytes = 0; } /* early, on purpose: a resize drops the AOVs, a load the old scene */
};
struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream&) = delete; DevStream& operator=(const DevStream&) = delete;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
    void create() { HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    operator hipStream_t() const { return s; }
};
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete; DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
    hipEvent_t create(unsigned flags = hipEventDefault) { if (!e) HIP_TRY(hipEventCreateWithFlags(&e, flags)); return e; } /* the event, made at its first use */
    operator hipEvent_t() const { return e; }
};
struct MappedWords { /* zeroed host memory the device writes and the host polls */
    uint32_t* p = nullptr;
    MappedWords() = default;
    MappedWords(const MappedWords&) = delete; MappedWords& operator=(const MappedWords&) = delete;
    ~MappedWords() { if (p) (void)hipHostFree(p); }
    uint32_t* create(size_t bytes) { if (!p) { HIP_TRY(hipHostMalloc((void**)&p, bytes, hipHostMallocMapped)); memset(p, 0, bytes); } return p; }
    operator uint32_t*() const { return p; }
};

} // namespace tbctx
using tbctx::DevBuf;

struct tb_context {
    tb_context() = default;
    tb_context(const tb_context&) = delete; tb_context& operator=(const tb_context&) = delete;
    int device = 0;
    /* frame-group launches alternate between two side streams and two sample buffers: launch k+1 starts while the last paths
     * of launch k drain; the folds stay on `stream`, in order (renderImpl).  The streams stand before every buffer and event: they go last */
    tbctx::DevStream stream, side[2];
    tbctx::DevEvent ev0, ev1, evKernelStart, evKernel; /* evKernelStart..evKernel: the render's first path-tracing launch */
    tbctx::DevEvent evPt[2], evFold[2], evMain;
    DevBuf fgSamples[2];
    int numCUs = 0;           /* of `device` (deviceCUs) */
    uint32_t launchEpoch = 0; /* TbDeviceTargets::launchEpoch of the last frame-group launch */
    DevBuf fgSlotLog[2]; /* frame-group mode: the workgroups' logs of bound slots (TbDeviceTargets::slotLog) */
    DevBuf fgHits[2];   /* primary-visibility pre-pass: 16-B or 32-B record of every sample's first hit (TbDeviceTargets::primaryHits) */
    DevBuf regionCost, regionOrder[2]; uint64_t regionCostKey = ~0ull; /* costly regions first (TbDeviceTargets::regionCost / regionOrder): 2^20 counts; per side stream 1 + 2 x regions words */
    /* the adaptive launch (option "adaptive"): live list, its count and the list pass's scratch (pt_launch_live_list); what the last call was */
    DevBuf liveList; size_t liveCountOffset = 0; /* bytes of scratch before the count word */ bool lastAdaptive = false; uint64_t lastOwnedPixels = 0;
    /* the sample budget (context_budget.cpp): per pixel the global frame index at which it stops receiving samples; set: one is
     * held (values: its device copy, width x height words); lastBudgeted: the last call was planned under it.  stop: tb_budget_stop_converged's
     * scratch -- section 12's prepared and filtered surfaces of its own, and its two counters */
    struct Budget { DevBuf values, prepared, filtered, counts; bool set = false; uint32_t width = 0, height = 0; bool lastBudgeted = false;
        tbctx::DevEvent ev[2]; float lastStopMs = 0.0f; /* option last_budget_stop_us: the last noise target's three passes (HIP events) */ } budget;
    DevBuf stackOverflow; /* split traversal stack of the higher-occupancy kernel copies on deep trees (pt_scene.h) */
    std::vector<const void*> warmedLaunchers; /* frame-group kernels that have run once on both side streams (renderImpl) */
    uint32_t fgLaunch = 0; bool sideOrdered = false; /* sideOrdered: the side streams have been ordered after everything else on `stream` */
    uint32_t lastKernelFrames = 0; float lastKernelMs = 0.0f;
    std::string err;
    HostScene scene; bool hasScene = false;
    tb_camera camera{};
    std::vector<DevBuf> sceneBufs;
    TbDeviceScene ds{};
    uint32_t sceneFeatures = 0; bool sceneInLds = false;
    /* every index the kernels can form into the shading tables is in range (lds_image.h SceneTablesInRange; finalizeScene).  A material edit
     * keeps it: it changes no count and no index.  The copy for scenes in LDS, which fetches unguarded, needs it (context_render.cpp pickCopy) */
    bool tablesInRange = false;
    /* surfaces */
    uint32_t width = 0, height = 0;
    DevBuf output, jittered, aov[8], stats, rayStats, packed;
    DevBuf postOut, postRgba8, postHistogram, postAverage; /* output stage (post_kernels.hip) */
    /* real-time chain (context_realtime.cpp, rt_kernels.hip): ping-pong histories like TracerBoy.h:513-518,747-749.  last: which buffer holds each
     * stage's last output; lastRender: the last render was tb_render_realtime; chainFrame: renderImpl is rendering tb_render_realtime's frame: its
     * positions go to world-position half `active` (fillTargets) */
    struct Realtime {
        DevBuf indirect[2], moment[2], finalOut[2], denoise[2], composited;
        uint32_t active = 0, width = 0, height = 0; int last[5] = {-1, -1, -1, -1, -1};
        bool lastRender = false, chainFrame = false; tb_camera prevCamera{};
    } rt;
    /* wavefront pipeline: two ping-pong extend queues (4 columns), one shadow queue (11 columns), hits, samples, counters */
    DevBuf wfCols[2][6], wfShadowCols[12], wfHitA, wfHitG, wfSamples, wfCounts, workCounter;
    uint64_t wfCapacity = 0, wfSampleCapacity = 0;
    int lastPipeline = 0;
    uint32_t samplesRendered = 0;
    /* render states (render_state.cpp): the surfaces hold the samples of frames [firstFrame, samplesRendered) */
    uint32_t firstFrame = 0;
    DevBuf stateScratch; /* the digest's per-workgroup partials and its two results (state_launch.h) */
    tbctx::DevEvent evState[2]; float lastStateDigestMs = 0.0f, lastStateAddMs = 0.0f; /* options last_state_digest_us / last_state_add_us */
    uint64_t sceneDigest = 0, sceneDigestKey = ~0ull; uint32_t materialEdits = 0; /* tb_scene_digest, cached per (sceneGeneration, materialEdits) */
    /* the denoise of a progressive render (context_denoise.cpp): prepared, filtered, the filter passes' ping-pong, final, and
     * what the filter reads of the guide pass (normals, positions: resolved by tb_denoise; mode: option denoise_guides of the last tb_denoise).
     * valid: they belong to the accumulation surfaces as they are now -- whatever writes those clears it (touchAccumulation); lastPass: which
     * pass[] holds the last filter pass's output, -1 = no pass ran.  aovStaleUntilCall: the AOVs hold the first hits of frame samplesRendered - 1
     * once callCount has reached it (a state that was begun or loaded brings frames without AOVs).  lastMs: option last_denoise_us */
    struct StillDenoise {
        DevBuf prepared, filtered, pass[2], finalOut, normals, positions; bool valid = false; int lastPass = -1, mode = 0; uint64_t aovStaleUntilCall = 0;
        tbctx::DevEvent ev[2]; float lastMs = 0.0f;
    } dn;
    /* the guide pass (context_guides.cpp): the sums over its frames (albedo, normal, position) and its half of a split stack.
     * valid: they were traced of the scene, camera, size, settings and time seed in key, and no history reset has come since (resetHistory clears
     * it; guidesCurrent compares the key).  lastMs, lastOverflow: options last_guides_us, last_guides_stack_overflow */
    struct GuideKey { uint32_t sceneGeneration, materialEdits, width, height, alphaTest; tb_camera camera; tb_output_settings settings; float time; };
    struct Guides {
        DevBuf sum[3], overflow; bool valid = false; GuideKey key{};
        tbctx::DevEvent ev[2]; float lastMs = 0.0f; uint32_t lastOverflow = 0;
    } guides;
    /* FSR 1 upscaling (context_upscale.cpp): per surface type the EASU output and the RCAS output, at the size of the last
     * tb_upscale that ran that chain; events around the passes: [2 t] before EASU, [2 t + 1] between the passes, [4 + t] after RCAS */
    struct Fsr { DevBuf mid[2], out[2]; tbctx::DevEvent ev[6]; float lastUpscaleMs = 0.0f, lastEasuMs = 0.0f, lastRcasMs = 0.0f; } fsr;
    /* what both neural stages hold.  Activations, sized at the first use and kept while the size holds: the packed input and two tensors the
     * layers alternate between.  result, rgba8: the stage's float picture and its 8-bit one.  ev, lastMs: around the last network */
    struct NetStage { DevBuf input, pingPong[2], result, rgba8; tbctx::DevEvent ev[2]; float lastMs = 0.0f; };
    /* the neural still denoiser (context_neural.cpp).  inputs: 0 = no weights loaded, else enc_conv0's input channels (3 or 9);
     * in / out: the layers' channel counts; splitA: how many of a layer's input channels come from its first source (all of them, except where a
     * decoder reads an upsampled tensor in front of a skip tensor); weight / bias: the layers repacked for nn_convk.  skip: the three pooled skip
     * tensors; aux: tb_denoise_neural's resolved albedo and normals.  lastMs: option last_neural_us */
    struct Neural : NetStage {
        uint32_t inputs = 0, in[16] = {}, out[16] = {}, splitA[16] = {};
        DevBuf weight[16], bias[16], skip[3], aux[2];
    } nn;
    /* the neural 2 x super-resolution (context_sr.cpp).  loaded: tb_sr_load has succeeded; in / out / kernel: the seven layers'
     * channel counts and filter sizes; weight / bias: the layers repacked for nn_convk (the last has no bias).  lastMs: option last_sr_us */
    struct Sr : NetStage {
        bool loaded = false; uint32_t in[7] = {}, out[7] = {}, kernel[7] = {};
        DevBuf weight[7], bias[7];
    } sr;
    /* image-quality metrics (context_compare.cpp).  reference: the picture tb_set_reference uploaded, refW x refH (0: none);
     * scratch: the workgroups' records and the result (cmp_launch.h); sqErr, ssim: the two maps, held once a call has asked for them and while
     * the size holds.  ev: around the kernels of a tb_compare (tb_compare_result::gpu_us) */
    struct Compare { DevBuf reference, scratch, sqErr, ssim; uint32_t refW = 0, refH = 0; tbctx::DevEvent ev[2]; } cmp;
    /* the path inspector (context_visualize.cpp).  rays: the reference's ray buffer behind 12 B of padding -- the count word,
     * then at once the records, 16-B aligned; stored: the rays it holds, the host's count (resetHistory and tb_clear_paths zero it; the word on the
     * device is rewritten by every tb_record_paths).  overflow: the recorder's half of a split stack.  out, out8: the overlay's two pictures;
     * depthSource: option visualize_depth_source of the last overlay.  evPaths, evOverlay: around the kernels (last_paths_us, last_visualize_us) */
    struct Visualize {
        DevBuf rays, overflow, out, out8; uint32_t stored = 0; int depthSource = 0;
        tbctx::DevEvent evPaths[2], evOverlay[2]; float lastPathsMs = 0.0f, lastOverlayMs = 0.0f;
    } vis;
    /* ray queries (context_rays.cpp).  counter: the work counter of the any-hit walk's refilling form, made at its first
     * launch and kept: the device path of tb_trace_rays allocates nothing per call */
    struct RayQueries { DevBuf counter; } rq;
    /* point queries (context_nearest.cpp): the events around the last query's kernel; lastMs: option last_nearest_us */
    struct PointQueries { tbctx::DevEvent ev[2]; float lastMs = 0.0f; } pq;
    /* radiance queries (context_radiance.cpp).  counter: the work counter of the refilling form, made at its first launch and
     * kept; overflow: the query's half of a split stack.  lastMs, lastVariant, lastForm, lastLaunches: options last_radiance_us,
     * last_radiance_variant (the feature set's id, -1 before the first query), last_radiance_form, last_radiance_launches */
    struct Radiance { DevBuf counter, overflow; tbctx::DevEvent ev[2]; float lastMs = 0.0f; int lastVariant = -1, lastForm = 0; uint32_t lastLaunches = 0; } rad;
    /* dynamic geometry (context_dynamic.cpp): made at the first tb_update_* / tb_set_instance_transforms of a scene, released
     * with the scene (releaseScene); a context that never updates holds none of it.  positions / normals: the staged arrays, 3 floats per vertex
     * (normals at the first tb_update_normals); triVerts, triSlot, nodeSlot, schedule, rootBox: the tables of refit_launch.h, made once per
     * topology, with their host halves.  dirtyPositions / dirtyNormals: the staged vertex ranges [first, end) since the last commit;
     * transforms / transformStaged: staged objectToWorld rows per instance.  hostStale: a commit has changed the device tree and c->scene's bvhA,
     * nodesB, trisB, positions (and, vertexBufferStale, vertexBuffer) are what they were before -- refreshHostScene brings them up on first demand.
     * refitSinceBuild: the tree's topology was built of other positions than it holds.  lastMs: option last_refit_us */
    struct Dynamic {
        bool ready = false, hostStale = false, vertexBufferStale = false, refitSinceBuild = false;
        DevBuf positions, normals, triVerts, triSlot, nodeSlot, schedule, levelFirstDevice, rootBox;
        std::vector<uint32_t> hostTriVerts, levelFirst;
        std::vector<std::pair<uint32_t, uint32_t>> dirtyPositions, dirtyNormals;
        std::vector<float> transforms; std::vector<uint8_t> transformStaged;
        tbctx::DevEvent ev[2]; float lastMs = 0.0f;
        /* tb_recompute_normals: the marked vertex ranges since the last commit; the tables of a recomputation
         * (refit_launch.h RefitNormalTables) and the face vectors, made at the first call only; the events around its two launches */
        std::vector<std::pair<uint32_t, uint32_t>> markedNormals;
        bool normalTablesReady = false; uint32_t normalSlots = 0;
        DevBuf normalTriVerts, normalRowStart, normalSlotTable, faceVectors;
        tbctx::DevEvent evNormals[2];
    };
    std::unique_ptr<Dynamic> dyn;
    /* winding numbers (context_winding.cpp): made at the first winding call of a scene, released with the scene
     * (releaseScene); a context that never asks holds none of it.  triSlot, nodeSlot, schedule, levelFirst: the refit's slots and schedule
     * (treeSchedule), made once per topology; moments, areas, root: the subtree moments of wn_launch.h, fitted at scene generation fittedOf -- a
     * commit moves the generation on, so the next call fits them again.  ev / evFit: around the walk and the fit (options last_winding_us,
     * last_winding_fit_us) */
    struct Winding {
        DevBuf triSlot, nodeSlot, schedule, levelFirstDevice, moments, areas, root;
        std::vector<uint32_t> levelFirst; bool tablesReady = false, fitted = false; uint32_t fittedOf = 0;
        tbctx::DevEvent ev[2], evFit[2]; float lastMs = 0.0f, lastFitMs = 0.0f;
    };
    std::unique_ptr<Winding> wn;
    /* lightmap baking (context_bake.cpp): made at the first tb_bake_lightmap of a scene, released with the scene
     * (releaseScene); a context that never bakes holds none of it.  rays, texels, sums: the atlas in row-major order, what tb_read_bake returns and
     * TB_BAKE_ACCUMULATE adds to; rgba: the resolve's and the fill passes' ping-pong; scratch: the rasteriser's (bake_launch.h); triVerts,
     * positions: the scene's triangles and vertices as the rasteriser reads them, positions of scene generation positionsOf.  held: the buffers
     * hold a finished bake of width x height, rasterised at scene generation rasterOf.  ev: before the raster, after it, before the resolve,
     * after the last fill pass (options last_bake_raster_us, last_bake_finish_us; the trace between is the radiance query's own two events) */
    struct Bake {
        DevBuf rays, texels, sums, rgba[2], scratch, triVerts, positions, covered;
        uint32_t width = 0, height = 0, rasterOf = 0, positionsOf = 0xffffffffu, lastCovered = 0; bool held = false;
        tbctx::DevEvent ev[4]; float lastRasterMs = 0.0f, lastTraceMs = 0.0f, lastFinishMs = 0.0f;
    };
    std::unique_ptr<Bake> bake;
    /* light probes (context_probes.cpp): made at the first tb_bake_probes of a scene, released with the scene (releaseScene);
     * a context that never bakes probes holds none of it.  radRays, queryRays: the two ray records of one batch; sums, hits: what the two queries
     * answered -- of one batch, or, where the bake keeps its maps (TB_PROBES_KEEP_MAPS), of every ray of the bake, which tb_read_probe_maps
     * returns and TB_PROBES_ACCUMULATE adds to; records: the n probes; positions: the host path's copy of the caller's.  held: records holds a
     * finished bake of n probes at `resolution`, traced at scene generation bakedOf; mapsHeld: sums and hits hold all of its rays.  ev: around the
     * stages of a batch (options last_probes_*_us, summed over the batches; the trace is the radiance query's own two events) */
    struct Probes {
        DevBuf radRays, queryRays, sums, hits, records, positions;
        uint64_t n = 0; uint32_t resolution = 0, bakedOf = 0, lastBatches = 0; bool held = false, mapsHeld = false;
        tbctx::DevEvent ev[5]; float lastRaysMs = 0.0f, lastTraceMs = 0.0f, lastHitsMs = 0.0f, lastProjectMs = 0.0f;
    };
    std::unique_ptr<Probes> probes;
    tb_output_settings lastSettings{}; bool haveLastSettings = false;
    float lastTime = 0.0f;
    uint32_t selX = 0xffffffffu, selY = 0xffffffffu;
    TbTileMap tiles{0, 1, 64, 64};
    Options options; /* options.h; read with opt<OPT_name>(c) */
    float lastMs = 0.0f;
    std::string lastVariant;
    uint32_t lastCopyWaves = 0; /* waves per SIMD of the copy the last lock-step launch ran (option last_copy_waves; 0 = the base copy) */
    int lastNodeLayout = 0; /* 1: the last render walked the compact layout-C nodes */
    int lastSlotLogCap = 0;
    /* renderImpl */
    PrepassTrial prepassTrial; OverlapTrial overlapTrial; CallRec callRec[8]; /* launch_trials.h */
    tbctx::DevEvent evCallEnd[8]; uint64_t callCount = 0; int lastOverlap = 0;
    tb_launch_plan lastPlan{}; /* what PlanLaunch decided for the last render (options last_plan_rule_*) */
    uint64_t kernelEventStamp = 0; /* counts the renders that have recorded evKernelStart / evKernel: a trial's sample belongs to the render it was asked of */
    uint32_t sceneGeneration = 0; /* counts finalizeScene calls */
    float interiorWalkTriangleShare = 0; /* finalizeScene */
    uint32_t hitPrimBits = 32, hitGeomBits = 32; /* finalizeScene: bits that hold every primitive index / hit-group index of the scene (compact hit records) */
    int lastCompactHits = 0;
    DevBuf debugCounters; /* TbDeviceTargets::debugCounters (16 words, zeroed once) */
    /* pipeline 4: host-mapped abort word of the split-role kernel (renderSplit); travWaves * 100 + shadeWaves of the last launch */
    DevBuf splitProf; tbctx::MappedWords splitAbort; int lastSplitWaves = 0;
    int lastFgPar = 0;          /* which of the two sample buffers the last frame-group launch wrote (debug query) */
    int lastPrimaryPrepass = 0; /* 1: the last render took its first hits from the primary-visibility pre-pass */
    int lastFirstBounce = 0;    /* 1: ... its paths' state after the first bounce from the first-bounce pass */
    /* Multi-device group (context_group.cpp, tb_create_multi): this context is device 0 of the group and owns the assembled frame; `peers` are the
     * contexts of the other devices.  A render splits the frame into 64x64 tiles dealt round-robin over the devices (DESIGN.md
     * section 7), every device renders its own, the peers' packed tiles come over with hipMemcpyPeerAsync (xGMI) and are un-permuted
     * into this context's accumulation surfaces.  One host thread drives all devices; nothing blocks until the final wait. */
    struct Group {
        std::vector<tb_context*> peers;
        tb_context* owner = nullptr;     /* set on a peer: API calls on a peer handle are refused */
        DevBuf packed[2], gathered[2];   /* [0] output, [1] jittered: this device's packed tiles; (owner) world x capacity gathered tiles */
        tbctx::DevEvent evSent, evDone;  /* evSent (peer): its packed tiles are on their way; evDone (owner): the un-permute of the last group render has read `gathered` */
    } group;
    bool compactTried = false; /* layout C was asked for and built -- or could not be built -- for the loaded scene (ensureCompactNodes) */
};

namespace tbctx {

int fail(tb_context* c, int code, const std::string& msg);
/* forget the accumulated frames: the next render starts at frame 0 (where the kernels overwrite the surfaces instead of adding to them) */
/* (and the recorded paths: they were traced of the scene, camera, size and settings that have just changed) */
inline void resetHistory(tb_context* c) { c->samplesRendered = 0; c->firstFrame = 0; c->dn.valid = false; c->guides.valid = false; c->vis.stored = 0; }
/* the accumulation surfaces are about to change (a render, a state that is begun, loaded or added): the denoised surfaces no longer belong to them */
inline void touchAccumulation(tb_context* c) { c->dn.valid = false; }
/* an entry point that only a group's own context may be asked */
#define TB_REFUSE_PEER(c) do { if ((c) && (c)->group.owner) return fail((c), TB_E_INVALID, \
    "this context is a member of a multi-device group: call the group's context"); } while (0)
template <Opt K> inline int64_t opt(const tb_context* c) { return c->options.get<K>(); }

/* Every entry point runs on its context's device and hands the calling thread back the device it came with: a host that shares the
 * thread (torch in bench.py, an application's own hipMalloc) would otherwise go on allocating and launching on the last peer of a
 * device group. */
struct DeviceScope {
    int saved = -1;
    explicit DeviceScope(int dev) { if (hipGetDevice(&saved) != hipSuccess) saved = -1; (void)hipSetDevice(dev); }
    ~DeviceScope() { if (saved >= 0) (void)hipSetDevice(saved); }
};

/* a refusal thrown below an entry point's body (query_call.h): guarded() answers it as fail(c, code, msg) */
struct Refusal { int code; std::string msg; };

template <class F> int guarded(tb_context* c, F f)
{
    if (!c) return TB_E_INVALID;
    try { DeviceScope scope(c->device); return f(); }
    catch (const Refusal& r) { return fail(c, r.code, r.msg); }
    catch (const std::bad_alloc&) { return fail(c, TB_E_DEVICE, "out of host memory"); }
    catch (const std::exception& e) {
        std::string m = e.what();
        int code = TB_E_PARSE;
        if (m.find("hip") == 0 || m.find("HIP") != std::string::npos) code = TB_E_DEVICE;
        else if (m.find("open") != std::string::npos || m.find("Couldn't") != std::string::npos) code = TB_E_IO;
        else if (m.find("not supported") != std::string::npos || m.find("unsupported") != std::string::npos) code = TB_E_UNSUPPORTED;
        return fail(c, code, m);
    }
}

void ensure(DevBuf& b, size_t bytes); /* b holds exactly `bytes`: as it is if it does already, else freed and allocated */
template <class T> const T* upload(tb_context* c, const std::vector<T>& v)
{
    if (v.empty()) return nullptr;
    DevBuf b; ensure(b, v.size() * sizeof(T));
    HIP_TRY(hipMemcpyAsync(b.p, v.data(), b.bytes, hipMemcpyHostToDevice, c->stream));
    c->sceneBufs.push_back(std::move(b));
    return (const T*)c->sceneBufs.back().p;
}
/* v into a buffer the context keeps (at least 16 B), on the stream, not waited for: the tables of a refit and of the winding numbers' moment fit */
template <class T> void uploadInto(tb_context* c, DevBuf& b, const std::vector<T>& v)
{
    ensure(b, std::max<size_t>(16, v.size() * sizeof(T)));
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
}
/* The test hooks' staging (tb_trace_closest, tb_device_math, tb_run_*): temporary buffers only, nothing of the context but its stream.  staged: a
 * buffer of its own holding a copy of a host array; scratch: one to write into; copyBack: all of it to the host, where the caller gave a pointer --
 * d.bytes is what the hook asked for, since ensure makes a buffer hold exactly that */
inline DevBuf scratch(size_t bytes) { DevBuf d; ensure(d, bytes); return d; }
inline DevBuf staged(const void* host, size_t bytes) { DevBuf d = scratch(bytes); HIP_TRY(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice)); return d; }
inline void copyBack(void* host, const DevBuf& d) { if (host) HIP_TRY(hipMemcpy(host, d.p, d.bytes, hipMemcpyDeviceToHost)); }
/* why a hook or tb_upscale refuses a surface of that size; null: it does not */
inline const char* surfaceRefusal(uint32_t W, uint32_t H)
{
    if (W == 0 || H == 0) return "a dimension is 0";
    if ((uint64_t)W * H > (1ull << 24)) return "more than 2^24 pixels";
    return nullptr;
}
/* a context and the peers of its group */
inline std::vector<tb_context*> members(tb_context* c) { std::vector<tb_context*> all(1, c); all.insert(all.end(), c->group.peers.begin(), c->group.peers.end()); return all; }

/* context_scene.cpp */
void releaseScene(tb_context* c);
uint32_t sceneFeatureMask(const HostScene& s);
uint32_t sceneTextureUse(const tb_context* c);
uint32_t settingsFeatureMask(const tb_context* c, const tb_output_settings& s, bool aov);
void ensureCompactNodes(tb_context* c);
void finalizeScene(tb_context* c, bool build = true); /* build = false: c->scene already holds a built, reordered tree (a peer of a multi-device group) */
void BuildTlasGpu(tb_context* c, HostScene& s, const std::vector<float>& blasBoxes, std::vector<TbNodeB>& top, uint32_t& rootRef, uint32_t& depth);
/* context_dynamic.cpp: the host copies of the geometry (HostScene::bvhA, nodesB, trisB, positions, vertexBuffer, sceneMin / sceneMax) as the device
 * holds them now.  Every reader of those members outside the load path calls it first; it does nothing unless a commit has left them stale */
void refreshHostScene(tb_context* c);
/* context_dynamic.cpp: the slots and the height-ordered schedule of a bottom-up pass over s's layout-B tree (refit_launch.h RefitTables) */
void treeSchedule(const tbhost::HostScene& s, std::vector<uint32_t>& triSlot, std::vector<uint32_t>& nodeSlot, std::vector<uint32_t>& schedule,
    std::vector<uint32_t>& levelFirst);
/* context_rays.cpp: the closest-hit launch of tb_trace_rays on n device rays into n device hit records, on the context's stream, not waited for.
 * tb_trace_rays and tb_bake_probes (context_probes.cpp) both end here.  The caller has checked the scene and the pointers. */
void traceClosestOnDevice(tb_context* c, uint32_t n, const TbQueryRay* rays, TbQueryHit* hits);
/* context_render.cpp */
bool historyRelevantChange(const tb_output_settings& a, const tb_output_settings& b);
int deviceCUs(tb_context* c);
std::string splitAbortMessage(tb_context* c, bool clear = true);
int renderImpl(tb_context* c, uint32_t W, uint32_t H, uint32_t n, const tb_output_settings* settings, float timeSeed, bool sync);
void cameraConstants(const TbPerFrameConstants& pf, uint32_t W, uint32_t H, TbDeviceTargets& tg);
/* context_post.cpp: the output stage on the context's stream, into postOut / postRgba8; not waited for */
int launchPostProcess(tb_context* c, const tb_post_settings* post, uint32_t outputType);
/* context_group.cpp */
int shareSceneWithPeers(tb_context* c);
int renderGroup(tb_context* c, uint32_t W, uint32_t H, uint32_t n, const tb_output_settings* s, float t);
/* context_realtime.cpp: n passes of the a-trous filter (DenoiserPass.cpp:61-93) enqueued on `stream`.  Pass i reads the output of pass i - 1 -- the
 * first reads `first`, which every pass also gets as the undenoised surface -- and writes pingPong[i & 1], with OffsetMultiplier = 1 << i.
 * Returns which of the two holds the last output, -1 when n is 0. */
int runAtrousPasses(hipStream_t stream, uint32_t W, uint32_t H, uint32_t n, const TbFloat4* first, const TbFloat4* normals, const TbFloat4* positions,
    DevBuf (&pingPong)[2], const tb_denoiser_settings& dn, uint32_t frameCount);
/* context_guides.cpp: the guide surfaces belong to the context as it is now */
bool guidesCurrent(const tb_context* c);
/* context_neural.cpp, shared with context_sr.cpp: the bytes of a w x h tensor with its channels padded to 32; a layer's repacked weights on the device
 * (bias as fp32, zeros where the layer has none); unpadded NHWC on the host -> channels padded to 32 */
size_t tensorBytes(uint32_t w, uint32_t h, uint32_t channels);
void uploadLayer(const tbnn::PackedLayer& p, DevBuf& weight, DevBuf& bias);
std::vector<uint16_t> padChannels(const uint16_t* in, size_t pixels, uint32_t c);
/* The body of both layer seams, tb_run_conv3x3 and tb_run_conv, inside their guarded(): `name` heads the refusals; pool: -1, the seam has no
 * pool flag; else whether the max-pool follows (out is then halved).  d and every pointer but bias are checked here. */
int runConvSeam(tb_context* c, const char* name, const tb_conv_desc* d, int pool, const uint16_t* inA, const uint16_t* inB, const uint16_t* weight,
    const uint16_t* bias, uint16_t* out);
/* A stage's network and what follows it: `network` enqueues its kernels, which write the outW x outH RGBA32F device surface `result`, between the
 * stage's two events; then the 8-bit store where rgba8 is asked for, a synchronise, lastMs, and the copies to the host pointers that are not null */
void runStage(tb_context* c, tb_context::NetStage& n, const std::function<void()>& network, uint32_t outW, uint32_t outH, const void* result,
    float* rgbaF32, uint8_t* rgba8);

} // namespace tbctx
