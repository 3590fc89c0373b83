/* cli.cpp -- headless replacement of the reference's Win32 shell (WinMain/WinMain.cpp, D3D12App.cpp):
 *   tracerboy-hip scene.pbrt [--width W] [--height H] [--spp N] [--depth D] [--seed-time T] [--device I]
 *                 [--builder lbvh|sah|lbvh-gpu|treelets|treelets-gpu] [--blue-noise 0|1] [--tonemap 0..7] [--exposure E|auto]
 *                 [--out frame.png|frame.pfm|frame.exr]
 *                 [--ranks N] [--adaptive P [--adaptive-after F] [--adaptive-chunk C] [--adaptive-test frame|call]]
 *                 [--save-state f.tbs] [--resume f.tbs] [--add g.tbs]... [--frames A:B] [--checkpoint-every N]
 *                 [--denoise] [--denoise-iterations N] [--denoise-guides K [--denoise-demodulate]]
 *                 [--upscale WxH | --render-scale F] [--fsr-sharpness S]
 *                 [--denoise-neural FILE.tza [--denoise-guides K]]
 *                 [--upscale-neural FILE.bin]
 *                 [--crop X0,Y0,X1,Y1] [--spp-map FILE] [--noise-target T [--noise-after F] [--noise-chunk C]]
 *                 [--reference FILE [--metrics-out FILE] [--metrics-every N] [--error-map FILE.pfm]]
 *                 [--visualize-rays X,Y [--visualize-frames A:B] [--visualize-width R] [--visualize-depth D] [--visualize-count N] [--paths-out FILE.jsonl]]
 *   tracerboy-hip --compare A B [--metrics-out FILE] [--device I]
 * Uses only the C ABI (include/tracerboy_hip.h), the way an embedding application would.
 *
 * --ranks N (N > 1): the frame tiled across N GPUs of the node, natively.  The process starts N copies of itself -- before it
 * has made a single HIP call -- one per GPU (rank r -> device r); each loads the scene, takes its tiles (tb_set_tile_assignment:
 * tile t -> rank t % N), renders, packs (tb_pack_owned_device) and the packed HDR buffers travel to rank 0 over RCCL / xGMI as ONE
 * grouped exchange (ncclGroupStart; rank 0: N - 1 x ncclRecv, the others: one ncclSend; ncclGroupEnd -- SURVEY.md 8e), on the
 * context's stream; rank 0 un-permutes them on the device straight into its own accumulation surface
 * (tb_unpack_gathered_device -> tb_accum_device_ptr) and writes the picture exactly like the one-GPU path.  librccl is loaded with
 * dlopen, so the tool still runs where it is absent; the unique id goes from rank 0 to the others through a file.
 * TB_CLI_FORCE_RCCL=1 runs the same sequence with one rank (communicator of size 1, self-gather): the test of the plumbing on a
 * one-GPU machine.
 * Output by extension: .png = what the reference presents (auto exposure + PostProcessCS tonemap, 8-bit back buffer,
 * tb_post_process); .pfm = linear radiance sum(rgb*w)/sum(w), the value PostProcessCS divides out before tonemapping
 * (PostProcessCS.hlsl:23-47), RGB float32, bottom row first; .exr = the same radiance as OpenEXR (RGBA float32, A = 1).
 *
 * --adaptive P: stop sampling converged pixels (option "adaptive", ConvergencePercentage = P).  One plain call of
 * min(F + 1, N) frames (F = --adaptive-after, default 1024, the reference's threshold), then adaptive calls of C frames (--adaptive-chunk, default
 * 64) until N frames are rendered or no pixel is live; one line per call: frames so far, live pixels at the call's start, milliseconds.  With
 * --ranks every rank runs the schedule over its own tiles.  --adaptive-test call (option "adaptive_test" = 1; default frame): a pixel is tested once
 * per call, at the call's first frame, and the live ones get all C frames at the frame-group kernels' speed -- the form to prefer for scenes that
 * are fetched from memory.
 *
 * Render states (tb_state_begin / tb_state_save / tb_state_load): --save-state f writes the accumulation after the render;
 * --resume f loads one and renders on to --spp frames in all -- bit-identical to the render that was never interrupted -- or, without --spp or with
 * no more than the file holds, renders nothing and just writes the picture; --add g (repeatable, applied in order after --resume) adds states of
 * adjacent frame ranges: the merge tool of an spp split; --frames A:B renders the frames [A, B) instead of --spp frames from 0, for one job of
 * such a split; --checkpoint-every N renders in calls of N frames (with --adaptive: after every call of its schedule) and saves to the
 * --save-state path after each.  A resumed render takes size, settings and time seed from the file; flags that contradict it are refused.
 * Not together with --ranks N > 1 (exit status 2): the gather moves the output surface only, rank 0 would not hold a complete state.
 *
 * --denoise (tb_denoise; takes no value): the render runs with option "aov" from its first frame on (the option resets the
 * history), the picture is denoised after the last frame -- --denoise-iterations N a-trous passes, default 5, 0 = the mean itself -- and --out
 * is written from the result: .pfm / .exr directly, .png through option "post_denoised".  --save-state still saves the raw accumulation.  With
 * --resume at least one more frame must be rendered (AOVs are not part of a state).  Not together with --ranks N > 1 (exit status 2): the ranks'
 * AOVs are not gathered.
 *
 * --denoise-guides K (tb_render_guides; implies --denoise): the render runs WITHOUT option "aov", at full speed; after the last
 * frame the first hits of the last min(K, frames held) frames of the state's range are traced again and summed, and the filter is guided by their
 * means (option "denoise_guides" = 1).  Guides are not part of a state either, but they can be traced at any time: --resume s.tbs --denoise-guides 8
 * with no frame left to render works.  --denoise-demodulate (takes no value; needs --denoise-guides): the chain runs on colour divided by the mean
 * albedo of those frames and multiplies it back at the end (option "denoise_guides" = 2).  K is 1 to 256.
 *
 * --upscale WxH (tb_upscale): the finished render is post-processed at its own size and upscaled to W x H with FSR 1 (EASU, then
 * RCAS) before --out is written: .png through the R8G8B8A8_UNORM chain, the reference's; .pfm / .exr through the RGBA32F chain -- the POST-PROCESSED
 * picture then, not the linear radiance these formats hold without --upscale.  W x H is at least the rendered size and at most 2^24 pixels.
 * --render-scale F (0 < F <= 1; the reference's m_downscaleFactor): renders at max(1, (uint32_t)((float)W * F)) x the same of H -- the truncating
 * `Width *= m_downscaleFactor` of TracerBoy.cpp:2750-2751 -- and upscales to --width x --height.  Not together with --upscale, nor with --resume (the
 * state decides the rendered size).  --fsr-sharpness S: RCAS sharpness in stops, 0 = sharpest, default 0.2 (the reference's); needs one of the two.
 * With --denoise the denoised picture is what is upscaled.  Mistakes in these three are reported before any device call (exit status 2).
 *
 * --denoise-neural FILE.tza (tb_neural_load / tb_denoise_neural): the finished render is post-processed and denoised by the OIDN
 * U-Net whose weights FILE.tza holds (OIDN's rt_ldr_alb_nrm.tza or rt_ldr.tza; the tool ships none), and --out is the network's picture: .png its
 * 8-bit conversion, .pfm / .exr the float LDR picture -- the POST-PROCESSED one, as with --upscale.  A file with 9 inputs also reads the mean albedo
 * and normals of the guide pass: the first hits of the last min(K, frames held) frames are traced again after the last frame, as --denoise-guides
 * does it, K = 8 unless --denoise-guides K says otherwise (which here does not imply --denoise); a file with 3 inputs takes no --denoise-guides.
 * The network reads the output stage's 8-bit picture (k / 255 per channel, as the reference's network does): clamped, and a NaN of the float picture
 * -- the default tonemapper gives one for a black pixel -- is 0 there, so every tonemapper works.  The tool still warns when the result holds values
 * that are not finite (a non-finite albedo or normal, or an overflow inside the network).
 * Not together with --denoise (and its --denoise-iterations / --denoise-demodulate), --upscale, --render-scale or --ranks N > 1.  Mistakes, an
 * unreadable or malformed FILE.tza among them, are reported before any device call (exit status 2).
 *
 * --upscale-neural FILE.bin (tb_sr_load / tb_upscale_neural): the finished render is post-processed at its own size and brought
 * to 2 --width x 2 --height by the reference's super-resolution network, whose weights FILE.bin holds (the reference's ML/weights.bin; the tool
 * ships none).  --out is the network's picture: .png its 8-bit conversion, .pfm / .exr the float LDR picture, as with --denoise-neural; the network
 * reads the output stage's 8-bit picture here, too.  With --denoise the denoised picture is what is upscaled.  Not together with --upscale,
 * --render-scale, --denoise-neural (the reference builds with one network or the other) or --ranks N > 1.  Mistakes, an unreadable or malformed
 * FILE.bin among them, are reported before any device call (exit status 2).
 *
 * Sample budgets (tb_set_sample_budget / tb_budget_stop_converged): three flags that decide WHERE the samples go; they combine
 * (a pixel is sampled while all of them say so).  --crop X0,Y0,X1,Y1: only the pixels of the half-open window are rendered (budget 0xffffffff inside, 0
 * outside).  --spp-map FILE (.hdr .pfm .png .tga, of the frame's size): pixel p gets (uint32_t)(saturate(red) * spp + 0.5f) samples; the calls are
 * cut at the sorted distinct counts, so every pixel gets exactly its own; more than 256 distinct counts are refused.  --noise-target T: one call of
 * min(F, spp) frames (--noise-after, default 64), then calls of C frames (--noise-chunk, default 64), each preceded by tb_budget_stop_converged(T, F):
 * a pixel stops once the estimated standard error of its mean's luminance, relative to sqrt(luma^2 + 0.01), is below T; rendering ends early when
 * no pixel is live; one line per call: frames so far, live pixels at the call's start, milliseconds.  With --adaptive P --adaptive-test call the
 * reference's skip test applies as well, at the frames of its own schedule.  Pixels that were never sampled are 0 in .pfm / .exr files (the linear
 * radiance, and --denoise's picture) and in every .png; the float output stage has 0 / 0 = NaN for them, which FSR would spread: --upscale to a
 * float file is refused with these flags.  A state holds the sums, not the budget: give the flags again with --resume; --spp-map counts from frame 0
 * and does not go with --frames.  With --ranks every rank budgets its own tiles (0 outside them) and judges the noise target on its own surface,
 * where the tiles of other ranks hold zeros: along tile borders the prefiltered variance is lower than in a one-GPU run, so those pixels may stop
 * a call earlier -- a --ranks noise-target picture is not bit for bit the one-GPU one (crop and map pictures are).  The closing line counts the
 * samples actually taken (live pixels x frames of every call; with --ranks it keeps the full frame's count).
 * Exit status 2, before any device call: a malformed or empty window, T not finite or not above 0, a map that cannot be read, any of the three
 * with --adaptive unless --adaptive-test call, with --upscale-neural or with --render-scale; a window outside the frame or a map of another size
 * likewise where --width and --height are given, otherwise as soon as the scene (or the state) has told the frame's size.
 *
 * Image-quality metrics (tb_set_reference / tb_compare / tb_run_compare).  --reference FILE (.hdr .pfm .png .tga, of the RENDERED
 * size -- with --render-scale the shrunk one): the finished accumulation's mean is compared with it on the device and the metrics are printed as one
 * JSON object on a line of its own: "frames", "surface" ("mean"), then every field of tb_compare_result, a value that is not finite as null.
 * When --denoise or --denoise-guides ran, a second line with "surface": "denoised" follows for the denoised picture.  --metrics-out FILE writes
 * these lines to FILE instead.  --metrics-every N renders in calls of N frames -- the loop of --checkpoint-every; with both, the calls are cut at
 * either grid; with --adaptive or a sample budget, at their own schedule as well -- and writes a "mean" line after each call: the convergence curve
 * without one frame read back.  The final "mean" line is not repeated when the last call's line already holds the final frame count.
 * --error-map FILE.pfm: the squared-error map of the last line written (the denoised picture's when there is one), grey, three equal channels.
 * --metrics-out, --metrics-every and --error-map need --reference; --metrics-every does not go with --ranks N > 1, for the reason the state flags do
 * not; with --ranks the final line is rank 0's, of the gathered frame.  The metrics flags change no pixel of --out.
 * --compare A B takes the place of the scene: the two image files (of one size) go through tb_run_compare, the line ("frames": 0, "surface":
 * "files") goes to standard output or to --metrics-out.  No scene, no render.
 * Exit status 2, before any device call: a reference or a file of --compare that cannot be read, A and B of different sizes, N below 1, an
 * --error-map that is no .pfm, a flag without --reference; a reference of another size than the render likewise where --width and --height are
 * given, otherwise as soon as the scene (or the state) has told the frame's size.
 *
 * The path inspector (tb_record_paths / tb_visualize_rays): --visualize-rays X,Y draws the paths of pixel (X, Y) over the
 * picture, as the reference does for the pixel SelectPixel names while m_bVisualizeRays is on.  After the render: where it ran without AOVs (no
 * --denoise) a one-frame guide pass of the last frame supplies the world positions that hide rays behind surfaces (with --denoise-guides K the
 * mean positions of its K frames do, with --denoise the last frame's AOV); the pixel's paths are traced
 * again for the frames A:B of --visualize-frames (half-open, any range), by default the last min(64, frames held); the output stage runs; the overlay
 * runs; --out is written from the overlay: .png its 8-bit picture, .pfm / .exr the float one -- the POST-PROCESSED picture, as with --upscale.
 * --visualize-width R: the cylinders' radius in world units (m_VisualizeRayWidth, default 0.01); --visualize-depth D: bounces above D are not drawn,
 * the last one below is drawn at the fraction D - bounce of its length (m_VisualizeRayDepth, default 10); --visualize-count N: only the first N
 * stored rays (m_VisualizeRayCount, default 0 = all; the buffer holds 1024).  --paths-out FILE.jsonl: one JSON object per recorded frame, on a line
 * of its own: "frame", "sum" (what the render adds to the output surface for that sample: r g b weight), "flags" (1 also on the jittered surface,
 * 2 rejected by the NaN filter, 4 not all rays stored), "num_rays" and "rays", the stored ones: "origin", "direction", "hit_t" (-1: a miss),
 * "bounce"; a value that is not finite is null.  With --denoise the denoised picture is what the rays are drawn over.
 * Exit status 2, before any device call: a malformed X,Y or A:B, R not finite or not above 0, D not finite, N negative, one of the other five
 * without --visualize-rays, any of them with --ranks N > 1, --upscale, --render-scale, --upscale-neural or --denoise-neural; a pixel outside the
 * frame likewise where --width and --height are given, otherwise as soon as the scene (or the state) has told the frame's size. */
#include "../../../include/tracerboy_hip.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <signal.h>
#include <spawn.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fail(tb_context* c, const char* what, int rc)
{
    fprintf(stderr, "tracerboy-hip: %s failed (%d): %s\n", what, rc, tb_last_error(c));
    if (c) tb_destroy(c);
    return 1;
}

extern char** environ;

/* ---- image-quality metrics: one JSON object per line ---- */
static std::string jsonNumber(double v)
{
    if (!(v - v == 0.0)) return "null"; /* NaN, +-inf */
    char b[40]; snprintf(b, sizeof b, "%.17g", v); return b;
}
static std::string metricsJson(uint32_t frames, const char* surface, const tb_compare_result& r)
{
    char head[256];
    snprintf(head, sizeof head, "{\"frames\": %u, \"surface\": \"%s\", \"pixels\": %llu, \"excluded\": %llu, \"unsampled\": %llu, \"ssim_windows\": %llu, "
        "\"ssim_windows_skipped\": %llu", frames, surface, (unsigned long long)r.pixels, (unsigned long long)r.excluded, (unsigned long long)r.unsampled,
        (unsigned long long)r.ssim_windows, (unsigned long long)r.ssim_windows_skipped);
    return std::string(head) + ", \"mse\": " + jsonNumber(r.mse) + ", \"mae\": " + jsonNumber(r.mae) + ", \"rel_mse\": " + jsonNumber(r.rel_mse) +
        ", \"max_abs\": " + jsonNumber(r.max_abs) + ", \"psnr\": " + jsonNumber(r.psnr) + ", \"ssim\": " + jsonNumber(r.ssim) + ", \"gpu_us\": " +
        jsonNumber((double)r.gpu_us) + "}";
}
/* an image file as RGBA32F (tb_decode_image); false: it cannot be read */
static bool readImage(const std::string& path, uint32_t& w, uint32_t& h, std::vector<float>& rgba)
{
    int normalized = 0, alpha = 0;
    if (tb_decode_image(path.c_str(), &w, &h, &normalized, &alpha, nullptr) || !w || !h) return false;
    rgba.resize((size_t)w * h * 4);
    return tb_decode_image(path.c_str(), &w, &h, &normalized, &alpha, rgba.data()) == 0;
}
/* --compare A B: two files through tb_run_compare; no scene */
static int compareFiles(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "--compare takes two image files\n"); return 2; }
    std::string metricsOut; int device = 0;
    for (int i = 4; i < argc; i += 2) {
        const std::string k = argv[i];
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", k.c_str()); return 2; }
        if (k == "--metrics-out") metricsOut = argv[i + 1]; else if (k == "--device") device = atoi(argv[i + 1]);
        else { fprintf(stderr, "--compare goes with --metrics-out and --device only, not %s\n", k.c_str()); return 2; }
    }
    uint32_t w[2] = {0, 0}, h[2] = {0, 0}; std::vector<float> img[2];
    for (int j = 0; j < 2; j++) if (!readImage(argv[2 + j], w[j], h[j], img[j])) {
        fprintf(stderr, "--compare %s: cannot be read as an image (.hdr .pfm .png .tga)\n", argv[2 + j]); return 2; }
    if (w[0] != w[1] || h[0] != h[1]) { fprintf(stderr, "--compare: %s is %ux%u, %s is %ux%u\n", argv[2], w[0], h[0], argv[3], w[1], h[1]); return 2; }
    tb_context* ctx = nullptr;
    int rc = tb_create(&ctx, device);
    if (rc) return fail(nullptr, "tb_create", rc);
    tb_compare_result r;
    if ((rc = tb_run_compare(ctx, w[0], h[0], img[0].data(), img[1].data(), nullptr, &r, nullptr, nullptr))) return fail(ctx, "tb_run_compare", rc);
    const std::string line = metricsJson(0, "files", r);
    if (metricsOut.empty()) printf("%s\n", line.c_str());
    else { FILE* f = fopen(metricsOut.c_str(), "w"); if (!f || fprintf(f, "%s\n", line.c_str()) < 0 || fclose(f)) { perror("tracerboy-hip: --metrics-out");
        tb_destroy(ctx); return 1; } }
    tb_destroy(ctx);
    return 0;
}

/* scene.pbrt --bake-lightmap WxH --bake-samples N [--bake-dilate P] [--device I] --out lm.pfm|.exr (tb_bake_lightmap): the
 * scene's own UVs, default settings, samples [0, N), P fill passes (default 2); the RGBA32F atlas is written as it is.  A bake is no render: every
 * other flag -- render, denoise, upscale, resume, --ranks ... -- is refused here (exit status 2), before any device call. */
static bool isBake(int argc, char** argv) { for (int i = 2; i < argc; i++) if (!strcmp(argv[i], "--bake-lightmap")) return true; return false; }
static int bakeLightmap(int argc, char** argv)
{
    std::string out; int device = 0; unsigned long long w = 0, h = 0; long long samples = 0, dilate = 2; bool sized = false;
    for (int i = 2; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k != "--bake-lightmap" && k != "--bake-samples" && k != "--bake-dilate" && k != "--out" && k != "--device") {
            fprintf(stderr, "--bake-lightmap goes with --bake-samples, --bake-dilate, --device and --out only, not %s: a bake is no render\n", k.c_str()); return 2; }
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", k.c_str()); return 2; }
        const char* v = argv[i + 1]; char* end = nullptr;
        if (k == "--bake-lightmap") { w = strtoull(v, &end, 10); const char* x = end; h = (x != v && *x == 'x') ? strtoull(x + 1, &end, 10) : 0;
            if (x == v || *x != 'x' || end == x + 1 || *end || w < 1 || h < 1 || w > 8192 || h > 8192) { fprintf(stderr, "--bake-lightmap is WxH, both 1 to 8192\n"); return 2; }
            sized = true; }
        else if (k == "--bake-samples") { samples = strtoll(v, &end, 10);
            if (end == v || *end || samples < 1 || samples > (1ll << 24)) { fprintf(stderr, "--bake-samples is 1 to 2^24\n"); return 2; } }
        else if (k == "--bake-dilate") { dilate = strtoll(v, &end, 10);
            if (end == v || *end || dilate < 0 || dilate > 16) { fprintf(stderr, "--bake-dilate is 0 to 16\n"); return 2; } }
        else if (k == "--out") out = v; else device = atoi(v);
    }
    if (!sized || samples < 1) { fprintf(stderr, "--bake-lightmap WxH needs --bake-samples N\n"); return 2; }
    const bool floatFile = out.size() >= 4 && (out.compare(out.size() - 4, 4, ".pfm") == 0 || out.compare(out.size() - 4, 4, ".exr") == 0);
    if (!floatFile) { fprintf(stderr, "--bake-lightmap writes --out lm.pfm or lm.exr: the atlas is linear RGBA32F\n"); return 2; }
    tb_context* ctx = nullptr;
    int rc = tb_create(&ctx, device);
    if (rc) return fail(nullptr, "tb_create", rc);
    if ((rc = tb_load_scene(ctx, argv[1]))) return fail(ctx, "tb_load_scene", rc);
    std::vector<float> rgba((size_t)w * h * 4);
    const tb_bake_call call = {(uint32_t)w, (uint32_t)h, 0u, (uint32_t)samples, (uint32_t)dilate, 0u};
    if ((rc = tb_bake_lightmap(ctx, nullptr, 0.0f, &call, nullptr, rgba.data()))) return fail(ctx, "tb_bake_lightmap", rc);
    if ((rc = tb_write_image_f32(out.c_str(), (uint32_t)w, (uint32_t)h, rgba.data()))) return fail(ctx, "tb_write_image_f32", rc);
    printf("{\"bake\": \"%llux%llu\", \"samples\": %lld, \"dilate\": %lld, \"covered\": %lld, \"raster_us\": %lld, \"trace_us\": %lld, \"finish_us\": %lld}\n", w, h, samples,
        dilate, (long long)tb_get_option(ctx, "last_bake_covered"), (long long)tb_get_option(ctx, "last_bake_raster_us"),
        (long long)tb_get_option(ctx, "last_bake_trace_us"), (long long)tb_get_option(ctx, "last_bake_finish_us"));
    tb_destroy(ctx);
    return 0;
}

/* scene.pbrt --bake-probes NXxNYxNZ [--probe-bounds x0,y0,z0,x1,y1,z1] [--probe-res M] [--probe-samples S] [--device I] --out probes.jsonl (DESIGN.md
 * section 25; tb_bake_probes): NX x NY x NZ probes at the centres of equal cells of the bounds (default: the scene's box), an M x M map each (default
 * 16), samples [0, S) (default 64), default settings; one JSON line per probe: its number, position, 27 coefficients, five statistics.  A bake is no
 * render: every other flag is refused here (exit status 2), before any device call. */
static bool isProbeBake(int argc, char** argv) { for (int i = 2; i < argc; i++) if (!strcmp(argv[i], "--bake-probes")) return true; return false; }
static int bakeProbes(int argc, char** argv)
{
    std::string out; int device = 0; unsigned long long count[3] = {0, 0, 0}; long long res = 16, samples = 64; double bounds[6]; bool sized = false, bounded = false;
    for (int i = 2; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k != "--bake-probes" && k != "--probe-bounds" && k != "--probe-res" && k != "--probe-samples" && k != "--out" && k != "--device") {
            fprintf(stderr, "--bake-probes goes with --probe-bounds, --probe-res, --probe-samples, --device and --out only, not %s: a bake is no render\n", k.c_str()); return 2; }
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", k.c_str()); return 2; }
        const char* v = argv[i + 1]; char* end = nullptr;
        if (k == "--bake-probes") {
            const char* at = v; bool ok = true;
            for (int a = 0; a < 3 && ok; a++) {
                ok = *at >= '0' && *at <= '9';
                if (ok) { count[a] = strtoull(at, &end, 10); ok = count[a] >= 1 && count[a] <= (1ull << 24) && *end == (a < 2 ? 'x' : '\0'); at = end + 1; }
            }
            if (!ok || count[0] * count[1] * count[2] > (1ull << 24)) { fprintf(stderr, "--bake-probes is NXxNYxNZ, each at least 1, at most 2^24 probes\n"); return 2; }
            sized = true; }
        else if (k == "--probe-bounds") {
            const char* at = v; bool ok = true;
            for (int a = 0; a < 6 && ok; a++) { bounds[a] = strtod(at, &end); ok = end != at && std::isfinite(bounds[a]) && *end == (a < 5 ? ',' : '\0'); at = end + 1; }
            if (!ok) { fprintf(stderr, "--probe-bounds is x0,y0,z0,x1,y1,z1, six finite numbers\n"); return 2; }
            bounded = true; }
        else if (k == "--probe-res") { res = strtoll(v, &end, 10);
            if (end == v || *end || res < 2 || res > 64) { fprintf(stderr, "--probe-res is 2 to 64\n"); return 2; } }
        else if (k == "--probe-samples") { samples = strtoll(v, &end, 10);
            if (end == v || *end || samples < 1 || samples > (1ll << 24)) { fprintf(stderr, "--probe-samples is 1 to 2^24\n"); return 2; } }
        else if (k == "--out") out = v; else device = atoi(v);
    }
    if (!sized) { fprintf(stderr, "--bake-probes needs NXxNYxNZ\n"); return 2; }
    const uint64_t n = count[0] * count[1] * count[2];
    if (n * (uint64_t)(res * res) > (1ull << 31)) { fprintf(stderr, "--bake-probes: more than 2^31 rays\n"); return 2; }
    if (out.size() < 7 || out.compare(out.size() - 6, 6, ".jsonl") != 0) { fprintf(stderr, "--bake-probes writes --out probes.jsonl\n"); return 2; }
    tb_context* ctx = nullptr;
    int rc = tb_create(&ctx, device);
    if (rc) return fail(nullptr, "tb_create", rc);
    if ((rc = tb_load_scene(ctx, argv[1]))) return fail(ctx, "tb_load_scene", rc);
    if (!bounded) { tb_scene_info info; if ((rc = tb_scene_info_get(ctx, &info))) return fail(ctx, "tb_scene_info_get", rc);
        for (int a = 0; a < 3; a++) { bounds[a] = info.sceneMin[a]; bounds[3 + a] = info.sceneMax[a]; } }
    std::vector<float> positions(3 * n); std::vector<TbProbe> probes(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t at[3] = {i % count[0], (i / count[0]) % count[1], i / (count[0] * count[1])};
        for (int a = 0; a < 3; a++) positions[3 * i + a] = (float)(bounds[a] + ((double)at[a] + 0.5) * (bounds[3 + a] - bounds[a]) / (double)count[a]);
    }
    const tb_probe_call call = {(uint32_t)n, 0u, (uint32_t)res, 0u, (uint32_t)samples, 0u};
    if ((rc = tb_bake_probes(ctx, nullptr, 0.0f, &call, positions.data(), probes.data()))) return fail(ctx, "tb_bake_probes", rc);
    FILE* f = fopen(out.c_str(), "w");
    if (!f) { fprintf(stderr, "cannot open %s\n", out.c_str()); tb_destroy(ctx); return 1; }
    for (uint64_t i = 0; i < n; i++) {
        const TbProbe& p = probes[i];
        fprintf(f, "{\"probe\": %llu, \"position\": [%.9g, %.9g, %.9g], \"sh\": [", (unsigned long long)i, positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]);
        for (int k = 0; k < 27; k++) fprintf(f, "%s%.9g", k ? ", " : "", p.SH[k]);
        fprintf(f, "], \"weight\": %.9g, \"hits\": %.9g, \"backfaces\": %.9g, \"min_distance\": %.9g, \"mean_distance\": %.9g}\n", p.Weight, p.Hits, p.Backfaces,
            p.MinDistance, p.MeanDistance);
    }
    if (fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", out.c_str()); tb_destroy(ctx); return 1; }
    printf("{\"probes\": \"%llux%llux%llu\", \"resolution\": %lld, \"samples\": %lld, \"batches\": %lld, \"rays_us\": %lld, \"trace_us\": %lld, \"hits_us\": %lld, \"project_us\": %lld}\n",
        count[0], count[1], count[2], res, samples, (long long)tb_get_option(ctx, "last_probes_batches"), (long long)tb_get_option(ctx, "last_probes_rays_us"),
        (long long)tb_get_option(ctx, "last_probes_trace_us"), (long long)tb_get_option(ctx, "last_probes_hits_us"), (long long)tb_get_option(ctx, "last_probes_project_us"));
    tb_destroy(ctx);
    return 0;
}

/* ---- RCCL, loaded at run time: the handful of entry points the gather needs (rccl.h) ---- */
struct RcclId { char internal[128]; };                 /* ncclUniqueId */
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclId*) = nullptr;
    int (*CommInitRank)(void** comm, int nranks, RcclId id, int rank) = nullptr;
    int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int dtype, int peer, void* comm, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int dtype, int peer, void* comm, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load()
    {
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!lib) { fprintf(stderr, "tracerboy-hip: cannot load librccl: %s\n", dlerror()); return false; }
#define SYM(field, name) if (!((*(void**)&field) = dlsym(lib, name))) { fprintf(stderr, "tracerboy-hip: librccl lacks %s\n", name); return false; }
        SYM(GetUniqueId, "ncclGetUniqueId") SYM(CommInitRank, "ncclCommInitRank") SYM(GroupStart, "ncclGroupStart") SYM(GroupEnd, "ncclGroupEnd")
        SYM(Send, "ncclSend") SYM(Recv, "ncclRecv") SYM(CommDestroy, "ncclCommDestroy") SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
        return true;
    }
};
static const int kNcclFloat = 7; /* ncclFloat32 */

/* start `world` copies of this program, one per rank, and wait for them; nothing here touches HIP */
static int spawnRanks(int argc, char** argv, int world)
{
    /* The RCCL unique id travels from rank 0 to the others through a file in a directory only this user can enter (mkdtemp: mode
     * 0700, unpredictable name): nobody else can pre-create the file, plant a symlink where rank 0 writes, or read the id. */
    char idDir[] = "/tmp/tracerboy-hip-rccl-XXXXXX";
    if (!mkdtemp(idDir)) { perror("tracerboy-hip: mkdtemp"); return 1; }
    const std::string idFile = std::string(idDir) + "/id", idTmp = idFile + ".tmp";
    auto cleanup = [&]() { unlink(idFile.c_str()); unlink(idTmp.c_str()); rmdir(idDir); };
    std::vector<pid_t> kids;
    for (int r = 0; r < world; r++) {
        std::vector<std::string> envs;
        for (char** e = environ; *e; e++) if (strncmp(*e, "TB_CLI_", 7)) envs.push_back(*e);
        envs.push_back("TB_CLI_RANK=" + std::to_string(r)); envs.push_back("TB_CLI_WORLD=" + std::to_string(world)); envs.push_back("TB_CLI_ID_FILE=" + idFile);
        bool ipc = false; for (const std::string& e : envs) ipc |= e.rfind("HSA_ENABLE_IPC_MODE_LEGACY=", 0) == 0;
        if (!ipc) envs.push_back("HSA_ENABLE_IPC_MODE_LEGACY=0"); /* this pool's driver only supports dmabuf IPC */
        std::vector<char*> envp; for (std::string& e : envs) envp.push_back(&e[0]); envp.push_back(nullptr);
        pid_t pid = 0;
        if (posix_spawn(&pid, "/proc/self/exe", nullptr, nullptr, argv, envp.data()) != 0) {
            perror("tracerboy-hip: posix_spawn");
            for (pid_t k : kids) kill(k, SIGTERM);
            for (size_t i = 0; i < kids.size(); i++) { int st = 0; (void)waitpid(kids[i], &st, 0); }
            cleanup(); return 1;
        }
        kids.push_back(pid);
    }
    /* a rank that fails (no such device, scene error ...) would leave the others waiting in the communicator forever: the first
     * non-zero exit ends the ranks still running, and ITS status is what the tool returns (the others then die of the SIGTERM) */
    int first = 0;
    while (!kids.empty()) {
        int st = 0; const pid_t k = waitpid(-1, &st, 0);
        if (k < 0) break;
        auto it = std::find(kids.begin(), kids.end(), k);
        if (it == kids.end()) continue;                 /* not one of ours */
        kids.erase(it);                                 /* reaped: its pid may be reused, never signal it again */
        const int rc = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
        if (rc != 0 && first == 0) { first = rc; for (pid_t o : kids) kill(o, SIGTERM); }
    }
    cleanup();
    (void)argc;
    return first;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr,
        "usage: tracerboy-hip scene.pbrt [--width W --height H --spp N --depth D --seed-time T --device I --builder lbvh|sah|lbvh-gpu|treelets|treelets-gpu --blue-noise 0|1 --tonemap 0..7 --exposure E|auto --out f.png|f.pfm|f.exr --ranks N --adaptive P --adaptive-after F --adaptive-chunk C --adaptive-test frame|call --save-state f.tbs --resume f.tbs --add g.tbs --frames A:B --checkpoint-every N --denoise --denoise-iterations N --denoise-guides K --denoise-demodulate --upscale WxH --render-scale F --fsr-sharpness S --denoise-neural f.tza --upscale-neural f.bin --crop X0,Y0,X1,Y1 --spp-map FILE --noise-target T --noise-after F --noise-chunk C --reference FILE --metrics-out FILE --metrics-every N --error-map f.pfm --visualize-rays X,Y --visualize-frames A:B --visualize-width R --visualize-depth D --visualize-count N --paths-out f.jsonl]\n       tracerboy-hip scene.pbrt --bake-probes NXxNYxNZ [--probe-bounds x0,y0,z0,x1,y1,z1 --probe-res M --probe-samples S --device I] --out probes.jsonl\n       tracerboy-hip --compare A B [--metrics-out FILE --device I]\n"); return 2; }
    if (!strcmp(argv[1], "--compare")) return compareFiles(argc, argv);
    if (isProbeBake(argc, argv)) return bakeProbes(argc, argv);
    if (isBake(argc, argv)) return bakeLightmap(argc, argv);
    std::string scene = argv[1], out = "frame.png";
    tb_post_settings post; tb_default_post_settings(&post);
    uint32_t W = 0, H = 0, spp = 64; int depth = -1, device = 0, builder = 0, blue = -1, ranks = 1; float t = 0.0f;
    float adaptive = -1.0f; long long adaptiveAfter = 1024, adaptiveChunk = 64; int adaptiveTest = 0;
    std::string saveState, resume; std::vector<std::string> adds; long long frameA = -1, frameB = -1, checkpointEvery = 0;
    bool sppSet = false, timeSet = false, denoise = false, demodulate = false; long long denoiseIterations = -1, denoiseGuides = 0;
    std::string neural, neuralUp; bool denoiseFlag = false; /* --denoise itself, not what --denoise-guides implies */
    long long crop[4] = {0, 0, 0, 0}; bool cropSet = false; std::string sppMap; float noiseTarget = 0.0f; bool noiseSet = false;
    long long noiseAfter = 64, noiseChunk = 64;
    std::string reference, metricsOut, errorMap; long long metricsEvery = 0; bool metricsEverySet = false;
    bool visSet = false, visOther = false; long long visX = 0, visY = 0, visA = -1, visB = -1; std::string pathsOut; /* the path inspector */
    tb_visualize_settings vis; tb_default_visualize_settings(&vis);
    uint32_t upW = 0, upH = 0; float renderScale = 0.0f, fsrSharpness = -1.0f; bool upscaleSet = false, renderScaleSet = false, sharpnessSet = false;
    for (int i = 2; i < argc; i += 2) {
        std::string k = argv[i];
        if (k == "--denoise") { denoise = true; denoiseFlag = true; i--; continue; } /* the flags without a value */
        if (k == "--denoise-demodulate") { demodulate = true; i--; continue; }
        if (i + 1 >= argc) break;
        const char* v = argv[i + 1];
        if (k == "--width") W = (uint32_t)atoi(v); else if (k == "--height") H = (uint32_t)atoi(v); else if (k == "--spp") { spp = (uint32_t)atoi(v); sppSet = true; }
        else if (k == "--depth") depth = atoi(v); else if (k == "--seed-time") { t = (float)atof(v); timeSet = true; } else if (k == "--device") device = atoi(v);
        else if (k == "--builder") builder = !strcmp(v, "sah") ? 1 : !strcmp(v, "lbvh-gpu") ? 2 : !strcmp(v, "treelets") ? 3 : !strcmp(v,
            "treelets-gpu") ? 4 : 0; /* tb_set_option "bvh_builder" */ else if (k == "--blue-noise") blue = atoi(v); else if (k == "--out") out = v;
            else if (k == "--ranks") ranks = atoi(v);
        else if (k == "--adaptive") adaptive = (float)atof(v); else if (k == "--adaptive-after") adaptiveAfter = atoll(v);
        else if (k == "--adaptive-chunk") adaptiveChunk = atoll(v);
        else if (k == "--adaptive-test") { if (!strcmp(v, "call")) adaptiveTest = 1; else if (!strcmp(v, "frame")) adaptiveTest = 0;
            else { fprintf(stderr, "--adaptive-test is frame or call\n"); return 2; } }
        else if (k == "--save-state") saveState = v; else if (k == "--resume") resume = v; else if (k == "--add") adds.push_back(v);
        else if (k == "--checkpoint-every") checkpointEvery = atoll(v);
        else if (k == "--denoise-iterations") { denoiseIterations = atoll(v);
            if (denoiseIterations < 0 || denoiseIterations > 10) { fprintf(stderr, "--denoise-iterations is 0 to 10\n"); return 2; } }
        else if (k == "--denoise-guides") { denoiseGuides = atoll(v); denoise = true;
            if (denoiseGuides < 1 || denoiseGuides > 256) { fprintf(stderr, "--denoise-guides is 1 to 256\n"); return 2; } }
        else if (k == "--frames") { char* end = nullptr; frameA = strtoll(v, &end, 10); frameB = end && *end == ':' ? strtoll(end + 1, &end, 10) : -1;
            if (frameA < 0 || frameB < frameA || frameB > 0xffffffffll || !end || *end) { fprintf(stderr, "--frames is A:B with 0 <= A <= B\n"); return 2; } }
        else if (k == "--upscale") { char* end = nullptr; const unsigned long long uw = strtoull(v, &end, 10);
            const unsigned long long uh = end && end != v && *end == 'x' && end[1] >= '0' && end[1] <= '9' ? strtoull(end + 1, &end, 10) : 0;
            if (!uw || !uh || !end || *end || uw > (1ull << 24) || uh > (1ull << 24) || uw * uh > (1ull << 24)) {
                fprintf(stderr, "--upscale is WxH, both at least 1, at most 2^24 pixels\n"); return 2; }
            upW = (uint32_t)uw; upH = (uint32_t)uh; upscaleSet = true; }
        else if (k == "--render-scale") { char* end = nullptr; renderScale = strtof(v, &end); renderScaleSet = true;
            if (end == v || *end || !(renderScale > 0.0f) || !(renderScale <= 1.0f)) { fprintf(stderr, "--render-scale is above 0 and at most 1\n"); return 2; } }
        else if (k == "--fsr-sharpness") { char* end = nullptr; fsrSharpness = strtof(v, &end); sharpnessSet = true;
            if (end == v || *end || !(fsrSharpness >= 0.0f) || !(fsrSharpness < 1e30f)) { fprintf(stderr, "--fsr-sharpness is a finite number of stops, 0 or more\n"); return 2; } }
        else if (k == "--crop") { const char* p = v; char* end = nullptr; cropSet = true;
            for (int j = 0; j < 4 && p; j++) { crop[j] = strtoll(p, &end, 10); p = end != p && *end == (j < 3 ? ',' : '\0') && crop[j] >= 0 && crop[j] <= 16384 ? end + 1 : nullptr; }
            if (!p || crop[2] <= crop[0] || crop[3] <= crop[1]) { fprintf(stderr, "--crop is X0,Y0,X1,Y1 with 0 <= X0 < X1 and 0 <= Y0 < Y1 (half-open)\n"); return 2; } }
        else if (k == "--spp-map") sppMap = v;
        else if (k == "--noise-target") { char* end = nullptr; noiseTarget = strtof(v, &end); noiseSet = true;
            if (end == v || *end || !(noiseTarget > 0.0f) || !(noiseTarget < 3.0e38f)) { fprintf(stderr, "--noise-target is a finite relative error above 0\n"); return 2; } }
        else if (k == "--noise-after") noiseAfter = atoll(v); else if (k == "--noise-chunk") noiseChunk = atoll(v);
        else if (k == "--denoise-neural") neural = v;
        else if (k == "--reference") reference = v; else if (k == "--metrics-out") metricsOut = v; else if (k == "--error-map") errorMap = v;
        else if (k == "--metrics-every") { metricsEvery = atoll(v); metricsEverySet = true; }
        else if (k == "--upscale-neural") neuralUp = v;
        else if (k == "--visualize-rays") { char* end = nullptr; visX = strtoll(v, &end, 10); const char* second = end != v && *end == ',' ? end + 1 : nullptr;
            if (second) visY = strtoll(second, &end, 10);
            if (!second || end == second || *end || visX < 0 || visY < 0 || visX >= 16384 || visY >= 16384) { fprintf(stderr, "--visualize-rays is X,Y: a pixel of the frame\n"); return 2; }
            visSet = true; }
        else if (k == "--visualize-frames") { char* end = nullptr; visA = strtoll(v, &end, 10); visB = end && end != v && *end == ':' ? strtoll(end + 1, &end, 10) : -1;
            visOther = true;
            if (visA < 0 || visB <= visA || visB > 0xffffffffll || !end || *end) { fprintf(stderr, "--visualize-frames is A:B with 0 <= A < B\n"); return 2; } }
        else if (k == "--visualize-width") { char* end = nullptr; vis.RayWidth = strtof(v, &end); visOther = true;
            if (end == v || *end || !(vis.RayWidth > 0.0f) || !(vis.RayWidth < 3.0e38f)) { fprintf(stderr, "--visualize-width is a finite radius above 0\n"); return 2; } }
        else if (k == "--visualize-depth") { char* end = nullptr; vis.RayDepth = strtof(v, &end); visOther = true;
            if (end == v || *end || !(vis.RayDepth - vis.RayDepth == 0.0f)) { fprintf(stderr, "--visualize-depth is a finite number of bounces\n"); return 2; } }
        else if (k == "--visualize-count") { char* end = nullptr; const long long n = strtoll(v, &end, 10); visOther = true;
            if (end == v || *end || n < 0 || n > 0x7fffffffll) { fprintf(stderr, "--visualize-count is 0 (all) or a number of rays\n"); return 2; }
            vis.RayCount = (int32_t)n; }
        else if (k == "--paths-out") { pathsOut = v; visOther = true; }
        else if (k == "--tonemap") post.TonemapType = (uint32_t)atoi(v);
        else if (k == "--exposure") { if (!strcmp(v, "auto")) post.EnableAutoExposure = 1; else { post.EnableAutoExposure = 0;
            post.ExposureMultiplier = (float)atof(v); } }
        else { fprintf(stderr, "unknown option %s\n", k.c_str()); return 2; }
    }
    /* multi-GPU: the parent only starts the ranks; a rank knows itself from the environment */
    const char* envRank = getenv("TB_CLI_RANK");
    const bool forceRccl = getenv("TB_CLI_FORCE_RCCL") && atoi(getenv("TB_CLI_FORCE_RCCL")) != 0;
    if (ranks < 1) { fprintf(stderr, "--ranks must be at least 1\n"); return 2; }
    if (adaptiveAfter < 0 || adaptiveChunk < 1) { fprintf(stderr, "--adaptive-after must not be negative, --adaptive-chunk must be at least 1\n"); return 2; }
    /* sample budgets */
    const bool budgeted = cropSet || !sppMap.empty() || noiseSet;
    if (noiseAfter < 0 || noiseAfter > 0xffffffffll || noiseChunk < 1) { fprintf(stderr, "--noise-after must not be negative, --noise-chunk must be at least 1\n"); return 2; }
    if (budgeted && adaptive >= 0.0f && adaptiveTest != 1) { fprintf(stderr,
        "--crop, --spp-map and --noise-target go with --adaptive only as --adaptive-test call: a budget is applied once per call\n"); return 2; }
    if (budgeted && !neuralUp.empty()) { fprintf(stderr, "--crop, --spp-map and --noise-target do not go with --upscale-neural\n"); return 2; }
    if (!sppMap.empty() && frameA >= 0) { fprintf(stderr,
        "--spp-map does not go with --frames: its counts are samples from frame 0 on\n"); return 2; }
    if (budgeted && upscaleSet && !(out.size() >= 4 && out.compare(out.size() - 4, 4, ".png") == 0)) { fprintf(stderr,
        "--crop, --spp-map and --noise-target go with --upscale only for a .png: the float chain would spread the NaN of never-sampled pixels\n"); return 2; }
    if (budgeted && renderScaleSet) { fprintf(stderr, "--crop, --spp-map and --noise-target do not go with --render-scale: they are given in rendered pixels\n"); return 2; }
    if (!neural.empty()) {
        if (denoiseFlag || denoiseIterations >= 0 || demodulate) { fprintf(stderr,
            "--denoise-neural does not go with --denoise, --denoise-iterations or --denoise-demodulate: the network stands in place of the a-trous filter\n"); return 2; }
        if (upscaleSet || renderScaleSet) { fprintf(stderr, "--denoise-neural does not go with --upscale or --render-scale\n"); return 2; }
        if (ranks > 1) { fprintf(stderr, "--denoise-neural does not go with --ranks: the ranks' guide surfaces are not gathered\n"); return 2; }
        tb_nn_info nn; char err[512] = "";
        if (tb_nn_weights_info(neural.c_str(), &nn, err, sizeof err)) { fprintf(stderr, "--denoise-neural %s: %s\n", neural.c_str(), err); return 2; }
        if (nn.in_channels == 3u && denoiseGuides) { fprintf(stderr, "--denoise-neural %s: its weights have 3 inputs and read no guides: leave --denoise-guides out\n",
            neural.c_str()); return 2; }
        if (nn.in_channels == 9u && !denoiseGuides) denoiseGuides = 8;
        denoise = false; /* --denoise-guides K: the network's guides, not the filter's */
    }
    if (!neuralUp.empty()) {
        if (upscaleSet || renderScaleSet) { fprintf(stderr, "--upscale-neural does not go with --upscale or --render-scale: the network is the upscaler\n"); return 2; }
        if (!neural.empty()) { fprintf(stderr, "--upscale-neural does not go with --denoise-neural: the two networks are not chained\n"); return 2; }
        if (ranks > 1) { fprintf(stderr, "--upscale-neural does not go with --ranks: the network does not run across a device group\n"); return 2; }
        tb_sr_info sr; char err[512] = "";
        if (tb_sr_weights_info(neuralUp.c_str(), &sr, err, sizeof err)) { fprintf(stderr, "--upscale-neural %s: %s\n", neuralUp.c_str(), err); return 2; }
    }
    /* the path inspector */
    if (visOther && !visSet) { fprintf(stderr,
        "--visualize-frames, --visualize-width, --visualize-depth, --visualize-count and --paths-out need --visualize-rays X,Y: the pixel whose paths are drawn\n"); return 2; }
    if (visSet && (ranks > 1 || upscaleSet || renderScaleSet || !neuralUp.empty() || !neural.empty())) { fprintf(stderr,
        "--visualize-rays does not go with --ranks, --upscale, --render-scale, --upscale-neural or --denoise-neural: the rays are drawn over the output stage's picture of one device\n");
        return 2; }
    auto pixelFits = [&](uint32_t fw, uint32_t fh) {
        if (visSet && (visX >= (long long)fw || visY >= (long long)fh)) {
            fprintf(stderr, "--visualize-rays %lld,%lld lies outside the %ux%u frame\n", visX, visY, fw, fh); return false; }
        return true;
    };
    if (W && H && resume.empty() && !pixelFits(W, H)) return 2;
    /* image-quality metrics */
    if (reference.empty() && (!metricsOut.empty() || metricsEverySet || !errorMap.empty())) { fprintf(stderr,
        "--metrics-out, --metrics-every and --error-map need --reference FILE: the metrics are those against a reference picture\n"); return 2; }
    if (metricsEverySet && metricsEvery < 1) { fprintf(stderr, "--metrics-every N needs N >= 1\n"); return 2; }
    if (metricsEvery > 0 && ranks > 1) { fprintf(stderr,
        "--metrics-every does not go with --ranks: the gather moves the output surface after the last frame only, no rank holds the frame in between\n"); return 2; }
    if (!errorMap.empty() && !(errorMap.size() >= 4 && errorMap.compare(errorMap.size() - 4, 4, ".pfm") == 0)) { fprintf(stderr, "--error-map writes a .pfm file\n"); return 2; }
    std::vector<float> refRgba; uint32_t refW = 0, refH = 0;
    if (!reference.empty() && !readImage(reference, refW, refH, refRgba)) { /* host only: decoded before any device call */
        fprintf(stderr, "--reference %s: cannot be read as an image (.hdr .pfm .png .tga)\n", reference.c_str()); return 2; }
    auto referenceFits = [&](uint32_t fw, uint32_t fh) {
        if (!reference.empty() && (refW != fw || refH != fh)) {
            fprintf(stderr, "--reference %s is %ux%u, the render %ux%u\n", reference.c_str(), refW, refH, fw, fh); return false; }
        return true;
    };
    const bool states = !saveState.empty() || !resume.empty() || !adds.empty() || frameA >= 0 || checkpointEvery != 0;
    if (states && ranks > 1) { fprintf(stderr,
        "--save-state, --resume, --add, --frames and --checkpoint-every do not go with --ranks: the gather moves the output surface only\n"); return 2; }
    if (denoise && ranks > 1) { fprintf(stderr, "--denoise does not go with --ranks: the ranks' AOVs are not gathered\n"); return 2; }
    if (demodulate && !denoiseGuides) { fprintf(stderr, "--denoise-demodulate needs --denoise-guides K\n"); return 2; }
    if (denoiseIterations >= 0 && !denoise) { fprintf(stderr, "--denoise-iterations needs --denoise\n"); return 2; }
    if (checkpointEvery < 0 || (checkpointEvery > 0 && saveState.empty())) { fprintf(stderr, "--checkpoint-every N needs N >= 1 and --save-state\n"); return 2; }
    if (frameA >= 0 && (sppSet || !resume.empty())) { fprintf(stderr, "--frames A:B stands in place of --spp and starts its own accumulation (no --resume)\n"); return 2; }
    if (!adds.empty() && resume.empty()) { fprintf(stderr, "--add merges into the state --resume loads\n"); return 2; }
    if (upscaleSet && renderScaleSet) { fprintf(stderr, "--upscale and --render-scale do not go together: --render-scale upscales to --width x --height\n"); return 2; }
    if (sharpnessSet && !upscaleSet && !renderScaleSet) { fprintf(stderr, "--fsr-sharpness needs --upscale or --render-scale\n"); return 2; }
    if (renderScaleSet && !resume.empty()) { fprintf(stderr, "--render-scale does not go with --resume: the state decides the rendered size\n"); return 2; }
    std::vector<float> mapRgba; uint32_t mapW = 0, mapH = 0;
    if (!sppMap.empty()) { /* host only: decoded before any device call */
        int normalized = 0, alpha = 0;
        if (tb_decode_image(sppMap.c_str(), &mapW, &mapH, &normalized, &alpha, nullptr) || !mapW || !mapH) {
            fprintf(stderr, "--spp-map %s: cannot be read as an image (.hdr .pfm .png .tga)\n", sppMap.c_str()); return 2; }
        mapRgba.resize((size_t)mapW * mapH * 4);
        if (tb_decode_image(sppMap.c_str(), &mapW, &mapH, &normalized, &alpha, mapRgba.data())) {
            fprintf(stderr, "--spp-map %s: cannot be read as an image (.hdr .pfm .png .tga)\n", sppMap.c_str()); return 2; }
    }
    std::vector<uint32_t> mapBudget, mapCuts; /* per pixel; its sorted distinct values */
    if (!sppMap.empty()) {
        mapBudget.resize((size_t)mapW * mapH);
        for (size_t i = 0; i < mapBudget.size(); i++) { const float red = mapRgba[4 * i], sat = red > 0.0f ? (red < 1.0f ? red : 1.0f) : 0.0f; /* (NaN: 0) */
            mapBudget[i] = (uint32_t)(sat * (float)spp + 0.5f); }
        mapCuts = mapBudget; std::sort(mapCuts.begin(), mapCuts.end()); mapCuts.erase(std::unique(mapCuts.begin(), mapCuts.end()), mapCuts.end());
        if (mapCuts.size() > 256) { fprintf(stderr, "--spp-map %s holds %zu distinct sample counts: at most 256 (every count is a call of its own)\n",
            sppMap.c_str(), mapCuts.size()); return 2; }
    }
    /* the frame's size against window and map: exit status 2; before any device call where --width and --height say it */
    auto budgetFits = [&](uint32_t fw, uint32_t fh) {
        if (cropSet && (crop[2] > (long long)fw || crop[3] > (long long)fh)) {
            fprintf(stderr, "--crop %lld,%lld,%lld,%lld lies outside the %ux%u frame\n", crop[0], crop[1], crop[2], crop[3], fw, fh); return false; }
        if (!sppMap.empty() && (mapW != fw || mapH != fh)) {
            fprintf(stderr, "--spp-map %s is %ux%u, the frame %ux%u\n", sppMap.c_str(), mapW, mapH, fw, fh); return false; }
        return true;
    };
    if (budgeted && W && H && resume.empty() && !budgetFits(W, H)) return 2;
    if (W && H && resume.empty() && !renderScaleSet && !referenceFits(W, H)) return 2;
    if (ranks > 1 && !envRank) return spawnRanks(argc, argv, ranks);
    if (envRank && (!getenv("TB_CLI_WORLD") || atoi(getenv("TB_CLI_WORLD")) < 1 || atoi(envRank) < 0 || atoi(envRank) >= atoi(getenv("TB_CLI_WORLD")) ||
                    (atoi(getenv("TB_CLI_WORLD")) > 1 && !getenv("TB_CLI_ID_FILE")))) {
        fprintf(stderr,
            "tracerboy-hip: TB_CLI_RANK needs TB_CLI_WORLD (rank < world) and, for more than one rank, TB_CLI_ID_FILE -- these are set by --ranks, not by hand\n"); return 2;
    }
    const int rank = envRank ? atoi(envRank) : 0, world = envRank ? atoi(getenv("TB_CLI_WORLD")) : 1;
    if (world > 1) device = rank; /* one process per GPU */
    tb_context* ctx = nullptr;
    int rc = tb_create(&ctx, device);
    if (rc) return fail(nullptr, "tb_create", rc);
    tb_set_option(ctx, "bvh_builder", builder);
    if (denoise && !denoiseGuides && (rc = tb_set_option(ctx, "aov", 1))) return fail(ctx, "tb_set_option", rc); /* before the first frame: the option resets the history */
    auto t0 = std::chrono::steady_clock::now();
    if ((rc = tb_load_scene(ctx, scene.c_str()))) return fail(ctx, "tb_load_scene", rc);
    double loadS = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    tb_scene_info info; tb_scene_info_get(ctx, &info);
    const uint32_t argWidth = W, argHeight = H;
    if (!W) W = info.filmWidth ? info.filmWidth : 1920;
    if (!H) H = info.filmHeight ? info.filmHeight : 1080;
    if (renderScaleSet) { /* m_downscaleFactor: the picture keeps its size, the render surfaces shrink (TracerBoy.cpp:2750-2751) */
        upW = W; upH = H;
        W = std::max(1u, (uint32_t)((float)W * renderScale)); H = std::max(1u, (uint32_t)((float)H * renderScale));
    }
    tb_output_settings s; tb_default_output_settings(&s);
    if (depth >= 0) s.MaxBounces = depth;
    if (blue >= 0) s.EnableBlueNoise = (uint32_t)blue;
    const uint32_t TILE = 64;
    if (world > 1 && (rc = tb_set_tile_assignment(ctx, (uint32_t)rank, (uint32_t)world, TILE, TILE))) return fail(ctx, "tb_set_tile_assignment", rc);
    auto r0 = std::chrono::steady_clock::now();
    float ms = 0.0f;
    if (adaptive >= 0.0f) { /* before a state is loaded: the file's values of these options must be the context's */
        s.ConvergencePercentage = adaptive;
        if ((rc = tb_set_option(ctx, "adaptive", 1)) || (rc = tb_set_option(ctx, "adaptive_min_frames", adaptiveAfter)) ||
            (rc = tb_set_option(ctx, "adaptive_test", adaptiveTest))) return fail(ctx, "tb_set_option", rc);
    }
    /* `done`: the index of the next frame; the render goes on to frame `target` */
    uint32_t done = 0, target = spp;
    if (!resume.empty()) {
        if ((rc = tb_state_load(ctx, resume.c_str(), TB_STATE_REPLACE))) return fail(ctx, "tb_state_load", rc);
        for (const std::string& a : adds) if ((rc = tb_state_load(ctx, a.c_str(), TB_STATE_ADD))) return fail(ctx, ("tb_state_load (--add " + a + ")").c_str(), rc);
        tb_state_info held; char err[256] = "";
        if ((rc = tb_state_info_read(resume.c_str(), &held, err, sizeof err))) { fprintf(stderr, "tracerboy-hip: %s\n", err); tb_destroy(ctx); return 1; }
        /* the state decides size, settings and time seed: a flag that contradicts it would make tb_render start over at frame 0 */
        if ((argWidth && argWidth != held.width) || (argHeight && argHeight != held.height) || (depth >= 0 && depth != held.settings.MaxBounces) ||
            (blue >= 0 && (uint32_t)blue != held.settings.EnableBlueNoise) || (timeSet && t != held.time_seed)) {
            fprintf(stderr, "tracerboy-hip: --width / --height / --depth / --blue-noise / --seed-time contradict the state in %s\n", resume.c_str());
            tb_destroy(ctx); return 2; }
        W = held.width; H = held.height; t = held.time_seed;
        const float convergence = s.ConvergencePercentage; s = held.settings; if (adaptive >= 0.0f) s.ConvergencePercentage = convergence;
        done = tb_samples_rendered(ctx); /* after the --add files */
        target = sppSet ? std::max(spp, done) : done;
        if (denoise && !denoiseGuides && target <= done) { fprintf(stderr,
            "tracerboy-hip: --resume with --denoise: render at least one more frame (--spp above the %u the state holds): the filter is guided by the "
            "last frame's normals and positions, and AOVs are not part of a state\n", done); tb_destroy(ctx); return 1; }
    } else if (frameA >= 0) {
        if ((rc = tb_state_begin(ctx, W, H, &s, t, (uint32_t)frameA))) return fail(ctx, "tb_state_begin", rc);
        done = (uint32_t)frameA; target = (uint32_t)frameB;
    }
    if (upW && (upW < W || upH < H || (uint64_t)upW * upH > (1ull << 24))) { /* before the render, not after it */
        fprintf(stderr, "tracerboy-hip: cannot upscale the %ux%u render to %ux%u: FSR 1 only upscales, to at most 2^24 pixels\n", W, H, upW, upH);
        tb_destroy(ctx); return 2; }
    if (!neuralUp.empty() && (uint64_t)W * H * 4u > (1ull << 24)) { /* likewise */
        fprintf(stderr, "tracerboy-hip: cannot upscale the %ux%u render to twice that: more than 2^24 pixels\n", W, H); tb_destroy(ctx); return 2; }
    if (!referenceFits(W, H)) { tb_destroy(ctx); return 2; }
    if (!pixelFits(W, H)) { tb_destroy(ctx); return 2; }
    if (!reference.empty() && (rc = tb_set_reference(ctx, W, H, refRgba.data()))) return fail(ctx, "tb_set_reference", rc);
    /* a line of metrics: to --metrics-out, else to standard output.  lastLineFrames: the frame count of the last "mean" line */
    FILE* metricsFile = nullptr; /* opened at the first line: with --ranks only rank 0 writes one */
    long long lastLineFrames = -1;
    auto metricsLine = [&](uint32_t surface, uint32_t frames, float* sqErrMap, bool print) {
        tb_compare_result r;
        const int e = tb_compare(ctx, surface, nullptr, &r, sqErrMap, nullptr);
        if (e || !print) return e;
        const std::string line = metricsJson(frames, surface == TB_COMPARE_MEAN ? "mean" : "denoised", r);
        if (!metricsOut.empty() && !metricsFile && !(metricsFile = fopen(metricsOut.c_str(), "w"))) { perror("tracerboy-hip: --metrics-out"); return TB_E_IO; }
        if (metricsFile) { fprintf(metricsFile, "%s\n", line.c_str()); fflush(metricsFile); } else printf("%s\n", line.c_str());
        if (surface == TB_COMPARE_MEAN) lastLineFrames = frames;
        return 0;
    };
    auto curvePoint = [&](uint32_t frames) { return metricsEvery > 0 ? metricsLine(TB_COMPARE_MEAN, frames, nullptr, true) : 0; };
    const uint32_t start = done;
    uint64_t sampled = 0; /* budgeted runs: the samples actually taken, live pixels x frames of every call (this rank's) */
    auto checkpoint = [&]() { return checkpointEvery > 0 ? tb_state_save(ctx, saveState.c_str()) : 0; };
    if (budgeted) {
        /* Sample budgets.  Window and map make the budget before the first call (a rank's also holds 0 outside its tiles, so
         * that its live counts are its own); a noise target alone lets its first call run plain and tb_budget_stop_converged make the budget.  The
         * calls are cut where anything can change: at the map's counts, at the noise target's grid (frame F, then every C), at --adaptive's own
         * grid (frame F' + 1, then every C'), at --checkpoint-every. */
        if (!budgetFits(W, H)) { tb_destroy(ctx); return 2; }
        if (cropSet || !sppMap.empty() || world > 1) {
            std::vector<uint32_t> budget((size_t)W * H, 0xffffffffu);
            const uint32_t tilesX = (W + TILE - 1) / TILE;
            for (uint32_t y = 0; y < H; y++) for (uint32_t x = 0; x < W; x++) {
                uint32_t& b = budget[(size_t)y * W + x];
                if (!mapBudget.empty()) b = mapBudget[(size_t)y * W + x];
                if (cropSet && (x < crop[0] || x >= crop[2] || y < crop[1] || y >= crop[3])) b = 0;
                if (world > 1 && ((y / TILE) * tilesX + x / TILE) % (uint32_t)world != (uint32_t)rank) b = 0;
            }
            if ((rc = tb_set_sample_budget(ctx, W, H, budget.data()))) return fail(ctx, "tb_set_sample_budget", rc);
        }
        const uint32_t noiseStart = (uint32_t)std::min<long long>(noiseAfter, target), plainEnd = (uint32_t)std::min<long long>(adaptiveAfter + 1, target);
        while (done < target) {
            long long next = target;
            for (uint32_t cut : mapCuts) if (cut > done) { next = std::min<long long>(next, cut); break; }
            if (noiseSet) next = std::min<long long>(next, done < noiseStart ? (long long)noiseStart : done + noiseChunk - (done - noiseStart) % noiseChunk);
            if (adaptive >= 0.0f) next = std::min<long long>(next, done < plainEnd ? (long long)plainEnd : done + adaptiveChunk - (done - plainEnd) % adaptiveChunk);
            if (checkpointEvery > 0) next = std::min<long long>(next, (long long)done + checkpointEvery);
            if (metricsEvery > 0) next = std::min<long long>(next, (long long)done + metricsEvery);
            if (noiseSet && done >= noiseStart && done > start) { /* (never before this run's first call: a --frames job holds nothing yet) */
                uint64_t stopped = 0, live = 0;
                if ((rc = tb_budget_stop_converged(ctx, noiseTarget, (uint32_t)noiseAfter, &stopped, &live))) return fail(ctx, "tb_budget_stop_converged", rc);
                if (live == 0) { printf("noise target: %u frames, every pixel has stopped\n", done); break; }
            }
            const uint32_t n = (uint32_t)(next - done);
            if ((rc = tb_render(ctx, W, H, n, &s, t))) return fail(ctx, "tb_render", rc);
            const float callMs = tb_last_render_ms(ctx);
            const long long live = (long long)tb_get_option(ctx, "last_live_pixels");
            done += n; ms += callMs; sampled += (uint64_t)std::max<long long>(live, 0) * n;
            if (world > 1) printf("budget rank %d: %u frames, %lld live pixels, %.3f ms\n", rank, done, live, callMs);
            else printf("budget: %u frames, %lld live pixels, %.3f ms\n", done, live, callMs);
            if ((rc = checkpoint())) return fail(ctx, "tb_state_save", rc);
            if ((rc = curvePoint(done))) return fail(ctx, "tb_compare", rc);
        }
    } else if (adaptive < 0.0f) {
        const bool chunked = states || metricsEvery > 0;
        if (!chunked) { /* the plain render: one call */
            if ((rc = tb_render(ctx, W, H, spp, &s, t))) return fail(ctx, "tb_render", rc);
            ms = tb_last_render_ms(ctx); done = spp;
        }
        while (chunked && done < target) {
            long long n = (long long)target - done;
            if (checkpointEvery > 0) n = std::min<long long>(n, checkpointEvery);
            if (metricsEvery > 0) n = std::min<long long>(n, metricsEvery);
            if ((rc = tb_render(ctx, W, H, (uint32_t)n, &s, t))) return fail(ctx, "tb_render", rc);
            ms += tb_last_render_ms(ctx); done += (uint32_t)n;
            if ((rc = checkpoint())) return fail(ctx, "tb_state_save", rc);
            if ((rc = curvePoint(done))) return fail(ctx, "tb_compare", rc);
        }
    } else {
        /* the plain call: no pixel can skip before frame F + 1; a resumed state that is past it goes straight on with the adaptive calls */
        const uint32_t plainEnd = (uint32_t)std::min<long long>(adaptiveAfter + 1, target);
        if (done < plainEnd || !states) {
            if ((rc = tb_render(ctx, W, H, plainEnd - done, &s, t))) return fail(ctx, "tb_render", rc);
            ms = tb_last_render_ms(ctx); done = plainEnd;
            if ((rc = checkpoint())) return fail(ctx, "tb_state_save", rc);
            if ((rc = curvePoint(done))) return fail(ctx, "tb_compare", rc);
        }
        while (done < target) {
            /* the calls keep the grid of an uninterrupted schedule: with --adaptive-test call the pixels are tested at those frames */
            const long long toBoundary = adaptiveChunk - ((long long)(done - plainEnd) % adaptiveChunk);
            const uint32_t n = (uint32_t)std::min<long long>(toBoundary, (long long)target - done);
            if ((rc = tb_render(ctx, W, H, n, &s, t))) return fail(ctx, "tb_render", rc);
            const float callMs = tb_last_render_ms(ctx);
            const long long live = (long long)tb_get_option(ctx, "last_live_pixels");
            done += n; ms += callMs;
            if (world > 1) printf("adaptive rank %d: %u frames, %lld live pixels, %.3f ms\n", rank, done, live, callMs);
            else printf("adaptive: %u frames, %lld live pixels, %.3f ms\n", done, live, callMs);
            if ((rc = checkpoint())) return fail(ctx, "tb_state_save", rc);
            if ((rc = curvePoint(done))) return fail(ctx, "tb_compare", rc);
            if (live == 0) break;
        }
    }
    spp = done;
    if (!saveState.empty() && (rc = tb_state_save(ctx, saveState.c_str()))) return fail(ctx, "tb_state_save", rc);
    if (world > 1 || forceRccl) {
        /* ---- the gather: packed tiles of every rank -> rank 0's accumulation surface ---- */
        Rccl nccl; if (!nccl.load()) { tb_destroy(ctx); return 1; }
#define NCCL_TRY(x) do { int e_ = (x); if (e_) { fprintf(stderr, "tracerboy-hip: rank %d: %s: %s\n", rank, #x, nccl.GetErrorString(e_)); tb_destroy(ctx); \
    return 1; } } while (0)
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "tracerboy-hip: rank %d: %s: %s\n", rank, #x, hipGetErrorString(e_)); \
    tb_destroy(ctx); return 1; } } while (0)
        RcclId id; memset(&id, 0, sizeof id);
        const char* idFile = getenv("TB_CLI_ID_FILE");
        if (rank == 0) {
            NCCL_TRY(nccl.GetUniqueId(&id));
            if (world > 1) { /* publish atomically: write beside, rename */
                if (!idFile) { fprintf(stderr, "tracerboy-hip: TB_CLI_ID_FILE is not set\n"); return 1; }
                const std::string tmp = std::string(idFile) + ".tmp";
                /* never through a link, never over an existing file */
                const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
                if (fd < 0 || write(fd, &id, sizeof id) != (ssize_t)sizeof id) { perror("tracerboy-hip: unique id file"); if (fd >= 0) close(fd); return 1; }
                close(fd); if (rename(tmp.c_str(), idFile)) { perror("tracerboy-hip: rename"); return 1; }
            }
        } else {
            bool got = false;
            for (int tries = 0; tries < 6000 && !got; tries++) { /* up to 10 minutes: rank 0 may still be building its BVH */
                FILE* f = idFile ? fopen(idFile, "rb") : nullptr;
                if (f) { got = fread(&id, sizeof id, 1, f) == 1; fclose(f); }
                if (!got) usleep(100 * 1000);
            }
            if (!got) { fprintf(stderr, "tracerboy-hip: rank %d: no unique id from rank 0\n", rank); tb_destroy(ctx); return 1; }
        }
        HIP_OK(hipSetDevice(device));
        void* comm = nullptr;
        NCCL_TRY(nccl.CommInitRank(&comm, world, id, rank));
        hipStream_t stream = (hipStream_t)tb_stream(ctx);
        const uint32_t tilesX = (W + TILE - 1) / TILE, tilesY = (H + TILE - 1) / TILE, tiles = tilesX * tilesY;
        const uint64_t capacity = (uint64_t)((tiles + world - 1) / world) * TILE * TILE; /* pixels per rank buffer: every rank pads to the largest owner */
        float* packed = nullptr; HIP_OK(hipMalloc((void**)&packed, capacity * 16)); HIP_OK(hipMemsetAsync(packed, 0, capacity * 16, stream));
        if ((rc = tb_pack_owned_device_async(ctx, packed))) return fail(ctx, "tb_pack_owned_device_async", rc);
        float* gathered = nullptr;
        if (rank == 0) HIP_OK(hipMalloc((void**)&gathered, capacity * 16 * (uint64_t)world));
        NCCL_TRY(nccl.GroupStart());
        if (rank == 0) { for (int r = 1; r < world; r++) NCCL_TRY(nccl.Recv(gathered + (size_t)r * capacity * 4, capacity * 4, kNcclFloat, r, comm, stream)); }
        else NCCL_TRY(nccl.Send(packed, capacity * 4, kNcclFloat, 0, comm, stream));
        NCCL_TRY(nccl.GroupEnd());
        if (rank == 0) {
            HIP_OK(hipMemcpyAsync(gathered, packed, capacity * 16, hipMemcpyDeviceToDevice, stream));
            void *surface = nullptr, *jit = nullptr;
            if ((rc = tb_accum_device_ptr(ctx, &surface, &jit))) return fail(ctx, "tb_accum_device_ptr", rc);
            if ((rc = tb_unpack_gathered_device(ctx, stream, gathered, capacity, W, H, (uint32_t)world, TILE, TILE, surface))) return fail(ctx,
                "tb_unpack_gathered_device", rc);
        }
        if ((rc = tb_sync(ctx))) return fail(ctx, "tb_sync", rc);
        NCCL_TRY(nccl.CommDestroy(comm));
        (void)hipFree(packed); if (gathered) (void)hipFree(gathered);
        if (rank != 0) { tb_destroy(ctx); return 0; } /* the picture is rank 0's to write */
        /* render + gather + un-permute, rank 0's wall clock */
        ms = (float)(std::chrono::duration<double>(std::chrono::steady_clock::now() - r0).count() * 1e3);
#undef NCCL_TRY
#undef HIP_OK
    }
    const bool png = out.size() >= 4 && out.compare(out.size() - 4, 4, ".png") == 0;
    std::vector<float> denoised;
    if (denoise) { /* after --save-state: a state is the raw accumulation */
        tb_denoiser_settings dn; tb_default_denoiser_settings(&dn);
        if (denoiseIterations >= 0) dn.WaveletIterations = (uint32_t)denoiseIterations;
        if (!png && !upW && neuralUp.empty()) denoised.resize((size_t)W * H * 4);
        if (denoiseGuides) { /* the last min(K, frames held) frames of the state's range, traced again */
            const uint32_t next = tb_samples_rendered(ctx), first = (uint32_t)tb_get_option(ctx, "state_first_frame");
            const uint32_t k = (uint32_t)std::min<long long>(denoiseGuides, (long long)next - (long long)first);
            if ((rc = tb_render_guides(ctx, next - k, k))) return fail(ctx, "tb_render_guides", rc);
            printf("guides: first hits of frames [%u, %u), %.3f ms on the GPU\n", next - k, next, (double)tb_get_option(ctx, "last_guides_us") / 1e3);
            if ((rc = tb_set_option(ctx, "denoise_guides", demodulate ? 2 : 1))) return fail(ctx, "tb_set_option", rc);
        }
        if ((rc = tb_denoise(ctx, &dn, denoised.empty() ? nullptr : denoised.data()))) return fail(ctx, "tb_denoise", rc);
        printf("denoise: %u a-trous passes, %.3f ms on the GPU\n", dn.WaveletIterations, (double)tb_get_option(ctx, "last_denoise_us") / 1e3);
        if ((png || upW || !neuralUp.empty()) && (rc = tb_set_option(ctx, "post_denoised", 1))) return fail(ctx, "tb_set_option", rc);
    }
    if (!reference.empty()) { /* the final lines; the error map is that of the last one */
        std::vector<float> sq(errorMap.empty() ? 0 : (size_t)W * H);
        const bool meanMap = !denoise && !sq.empty(), meanLine = lastLineFrames != (long long)spp;
        if ((meanLine || meanMap) && (rc = metricsLine(TB_COMPARE_MEAN, spp, meanMap ? sq.data() : nullptr, meanLine))) return fail(ctx, "tb_compare", rc);
        if (denoise && (rc = metricsLine(TB_COMPARE_DENOISED, spp, sq.empty() ? nullptr : sq.data(), true))) return fail(ctx, "tb_compare", rc);
        if (metricsFile && fclose(metricsFile)) { perror("tracerboy-hip: --metrics-out"); tb_destroy(ctx); return 1; }
        metricsFile = nullptr;
        if (!sq.empty()) {
            std::vector<float> grey((size_t)W * H * 4);
            for (size_t i = 0; i < sq.size(); i++) { grey[4 * i] = grey[4 * i + 1] = grey[4 * i + 2] = sq[i]; grey[4 * i + 3] = 1.0f; }
            if ((rc = tb_write_image_f32(errorMap.c_str(), W, H, grey.data()))) return fail(ctx, "tb_write_image_f32 (--error-map)", rc);
        }
    }
    if (visSet) { /* the occluder, the paths, the output stage, the overlay */
        const uint32_t next = tb_samples_rendered(ctx), first = (uint32_t)tb_get_option(ctx, "state_first_frame");
        if (!denoise && next > first) { /* the render ran without AOVs: the last frame's first hits, traced again */
            if ((rc = tb_render_guides(ctx, next - 1u, 1u))) return fail(ctx, "tb_render_guides", rc);
        }
        uint32_t recA = (uint32_t)visA, recB = (uint32_t)visB;
        if (visA < 0) { recB = next; recA = next - std::min<uint32_t>(64u, next - first); }
        FILE* pathsFile = nullptr;
        if (!pathsOut.empty() && !(pathsFile = fopen(pathsOut.c_str(), "w"))) { perror("tracerboy-hip: --paths-out"); tb_destroy(ctx); return 1; }
        uint64_t raysTotal = 0; double pathsMs = 0.0;
        std::vector<TbPathFrame> frames; std::vector<TbVisualizerRay> rays;
        for (uint32_t f = recA; f < recB; ) { /* a call records at most 4096 frames */
            const uint32_t n = std::min<uint32_t>(4096u, recB - f);
            uint32_t total = 0, count = 0;
            frames.resize(n);
            if ((rc = tb_record_paths(ctx, (uint32_t)visX, (uint32_t)visY, f, n, frames.data(), &total))) return fail(ctx, "tb_record_paths", rc);
            raysTotal += total; pathsMs += (double)tb_get_option(ctx, "last_paths_us") / 1e3;
            if (pathsFile) {
                rays.resize(TB_MAX_VISUALIZER_RAYS);
                if ((rc = tb_read_paths(ctx, rays.data(), TB_MAX_VISUALIZER_RAYS, &count))) return fail(ctx, "tb_read_paths", rc);
                for (const TbPathFrame& fr : frames) {
                    std::string line = "{\"frame\": " + std::to_string(fr.frame) + ", \"sum\": [" + jsonNumber(fr.sum[0]) + ", " + jsonNumber(fr.sum[1]) + ", " +
                        jsonNumber(fr.sum[2]) + ", " + jsonNumber(fr.sum[3]) + "], \"flags\": " + std::to_string(fr.flags) + ", \"num_rays\": " +
                        std::to_string(fr.num_rays) + ", \"rays\": [";
                    const uint32_t stored = fr.first_ray == 0xffffffffu ? 0u : std::min<uint32_t>(fr.num_rays, count - std::min(count, fr.first_ray));
                    for (uint32_t i = 0; i < stored; i++) {
                        const TbVisualizerRay& r = rays[fr.first_ray + i];
                        line += std::string(i ? ", " : "") + "{\"origin\": [" + jsonNumber(r.Origin[0]) + ", " + jsonNumber(r.Origin[1]) + ", " + jsonNumber(r.Origin[2]) +
                            "], \"direction\": [" + jsonNumber(r.Direction[0]) + ", " + jsonNumber(r.Direction[1]) + ", " + jsonNumber(r.Direction[2]) + "], \"hit_t\": " +
                            jsonNumber(r.HitT) + ", \"bounce\": " + jsonNumber(r.BounceCount) + "}";
                    }
                    fprintf(pathsFile, "%s]}\n", line.c_str());
                }
            }
            f += n;
        }
        if (pathsFile && fclose(pathsFile)) { perror("tracerboy-hip: --paths-out"); tb_destroy(ctx); return 1; }
        uint32_t held = 0;
        if ((rc = tb_read_paths(ctx, nullptr, 0, &held))) return fail(ctx, "tb_read_paths", rc);
        printf("paths: pixel (%lld, %lld), frames [%u, %u): %llu rays, %u stored, %.3f ms on the GPU\n", visX, visY, recA, recB, (unsigned long long)raysTotal,
               held, pathsMs);
        if ((rc = tb_post_process(ctx, &post, TB_OUTPUT_TYPE_LIT, nullptr, nullptr))) return fail(ctx, "tb_post_process", rc);
        std::vector<uint8_t> img(png ? (size_t)W * H * 4 : 0); std::vector<float> imgF(png ? 0 : (size_t)W * H * 4);
        if ((rc = tb_visualize_rays(ctx, &vis, png ? nullptr : imgF.data(), png ? img.data() : nullptr))) return fail(ctx, "tb_visualize_rays", rc);
        printf("visualize: depth source %lld, %.3f ms on the GPU\n", (long long)tb_get_option(ctx, "visualize_depth_source"),
               (double)tb_get_option(ctx, "last_visualize_us") / 1e3);
        if (png) { if ((rc = tb_write_image_rgba8(out.c_str(), W, H, img.data()))) return fail(ctx, "tb_write_image_rgba8", rc); }
        else if ((rc = tb_write_image_f32(out.c_str(), W, H, imgF.data()))) return fail(ctx, "tb_write_image_f32 (use .png, .pfm or .exr)", rc);
    } else if (!neural.empty()) { /* the output stage, then the network; after --save-state: a state is the raw accumulation */
        if ((rc = tb_neural_load(ctx, neural.c_str()))) return fail(ctx, "tb_neural_load", rc);
        if (denoiseGuides) { /* the last min(K, frames held) frames of the state's range, traced again */
            const uint32_t next = tb_samples_rendered(ctx), first = (uint32_t)tb_get_option(ctx, "state_first_frame");
            const uint32_t k = (uint32_t)std::min<long long>(denoiseGuides, (long long)next - (long long)first);
            if ((rc = tb_render_guides(ctx, next - k, k))) return fail(ctx, "tb_render_guides", rc);
            printf("guides: first hits of frames [%u, %u), %.3f ms on the GPU\n", next - k, next, (double)tb_get_option(ctx, "last_guides_us") / 1e3);
        }
        std::vector<uint8_t> img(png ? (size_t)W * H * 4 : 0); std::vector<float> imgF((size_t)W * H * 4);
        if ((rc = tb_denoise_neural(ctx, &post, imgF.data(), png ? img.data() : nullptr))) return fail(ctx, "tb_denoise_neural", rc);
        printf("neural denoise: %lld input channels, %.3f ms on the GPU\n", (long long)tb_get_option(ctx, "neural_inputs"),
               (double)tb_get_option(ctx, "last_neural_us") / 1e3);
        size_t notFinite = 0; /* the colour goes in clamped; a non-finite guide value or an overflow inside the network would still show here */
        for (float v : imgF) notFinite += !(v - v == 0.0f);
        if (notFinite) fprintf(stderr, "tracerboy-hip: warning: %zu values of the network's picture are not finite\n", notFinite);
        if (png) { if ((rc = tb_write_image_rgba8(out.c_str(), W, H, img.data()))) return fail(ctx, "tb_write_image_rgba8", rc); }
        else if ((rc = tb_write_image_f32(out.c_str(), W, H, imgF.data()))) return fail(ctx, "tb_write_image_f32 (use .png, .pfm or .exr)", rc);
    } else if (!neuralUp.empty()) { /* the output stage at the rendered size, then the network to twice that */
        if ((rc = tb_sr_load(ctx, neuralUp.c_str()))) return fail(ctx, "tb_sr_load", rc);
        std::vector<uint8_t> img(png ? (size_t)W * H * 16 : 0); std::vector<float> imgF((size_t)W * H * 16);
        if ((rc = tb_upscale_neural(ctx, &post, imgF.data(), png ? img.data() : nullptr))) return fail(ctx, "tb_upscale_neural", rc);
        printf("neural upscale: %ux%u -> %ux%u, %.3f ms on the GPU\n", W, H, 2u * W, 2u * H, (double)tb_get_option(ctx, "last_sr_us") / 1e3);
        size_t notFinite = 0; /* the picture goes in clamped; an overflow inside the network would still show here */
        for (float v : imgF) notFinite += !(v - v == 0.0f);
        if (notFinite) fprintf(stderr, "tracerboy-hip: warning: %zu values of the network's picture are not finite\n", notFinite);
        if (png) { if ((rc = tb_write_image_rgba8(out.c_str(), 2u * W, 2u * H, img.data()))) return fail(ctx, "tb_write_image_rgba8", rc); }
        else if ((rc = tb_write_image_f32(out.c_str(), 2u * W, 2u * H, imgF.data()))) return fail(ctx, "tb_write_image_f32 (use .png, .pfm or .exr)", rc);
    } else if (upW) { /* the output stage at the rendered size, then FSR 1 to the picture's */
        std::vector<uint8_t> img(png ? (size_t)upW * upH * 4 : 0); std::vector<float> imgF(png ? 0 : (size_t)upW * upH * 4);
        if ((rc = tb_upscale(ctx, &post, TB_OUTPUT_TYPE_LIT, upW, upH, fsrSharpness, png ? nullptr : imgF.data(), png ? img.data() : nullptr)))
            return fail(ctx, "tb_upscale", rc);
        printf("upscale: %ux%u -> %ux%u, EASU %.3f ms + RCAS %.3f ms on the GPU\n", W, H, upW, upH, (double)tb_get_option(ctx, "last_easu_us") / 1e3,
               (double)tb_get_option(ctx, "last_rcas_us") / 1e3);
        if (png) { if ((rc = tb_write_image_rgba8(out.c_str(), upW, upH, img.data()))) return fail(ctx, "tb_write_image_rgba8", rc); }
        else if ((rc = tb_write_image_f32(out.c_str(), upW, upH, imgF.data()))) return fail(ctx, "tb_write_image_f32 (use .png, .pfm or .exr)", rc);
    } else if (png) {
        std::vector<uint8_t> img((size_t)W * H * 4);
        if ((rc = tb_post_process(ctx, &post, TB_OUTPUT_TYPE_LIT, nullptr, img.data()))) return fail(ctx, "tb_post_process", rc);
        if ((rc = tb_write_image_rgba8(out.c_str(), W, H, img.data()))) return fail(ctx, "tb_write_image_rgba8", rc);
    } else if (denoise) {
        if ((rc = tb_write_image_f32(out.c_str(), W, H, denoised.data()))) return fail(ctx, "tb_write_image_f32 (use .png, .pfm or .exr)", rc);
    } else {
        std::vector<float> acc((size_t)W * H * 4);
        if ((rc = tb_read_accum(ctx, acc.data(), nullptr))) return fail(ctx, "tb_read_accum", rc);
        for (size_t i = 0; i < (size_t)W * H; i++) { float w = acc[4 * i + 3], inv = w > 0 ? 1.0f / w : 0.0f; acc[4 * i] *= inv; acc[4 * i + 1] *= inv;
            acc[4 * i + 2] *= inv; acc[4 * i + 3] = w > 0 ? 1.0f : 0.0f; }
        if ((rc = tb_write_image_f32(out.c_str(), W, H, acc.data()))) return fail(ctx, "tb_write_image_f32 (use .png, .pfm or .exr)", rc);
    }
    printf("%s: %u triangles, %ux%u x %u spp, depth %d, %d GPU%s: %.2f ms (%.1f Msamples/s), scene load + BVH %.2f s -> %s\n",
           scene.c_str(), info.numTriangles, W, H, spp, s.MaxBounces, world, world > 1 ? "s (tiles gathered over RCCL)" : "", ms,
               ms > 0.0f ? (budgeted && world == 1 ? (double)sampled : (double)W * H * (spp - start)) / (ms * 1e3) : 0.0, loadS, out.c_str());
    if (budgeted && world == 1) printf("budget: %llu samples taken of the %llu a full render of these frames takes\n", (unsigned long long)sampled,
        (unsigned long long)W * H * (spp - start));
    tb_destroy(ctx);
    return 0;
}
