/* context_neural.cpp -- the neural still denoiser (include/tracerboy_hip.h tb_neural_load / tb_run_conv3x3 / tb_run_neural /
 * tb_denoise_neural): the reference's TAAUpscaler::OIDN path (TracerBoy.cpp:3306-3322, OpenImageDenoise.cpp:855-1039) -- the OIDN U-Net of 16
 * 3 x 3 convolutions on the post-processed picture, the mean albedo and the mean normals -- on the fp16 matrix cores (nn_convk_kernels.hip).  The weights
 * come from a TZA file the caller names (nn_weights.cpp); the library ships none.  Reads what the output stage and the guide pass wrote, writes
 * surfaces of its own: accumulation, AOVs, frame counter, history, guides and denoised surfaces stay as they are. */
#include "context_internal.h"
#include "nn_weights.h"
#include "../kernels/nn_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace tbctx {

size_t tensorBytes(uint32_t w, uint32_t h, uint32_t channels) { return (size_t)w * h * nn_padded_channels(channels) * sizeof(uint16_t); }

/* a layer's weights on the device, as nn_convk reads them */
void uploadLayer(const tbnn::PackedLayer& p, DevBuf& weight, DevBuf& bias)
{
    ensure(weight, p.weight.size() * sizeof(uint16_t)); ensure(bias, p.bias.size() * sizeof(float));
    HIP_TRY(hipMemcpy(weight.p, p.weight.data(), weight.bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bias.p, p.bias.data(), bias.bytes, hipMemcpyHostToDevice));
}

/* unpadded NHWC on the host <-> channels padded to 32 */
std::vector<uint16_t> padChannels(const uint16_t* in, size_t pixels, uint32_t c)
{
    const uint32_t pad = nn_padded_channels(c);
    std::vector<uint16_t> v(pixels * pad, 0);
    for (size_t i = 0; i < pixels; i++) memcpy(&v[i * pad], in + i * c, c * sizeof(uint16_t));
    return v;
}

int runConvSeam(tb_context* c, const char* name, const tb_conv_desc* d, int pool, const uint16_t* inA, const uint16_t* inB, const uint16_t* weight,
    const uint16_t* bias, uint16_t* out)
{
    const uint32_t kMaxSeamChannels = 512;
    const auto refuse = [&](const std::string& why) { return fail(c, TB_E_INVALID, std::string(name) + ": " + why); };
    if (!d || !inA || !weight || !out) return refuse("null pointer");
    if (const char* why = surfaceRefusal(d->width, d->height)) return refuse(why);
    if (d->kernel != 3u && d->kernel != 5u) return refuse("kernel " + std::to_string(d->kernel) + " (3 or 5)");
    if (d->form > 1u) return refuse("form " + std::to_string(d->form) + " (0 plain, 1 staged)");
    if (!d->c_a || !d->c_out) return refuse("a channel count is 0");
    if (d->c_a > kMaxSeamChannels || d->c_b > kMaxSeamChannels || d->c_out > kMaxSeamChannels)
        return refuse("more than " + std::to_string(kMaxSeamChannels) + " channels in a tensor");
    if ((d->c_b != 0u) != (inB != nullptr)) return refuse("source B is given exactly when c_b is not 0");
    if ((pool > 0 || d->upsample_a) && ((d->width | d->height) & 1u))
        return refuse(pool < 0 ? "upsample_a needs an even width and height" : "pool and upsample_a need an even width and height");
    if (d->form == 1u && !nn_convk_staged_fits(d->c_a, d->c_b)) return refuse("the staged form holds at most 64 input channels, each source padded to a multiple of 32");
    const uint32_t W = d->width, H = d->height, wA = d->upsample_a ? W / 2u : W, hA = d->upsample_a ? H / 2u : H;
    const uint32_t wOut = pool > 0 ? W / 2u : W, hOut = pool > 0 ? H / 2u : H, padOut = nn_padded_channels(d->c_out);
    const std::vector<uint16_t> hostA = padChannels(inA, (size_t)wA * hA, d->c_a);
    const DevBuf dA = staged(hostA.data(), hostA.size() * sizeof(uint16_t));
    DevBuf dB;
    if (inB) { const std::vector<uint16_t> hostB = padChannels(inB, (size_t)W * H, d->c_b); dB = staged(hostB.data(), hostB.size() * sizeof(uint16_t)); }
    DevBuf dWeight, dBias;
    uploadLayer(tbnn::packLayer(d->c_a, d->c_b, d->c_out, weight, bias, d->kernel * d->kernel), dWeight, dBias);
    const DevBuf dConv = scratch(tensorBytes(W, H, d->c_out));
    HIP_TRY(nn_launch_convk(c->stream, W, H, d->kernel, d->form, (const uint16_t*)dA.p, d->c_a, d->upsample_a, (const uint16_t*)dB.p, d->c_b,
        (const uint16_t*)dWeight.p, bias ? (const float*)dBias.p : nullptr, d->c_out, d->relu, (uint16_t*)dConv.p));
    DevBuf dPool;
    if (pool > 0) { dPool = scratch(tensorBytes(wOut, hOut, d->c_out)); HIP_TRY(nn_launch_maxpool2x2(c->stream, W, H, padOut, (const uint16_t*)dConv.p, (uint16_t*)dPool.p)); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    const DevBuf& result = pool > 0 ? dPool : dConv;
    std::vector<uint16_t> host(result.bytes / sizeof(uint16_t));
    copyBack(host.data(), result);
    for (size_t i = 0; i < (size_t)wOut * hOut; i++) memcpy(out + i * d->c_out, &host[i * padOut], d->c_out * sizeof(uint16_t));
    return TB_OK;
}

void runStage(tb_context* c, tb_context::NetStage& n, const std::function<void()>& network, uint32_t outW, uint32_t outH, const void* result,
    float* rgbaF32, uint8_t* rgba8)
{
    const size_t px = (size_t)outW * outH;
    HIP_TRY(hipEventRecord(n.ev[0].create(), c->stream));
    network();
    HIP_TRY(hipEventRecord(n.ev[1].create(), c->stream));
    if (rgba8) { ensure(n.rgba8, px * 4); HIP_TRY(nn_launch_to_rgba8(c->stream, outW, outH, (const TbFloat4*)result, (uint32_t*)n.rgba8.p)); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hipEventElapsedTime(&n.lastMs, n.ev[0], n.ev[1]) != hipSuccess) n.lastMs = 0.0f;
    if (rgbaF32) HIP_TRY(hipMemcpy(rgbaF32, result, px * sizeof(TbFloat4), hipMemcpyDeviceToHost));
    if (rgba8) HIP_TRY(hipMemcpy(rgba8, n.rgba8.p, px * 4, hipMemcpyDeviceToHost));
}

} // namespace tbctx

namespace {

enum { E0, E1, E2, E3, E4, E5A, E5B, D4A, D4B, D3A, D3B, D2A, D2B, D1A, D1B, D0 }; /* tbnn::kLayerNames */

/* The 16 layers on the context's activation buffers, enqueued on its stream: color / albedo / normal are width x height RGBA32F device surfaces
 * (albedo and normal null with 3-input weights), out likewise.  The picture is zero-extended to multiples of 16 and the result cropped.
 * unormColor: the colour is packed through the R8G8B8A8_UNORM store (nn_launch_pack_input). */
void runNetwork(tb_context* c, uint32_t width, uint32_t height, const void* color, const void* albedo, const void* normal, bool unormColor, void* out)
{
    tb_context::Neural& n = c->nn;
    const uint32_t W0 = tbnn::roundUp(width, 16u), H0 = tbnn::roundUp(height, 16u);
    const uint32_t* co = n.out;
    /* the size of the level a layer writes at: 0 = the picture, 4 = a sixteenth of it each way */
    const uint32_t level[tbnn::kLayers] = {0, 0, 1, 2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0};
    size_t most = 0;
    for (uint32_t l = 0; l < tbnn::kLayers; l++) most = std::max(most, tensorBytes(W0 >> level[l], H0 >> level[l], co[l]));
    ensure(n.input, tensorBytes(W0, H0, n.inputs)); ensure(n.pingPong[0], most); ensure(n.pingPong[1], most);
    for (uint32_t s = 0; s < 3u; s++) ensure(n.skip[s], tensorBytes(W0 >> (s + 1u), H0 >> (s + 1u), co[E1 + s]));
    uint16_t* const x = (uint16_t*)n.input.p; uint16_t* const a = (uint16_t*)n.pingPong[0].p; uint16_t* const b = (uint16_t*)n.pingPong[1].p;
    uint16_t* const skip[3] = {(uint16_t*)n.skip[0].p, (uint16_t*)n.skip[1].p, (uint16_t*)n.skip[2].p};
    hipStream_t s = c->stream;
    auto conv = [&](uint32_t l, uint32_t lvl, const uint16_t* inA, bool up, const uint16_t* inB, uint16_t* dst) {
        const uint32_t cB = inB ? n.in[l] - n.splitA[l] : 0u;
        HIP_TRY(nn_launch_convk(s, W0 >> lvl, H0 >> lvl, 3u, 0u, inA, n.splitA[l], up, inB, cB, (const uint16_t*)n.weight[l].p, (const float*)n.bias[l].p, co[l], 1u, dst));
    };
    auto pool = [&](uint32_t l, uint32_t lvl, const uint16_t* in, uint16_t* dst) {
        HIP_TRY(nn_launch_maxpool2x2(s, W0 >> lvl, H0 >> lvl, nn_padded_channels(co[l]), in, dst));
    };
    HIP_TRY(nn_launch_pack_input(s, width, height, W0, H0, (const TbFloat4*)color, (const TbFloat4*)albedo, (const TbFloat4*)normal, unormColor, x));
    conv(E0, 0, x, false, nullptr, a);
    conv(E1, 0, a, false, nullptr, b); pool(E1, 0, b, skip[0]);
    conv(E2, 1, skip[0], false, nullptr, a); pool(E2, 1, a, skip[1]);
    conv(E3, 2, skip[1], false, nullptr, a); pool(E3, 2, a, skip[2]);
    conv(E4, 3, skip[2], false, nullptr, a); pool(E4, 3, a, b);
    conv(E5A, 4, b, false, nullptr, a); conv(E5B, 4, a, false, nullptr, b);
    conv(D4A, 3, b, true, skip[2], a); conv(D4B, 3, a, false, nullptr, b);
    conv(D3A, 2, b, true, skip[1], a); conv(D3B, 2, a, false, nullptr, b);
    conv(D2A, 1, b, true, skip[0], a); conv(D2B, 1, a, false, nullptr, b);
    conv(D1A, 0, b, true, x, a); conv(D1B, 0, a, false, nullptr, b);
    conv(D0, 0, b, false, nullptr, a);
    HIP_TRY(nn_launch_unpack_output(s, width, height, W0, a, (TbFloat4*)out));
}

/* why the network refuses a picture of that size; null: it does not */
const char* pictureRefusal(uint32_t W, uint32_t H)
{
    if (const char* why = surfaceRefusal(W, H)) return why;
    if ((uint64_t)tbnn::roundUp(W, 16u) * tbnn::roundUp(H, 16u) > (1ull << 24)) return "more than 2^24 pixels once extended to multiples of 16";
    return nullptr;
}

} // namespace

extern "C" {

int tb_neural_load(tb_context* c, const char* path)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (!path) return fail(c, TB_E_INVALID, "tb_neural_load: null path");
        tbnn::Weights w;
        try { w = tbnn::readTza(path); } catch (const tbnn::Error& e) { return fail(c, e.code, "tb_neural_load: " + e.message); }
        tb_context::Neural& n = c->nn;
        HIP_TRY(hipStreamSynchronize(c->stream)); /* a network of the weights loaded before has finished */
        n.inputs = 0;
        const tbnn::Layer* L = w.layer;
        for (uint32_t l = 0; l < tbnn::kLayers; l++) {
            /* a decoder's first layer reads the upsampled tensor (source A) in front of the skip tensor (source B) */
            const uint32_t cA = l == D4A ? L[E5B].out : l == D3A ? L[D4B].out : l == D2A ? L[D3B].out : l == D1A ? L[D2B].out : L[l].in;
            uploadLayer(tbnn::packLayer(cA, L[l].in - cA, L[l].out, L[l].weight.data(), L[l].bias.data()), n.weight[l], n.bias[l]);
            n.in[l] = L[l].in; n.out[l] = L[l].out; n.splitA[l] = cA;
        }
        n.inputs = L[E0].in;
        return TB_OK;
    });
}

int tb_run_conv3x3(tb_context* c, const tb_conv3x3_desc* d, const uint16_t* inA, const uint16_t* inB, const uint16_t* weight, const uint16_t* bias, uint16_t* out)
{
    return guarded(c, [&]() {
        if (!d || !bias) return fail(c, TB_E_INVALID, "tb_run_conv3x3: null pointer");
        const tb_conv_desc k = {d->width, d->height, d->c_a, d->c_b, d->c_out, 3u, d->upsample_a, d->relu, 0u};
        return runConvSeam(c, "tb_run_conv3x3", &k, d->pool ? 1 : 0, inA, inB, weight, bias, out);
    });
}

int tb_run_neural(tb_context* c, uint32_t W, uint32_t H, const float* color, const float* albedo, const float* normal, float* out)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (!color || !out) return fail(c, TB_E_INVALID, "tb_run_neural: null pointer");
        if (!c->nn.inputs) return fail(c, TB_E_INVALID, "tb_run_neural: no weights: call tb_neural_load");
        if (const char* why = pictureRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_neural: ") + why);
        const bool aux = c->nn.inputs == 9u;
        if ((albedo != nullptr) != aux || (normal != nullptr) != aux) return fail(c, TB_E_INVALID, aux ?
            "tb_run_neural: the loaded weights have 9 inputs: albedo and normal are needed" : "tb_run_neural: the loaded weights have 3 inputs: they take no albedo and no normal");
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        const DevBuf dColor = staged(color, bytes), dOut = scratch(bytes);
        DevBuf dAlbedo, dNormal;
        if (aux) { dAlbedo = staged(albedo, bytes); dNormal = staged(normal, bytes); }
        runStage(c, c->nn, [&]() { runNetwork(c, W, H, dColor.p, dAlbedo.p, dNormal.p, false, dOut.p); }, W, H, dOut.p, out, nullptr);
        return TB_OK;
    });
}

/* The four helper kernels of nn_kernels.hip on host arrays, like tb_run_composite: temporary device buffers, the context's stream, nothing else. */
int tb_run_nn_pack(tb_context* c, uint32_t W, uint32_t H, uint32_t paddedW, uint32_t paddedH, uint32_t unormColor, const float* color, const float* albedo,
                   const float* normal, uint16_t* out)
{
    return guarded(c, [&]() {
        if (!color || !out) return fail(c, TB_E_INVALID, "tb_run_nn_pack: null array");
        if ((albedo != nullptr) != (normal != nullptr)) return fail(c, TB_E_INVALID, "tb_run_nn_pack: albedo and normal are given together or not at all");
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_nn_pack: ") + why);
        if (paddedW < W || paddedH < H) return fail(c, TB_E_INVALID, "tb_run_nn_pack: the padded size is smaller than the picture");
        if (const char* why = surfaceRefusal(paddedW, paddedH)) return fail(c, TB_E_INVALID, std::string("tb_run_nn_pack: padded: ") + why);
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        const DevBuf dColor = staged(color, bytes), dOut = scratch(tensorBytes(paddedW, paddedH, 9u));
        DevBuf dAlbedo, dNormal;
        if (albedo) { dAlbedo = staged(albedo, bytes); dNormal = staged(normal, bytes); }
        HIP_TRY(nn_launch_pack_input(c->stream, W, H, paddedW, paddedH, (const TbFloat4*)dColor.p, (const TbFloat4*)dAlbedo.p, (const TbFloat4*)dNormal.p,
            unormColor, (uint16_t*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_run_nn_unpack(tb_context* c, uint32_t W, uint32_t H, uint32_t paddedW, uint32_t paddedH, const uint16_t* in, float* out)
{
    return guarded(c, [&]() {
        if (!in || !out) return fail(c, TB_E_INVALID, "tb_run_nn_unpack: null array");
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_nn_unpack: ") + why);
        if (paddedW < W || paddedH < H) return fail(c, TB_E_INVALID, "tb_run_nn_unpack: the padded size is smaller than the picture");
        if (const char* why = surfaceRefusal(paddedW, paddedH)) return fail(c, TB_E_INVALID, std::string("tb_run_nn_unpack: padded: ") + why);
        const DevBuf dIn = staged(in, tensorBytes(paddedW, paddedH, 3u)), dOut = scratch((size_t)W * H * sizeof(TbFloat4));
        HIP_TRY(nn_launch_unpack_output(c->stream, W, H, paddedW, (const uint16_t*)dIn.p, (TbFloat4*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_run_nn_resolve_aux(tb_context* c, uint32_t W, uint32_t H, const float* albedoSum, const float* normalSum, float* albedo, float* normal)
{
    return guarded(c, [&]() {
        if (!albedoSum || !normalSum || !albedo || !normal) return fail(c, TB_E_INVALID, "tb_run_nn_resolve_aux: null array");
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_nn_resolve_aux: ") + why);
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        const DevBuf dA = staged(albedoSum, bytes), dN = staged(normalSum, bytes), dAlbedo = scratch(bytes), dNormal = scratch(bytes);
        HIP_TRY(nn_launch_resolve_aux(c->stream, W, H, (const TbFloat4*)dA.p, (const TbFloat4*)dN.p, (TbFloat4*)dAlbedo.p, (TbFloat4*)dNormal.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(albedo, dAlbedo); copyBack(normal, dNormal);
        return TB_OK;
    });
}

int tb_run_nn_to_rgba8(tb_context* c, uint32_t W, uint32_t H, const float* in, uint8_t* out)
{
    return guarded(c, [&]() {
        if (!in || !out) return fail(c, TB_E_INVALID, "tb_run_nn_to_rgba8: null array");
        if (const char* why = surfaceRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_nn_to_rgba8: ") + why);
        const DevBuf dIn = staged(in, (size_t)W * H * sizeof(TbFloat4)), dOut = scratch((size_t)W * H * 4u);
        HIP_TRY(nn_launch_to_rgba8(c->stream, W, H, (const TbFloat4*)dIn.p, (uint32_t*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_denoise_neural(tb_context* c, const tb_post_settings* post, float* rgbaF32, uint8_t* rgba8)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_denoise_neural: not supported for a multi-device group: the guide surfaces are not gathered across its devices");
    return guarded(c, [&]() {
        if (!rgbaF32 && !rgba8) return fail(c, TB_E_INVALID, "tb_denoise_neural: both output pointers are null");
        if (!c->nn.inputs) return fail(c, TB_E_INVALID, "tb_denoise_neural: no weights: call tb_neural_load");
        if (!c->output.p || !c->width) return fail(c, TB_E_INVALID, "tb_denoise_neural: nothing rendered: the context holds no frames");
        const bool aux = c->nn.inputs == 9u;
        if (aux && !guidesCurrent(c)) return fail(c, TB_E_INVALID,
            "tb_denoise_neural: the loaded weights read albedo and normals and the context holds no valid guide surfaces: call tb_render_guides (a history "
            "reset, a resize, a scene load or a change of camera, settings or time seed invalidates them)");
        const uint32_t W = c->width, H = c->height;
        if (const char* why = pictureRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_denoise_neural: ") + why);
        if (int rc = launchPostProcess(c, post, TB_OUTPUT_TYPE_LIT)) return rc; /* refuses what tb_post_process refuses, with its message */
        tb_context::Neural& n = c->nn;
        const size_t px = (size_t)W * H;
        ensure(n.result, px * sizeof(TbFloat4));
        if (aux) { ensure(n.aux[0], px * sizeof(TbFloat4)); ensure(n.aux[1], px * sizeof(TbFloat4));
            HIP_TRY(nn_launch_resolve_aux(c->stream, W, H, (const TbFloat4*)c->guides.sum[0].p, (const TbFloat4*)c->guides.sum[1].p, (TbFloat4*)n.aux[0].p,
                (TbFloat4*)n.aux[1].p)); }
        /* the reference's network reads its R8G8B8A8_UNORM post-process surface: the colour is packed through that store */
        runStage(c, n, [&]() { runNetwork(c, W, H, c->postOut.p, aux ? n.aux[0].p : nullptr, aux ? n.aux[1].p : nullptr, true, n.result.p); }, W, H,
            n.result.p, rgbaF32, rgba8);
        return TB_OK;
    });
}

} // extern "C"
