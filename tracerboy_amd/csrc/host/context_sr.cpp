/* context_sr.cpp -- the neural 2 x super-resolution (include/tracerboy_hip.h tb_sr_load / tb_run_conv / tb_run_sr_finish /
 * tb_run_sr / tb_upscale_neural): the reference's DirectMLSuperResolutionPass (DirectMLSuperResolution.cpp:304-409, :986-1091) -- seven convolutions,
 * three at the rendered size, four at twice that, and a residual add onto the nearest-upsampled input -- on the fp16 matrix cores
 * (nn_convk_kernels.hip).  The weights come from a file of the reference's container that the caller names (sr_weights.cpp); the library ships
 * none.  Reads what the output stage wrote, writes surfaces of its own: accumulation, AOVs, frame counter, history, guides and denoised surfaces
 * stay as they are. */
#include "context_internal.h"
#include "sr_weights.h"
#include "../kernels/nn_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

const uint32_t kMaxSeamChannels = 512;

/* The seven layers and the residual add on the context's activation buffers, enqueued on its stream: color is a width x height RGBA32F device
 * surface, out 2 width x 2 height.  unormColor: the colour is packed through the R8G8B8A8_UNORM store (nn_launch_pack_input).  The two
 * upsamples cost no pass: conv_up1 gathers its source at (y >> 1, x >> 1), and so does the residual add.  Option sr_conv_form picks the form of
 * the convolutions; a layer with more input channels than the staged form's LDS image holds runs in the plain form -- the same bits. */
void runNetwork(tb_context* c, uint32_t width, uint32_t height, const void* color, bool unormColor, void* out)
{
    tb_context::Sr& n = c->sr;
    const uint32_t W2 = width * 2u, H2 = height * 2u;
    size_t most = 0;
    for (uint32_t l = 0; l < tbsr::kLayers; l++) most = std::max(most, l < 3u ? tensorBytes(width, height, n.out[l]) : tensorBytes(W2, H2, n.out[l]));
    ensure(n.input, tensorBytes(width, height, 3u)); ensure(n.pingPong[0], most); ensure(n.pingPong[1], most);
    uint16_t* const x = (uint16_t*)n.input.p; uint16_t* const a = (uint16_t*)n.pingPong[0].p; uint16_t* const b = (uint16_t*)n.pingPong[1].p;
    hipStream_t s = c->stream;
    auto conv = [&](uint32_t l, const uint16_t* in, uint16_t* dst) {
        const bool full = l >= 3u, last = l + 1u == tbsr::kLayers;
        const uint32_t form = opt<OPT_sr_conv_form>(c) && nn_convk_staged_fits(n.in[l], 0u) ? 1u : 0u;
        HIP_TRY(nn_launch_convk(s, full ? W2 : width, full ? H2 : height, n.kernel[l], form, in, n.in[l], l == 3u, nullptr, 0u, (const uint16_t*)n.weight[l].p,
            last ? nullptr : (const float*)n.bias[l].p, n.out[l], last ? 0u : 1u, dst));
    };
    HIP_TRY(nn_launch_pack_input(s, width, height, width, height, (const TbFloat4*)color, nullptr, nullptr, unormColor, x));
    conv(0, x, a); conv(1, a, b); conv(2, b, a);
    conv(3, a, b); conv(4, b, a); conv(5, a, b); conv(6, b, a);
    HIP_TRY(nn_launch_sr_finish(s, width, height, a, x, (TbFloat4*)out));
}

/* why the network refuses a picture of that size; null: it does not */
const char* pictureRefusal(uint32_t W, uint32_t H)
{
    if (W == 0 || H == 0) return "a dimension is 0";
    if ((uint64_t)W * H * 4u > (1ull << 24)) return "more than 2^24 output pixels";
    return nullptr;
}

void timedNetwork(tb_context* c, uint32_t W, uint32_t H, const void* color, bool unormColor, void* out)
{
    HIP_TRY(hipEventRecord(c->sr.ev[0].create(), c->stream));
    runNetwork(c, W, H, color, unormColor, out);
    HIP_TRY(hipEventRecord(c->sr.ev[1].create(), c->stream));
}

void readTime(tb_context* c) { if (hipEventElapsedTime(&c->sr.lastMs, c->sr.ev[0], c->sr.ev[1]) != hipSuccess) c->sr.lastMs = 0.0f; }

} // namespace

extern "C" {

int tb_sr_load(tb_context* c, const char* path)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (!path) return fail(c, TB_E_INVALID, "tb_sr_load: null path");
        tbsr::Weights w;
        try { w = tbsr::read(path); } catch (const tbnn::Error& e) { return fail(c, e.code, "tb_sr_load: " + e.message); }
        tb_context::Sr& n = c->sr;
        HIP_TRY(hipStreamSynchronize(c->stream)); /* a network of the weights loaded before has finished */
        n.loaded = false;
        for (uint32_t l = 0; l < tbsr::kLayers; l++) {
            const tbsr::Layer& L = w.layer[l];
            uploadLayer(tbnn::packLayer(L.in, 0u, L.out, L.weight.data(), L.bias.empty() ? nullptr : L.bias.data(), L.kernel * L.kernel), n.weight[l], n.bias[l]);
            n.in[l] = L.in; n.out[l] = L.out; n.kernel[l] = L.kernel;
        }
        n.loaded = true;
        return TB_OK;
    });
}

int tb_run_conv(tb_context* c, const tb_conv_desc* d, const uint16_t* inA, const uint16_t* inB, const uint16_t* weight, const uint16_t* bias, uint16_t* out)
{
    return guarded(c, [&]() {
        if (!d || !inA || !weight || !out) return fail(c, TB_E_INVALID, "tb_run_conv: null pointer");
        if (const char* why = surfaceRefusal(d->width, d->height)) return fail(c, TB_E_INVALID, std::string("tb_run_conv: ") + why);
        if (d->kernel != 3u && d->kernel != 5u) return fail(c, TB_E_INVALID, "tb_run_conv: kernel " + std::to_string(d->kernel) + " (3 or 5)");
        if (d->form > 1u) return fail(c, TB_E_INVALID, "tb_run_conv: form " + std::to_string(d->form) + " (0 plain, 1 staged)");
        if (!d->c_a || !d->c_out) return fail(c, TB_E_INVALID, "tb_run_conv: a channel count is 0");
        if (d->c_a > kMaxSeamChannels || d->c_b > kMaxSeamChannels || d->c_out > kMaxSeamChannels) return fail(c, TB_E_INVALID,
            "tb_run_conv: more than " + std::to_string(kMaxSeamChannels) + " channels in a tensor");
        if ((d->c_b != 0u) != (inB != nullptr)) return fail(c, TB_E_INVALID, "tb_run_conv: source B is given exactly when c_b is not 0");
        if (d->upsample_a && ((d->width | d->height) & 1u)) return fail(c, TB_E_INVALID, "tb_run_conv: upsample_a needs an even width and height");
        if (d->form == 1u && !nn_convk_staged_fits(d->c_a, d->c_b)) return fail(c, TB_E_INVALID,
            "tb_run_conv: the staged form holds at most 64 input channels, each source padded to a multiple of 32");
        const uint32_t W = d->width, H = d->height, wA = d->upsample_a ? W / 2u : W, hA = d->upsample_a ? H / 2u : H, padOut = nn_padded_channels(d->c_out);
        const std::vector<uint16_t> hostA = padChannels(inA, (size_t)wA * hA, d->c_a);
        const DevBuf dA = staged(hostA.data(), hostA.size() * sizeof(uint16_t));
        DevBuf dB;
        if (inB) { const std::vector<uint16_t> hostB = padChannels(inB, (size_t)W * H, d->c_b); dB = staged(hostB.data(), hostB.size() * sizeof(uint16_t)); }
        DevBuf dWeight, dBias;
        uploadLayer(tbnn::packLayer(d->c_a, d->c_b, d->c_out, weight, bias, d->kernel * d->kernel), dWeight, dBias);
        const DevBuf dOut = scratch(tensorBytes(W, H, d->c_out));
        HIP_TRY(nn_launch_convk(c->stream, W, H, d->kernel, d->form, (const uint16_t*)dA.p, d->c_a, d->upsample_a, (const uint16_t*)dB.p, d->c_b,
            (const uint16_t*)dWeight.p, bias ? (const float*)dBias.p : nullptr, d->c_out, d->relu, (uint16_t*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<uint16_t> host(dOut.bytes / sizeof(uint16_t));
        copyBack(host.data(), dOut);
        for (size_t i = 0; i < (size_t)W * H; i++) memcpy(out + i * d->c_out, &host[i * padOut], d->c_out * sizeof(uint16_t));
        return TB_OK;
    });
}

int tb_run_sr_finish(tb_context* c, uint32_t inW, uint32_t inH, const uint16_t* residual, const uint16_t* input, float* out)
{
    return guarded(c, [&]() {
        if (!residual || !input || !out) return fail(c, TB_E_INVALID, "tb_run_sr_finish: null array");
        if (const char* why = pictureRefusal(inW, inH)) return fail(c, TB_E_INVALID, std::string("tb_run_sr_finish: ") + why);
        const size_t px = (size_t)inW * inH;
        const std::vector<uint16_t> hostR = padChannels(residual, px * 4u, 3u), hostI = padChannels(input, px, 3u);
        const DevBuf dR = staged(hostR.data(), hostR.size() * sizeof(uint16_t)), dI = staged(hostI.data(), hostI.size() * sizeof(uint16_t));
        const DevBuf dOut = scratch(px * 4u * sizeof(TbFloat4));
        HIP_TRY(nn_launch_sr_finish(c->stream, inW, inH, (const uint16_t*)dR.p, (const uint16_t*)dI.p, (TbFloat4*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_run_sr(tb_context* c, uint32_t W, uint32_t H, const float* color, float* out)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        if (!color || !out) return fail(c, TB_E_INVALID, "tb_run_sr: null pointer");
        if (!c->sr.loaded) return fail(c, TB_E_INVALID, "tb_run_sr: no weights: call tb_sr_load");
        if (const char* why = pictureRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_run_sr: ") + why);
        const size_t bytes = (size_t)W * H * sizeof(TbFloat4);
        const DevBuf dColor = staged(color, bytes), dOut = scratch(bytes * 4u);
        timedNetwork(c, W, H, dColor.p, false, dOut.p);
        HIP_TRY(hipStreamSynchronize(c->stream));
        readTime(c);
        copyBack(out, dOut);
        return TB_OK;
    });
}

int tb_upscale_neural(tb_context* c, const tb_post_settings* post, float* rgbaF32, uint8_t* rgba8)
{
    if (c && (!c->group.peers.empty() || c->group.owner)) return fail(c, TB_E_UNSUPPORTED,
        "tb_upscale_neural: not supported for a multi-device group");
    return guarded(c, [&]() {
        if (!rgbaF32 && !rgba8) return fail(c, TB_E_INVALID, "tb_upscale_neural: both output pointers are null");
        if (!c->sr.loaded) return fail(c, TB_E_INVALID, "tb_upscale_neural: no weights: call tb_sr_load");
        if (!c->output.p || !c->width) return fail(c, TB_E_INVALID, "tb_upscale_neural: nothing rendered: the context holds no frames");
        const uint32_t W = c->width, H = c->height;
        if (const char* why = pictureRefusal(W, H)) return fail(c, TB_E_INVALID, std::string("tb_upscale_neural: ") + why);
        if (int rc = launchPostProcess(c, post, TB_OUTPUT_TYPE_LIT)) return rc; /* refuses what tb_post_process refuses, with its message */
        tb_context::Sr& n = c->sr;
        const size_t px = (size_t)W * H * 4u;
        ensure(n.result, px * sizeof(TbFloat4));
        /* the reference's network reads its R8G8B8A8_UNORM post-process surface: the colour is packed through that store */
        timedNetwork(c, W, H, c->postOut.p, true, n.result.p);
        if (rgba8) { ensure(n.rgba8, px * 4); HIP_TRY(nn_launch_to_rgba8(c->stream, W * 2u, H * 2u, (const TbFloat4*)n.result.p, (uint32_t*)n.rgba8.p)); }
        HIP_TRY(hipStreamSynchronize(c->stream));
        readTime(c);
        if (rgbaF32) HIP_TRY(hipMemcpy(rgbaF32, n.result.p, px * sizeof(TbFloat4), hipMemcpyDeviceToHost));
        if (rgba8) HIP_TRY(hipMemcpy(rgba8, n.rgba8.p, px * 4, hipMemcpyDeviceToHost));
        return TB_OK;
    });
}

} // extern "C"
