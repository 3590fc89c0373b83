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
    return guarded(c, [&]() { return runConvSeam(c, "tb_run_conv", d, -1, inA, inB, weight, bias, out); });
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
        runStage(c, c->sr, [&]() { runNetwork(c, W, H, dColor.p, false, dOut.p); }, W * 2u, H * 2u, dOut.p, out, nullptr);
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
        runStage(c, n, [&]() { runNetwork(c, W, H, c->postOut.p, true, n.result.p); }, W * 2u, H * 2u, n.result.p, rgbaF32, rgba8);
        return TB_OK;
    });
}

} // extern "C"
