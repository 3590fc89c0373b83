/* sr_weights.cpp -- reads the weights of the 2 x super-resolution network from the reference's container (DESIGN.md section 16;
 * include/tracerboy_hip.h tb_sr_weights_info / tb_sr_read_layer) and folds each layer's batch-norm scale into its filter.  Host only: no HIP header,
 * no context.
 *
 * The container (DirectMLSuperResolution.cpp:94-160), all values little-endian:
 *   int32 tensor count, then per tensor: u32 name length (at most 255), the name, u32 element count, that many binary32 values
 * A layer's filter is `<layer>/weights` in oihw order; the layers with a batch norm also have `<layer>/BatchNorm/scale` and `/shift`, one value per
 * output channel.  The file holds no shapes: the kernel sizes are the graph's, `out` is the scale tensor's length (3 for the last layer, which has
 * none) and `in` follows from the filter's element count.
 * The fold (DirectMLSuperResolution.cpp:1182-1219): filter * scale[o], one fp32 multiply, then compress(); the bias is compress(shift[o]).
 * Every read is checked against the file's length first; nothing is trusted. */
#include "sr_weights.h"
#include "tracerboy_hip.h"

#include <cstdio>
#include <cstring>
#include <map>

namespace tbsr {

const char* const kLayerNames[kLayers] = {"conv1", "conv2", "conv3", "conv_up1/conv", "conv4", "conv5", "conv6"};
const uint32_t kKernel[kLayers] = {5u, 3u, 3u, 5u, 3u, 3u, 3u};

uint16_t compress(float value)
{
    uint32_t u; memcpy(&u, &value, 4);
    const uint32_t sign = u & 0x80000000u;
    uint32_t a = u ^ sign;
    if (a < 0x38800000u) {                       /* below 2^-14, the smallest normal binary16: the subnormal's 10 bits are trunc(|value| * 2^24) ... */
        float f; memcpy(&f, &a, 4);
        a = (uint32_t)(int32_t)(f * 0x1p37f);    /* ... taken as trunc(|value| * 2^37) >> 13: the product is exact and below 2^23 */
    } else if (a > 0x477FE000u && a < 0x7F800000u) a = 0x7F800000u; /* above 65504, the largest finite binary16: infinity, whatever a rounding would say */
    else if (a > 0x7F800000u && a < 0x7F802000u) a = 0x7F802000u;   /* a NaN whose payload the shift would lose: the smallest that survives it */
    a >>= 13;                                    /* truncation */
    if (a > 0x23BFFu) a -= 0x1C000u;             /* infinity and NaN: exponent 255 -> 143, and with the line below -> 31 */
    if (a > 0x3FFu) a -= 0x1C000u;               /* normal values: the exponent's bias 127 -> 15 */
    return (uint16_t)(a | (sign >> 16));
}

uint64_t Weights::weightBytes() const
{
    uint64_t n = 0;
    for (const Layer& l : layer) n += (uint64_t)(l.weight.size() + l.bias.size()) * 2u;
    return n;
}

namespace {

[[noreturn]] void parseError(const std::string& m) { throw tbnn::Error{TB_E_PARSE, "weights.bin: " + m}; }

struct Reader {
    const uint8_t* data; size_t size, pos;
    void need(uint64_t n, const std::string& what) const { if (n > size - pos) parseError(what + " runs past the end of the file"); }
    uint32_t u32(const std::string& what)
    {
        need(4, what);
        const uint32_t v = (uint32_t)data[pos] | ((uint32_t)data[pos + 1] << 8) | ((uint32_t)data[pos + 2] << 16) | ((uint32_t)data[pos + 3] << 24);
        pos += 4; return v;
    }
};

struct Tensor { size_t offset; uint32_t count; };

float valueAt(const uint8_t* data, const Tensor& t, size_t i)
{
    float f; memcpy(&f, data + t.offset + 4 * i, 4); /* the hosts this builds for are little-endian, like the file */
    return f;
}

} // namespace

Weights parse(const uint8_t* data, size_t size)
{
    Reader r{data, size, 0};
    const int32_t count = (int32_t)r.u32("the tensor count");
    if (count < 0) parseError("negative tensor count " + std::to_string(count));
    std::map<std::string, Tensor> tensors;
    for (int32_t i = 0; i < count; i++) {
        const std::string which = "tensor " + std::to_string(i);
        const uint32_t nameLen = r.u32(which + ": the name length");
        if (nameLen > 255u) parseError(which + ": name length " + std::to_string(nameLen) + " (at most 255)");
        r.need(nameLen, which + ": the name (" + std::to_string(nameLen) + " bytes)");
        const std::string name((const char*)data + r.pos, nameLen); r.pos += nameLen;
        Tensor t;
        t.count = r.u32(name + ": the element count");
        r.need((uint64_t)t.count * 4u, name + ": the data (" + std::to_string(t.count) + " values)");
        t.offset = r.pos; r.pos += (size_t)t.count * 4u;
        tensors[name] = t; /* a name given twice: the last one holds */
    }
    auto find = [&](const std::string& name) -> const Tensor& {
        const auto it = tensors.find(name);
        if (it == tensors.end()) parseError(name + ": missing tensor");
        return it->second;
    };
    Weights w;
    for (uint32_t l = 0; l < kLayers; l++) {
        const std::string base = kLayerNames[l], wn = base + "/weights";
        const bool norm = l + 1u < kLayers;
        Layer& L = w.layer[l];
        L.kernel = kKernel[l];
        const Tensor& filter = find(wn);
        const Tensor* scale = norm ? &find(base + "/BatchNorm/scale") : nullptr;
        const Tensor* shift = norm ? &find(base + "/BatchNorm/shift") : nullptr;
        L.out = norm ? scale->count : 3u;
        if (L.out < 1u || L.out > kMaxFileChannels) parseError(base + "/BatchNorm/scale: " + std::to_string(L.out) + " output channels are outside 1 ... " +
            std::to_string(kMaxFileChannels));
        if (norm && shift->count != L.out) parseError(base + "/BatchNorm/shift: " + std::to_string(shift->count) + " values for " + std::to_string(L.out) +
            " output channels");
        const uint32_t per = L.out * L.kernel * L.kernel;
        if (filter.count % per) parseError(wn + ": " + std::to_string(filter.count) + " values do not divide into " + std::to_string(L.out) + " output channels of " +
            std::to_string(L.kernel) + " x " + std::to_string(L.kernel) + " taps");
        L.in = filter.count / per;
        if (L.in < 1u || L.in > kMaxFileChannels) parseError(wn + ": " + std::to_string(L.in) + " input channels are outside 1 ... " + std::to_string(kMaxFileChannels));
        const uint32_t expected = l ? w.layer[l - 1u].out : 3u;
        if (L.in != expected) parseError(wn + ": the graph does not close: " + std::to_string(L.in) + " input channels, " +
            (l ? std::string(kLayerNames[l - 1u]) : std::string("the picture")) + " gives " + std::to_string(expected));
        L.weight.resize(filter.count);
        const size_t perOut = (size_t)L.in * L.kernel * L.kernel;
        for (uint32_t o = 0; o < L.out; o++) {
            const float s = norm ? valueAt(data, *scale, o) : 1.0f;
            for (size_t i = 0; i < perOut; i++) {
                const float f = valueAt(data, filter, o * perOut + i);
                L.weight[o * perOut + i] = compress(norm ? f * s : f);
            }
            if (norm) L.bias.push_back(compress(valueAt(data, *shift, o)));
        }
    }
    return w;
}

Weights read(const char* path)
{
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) throw tbnn::Error{TB_E_IO, std::string("cannot open ") + (path ? path : "(null)")};
    std::vector<uint8_t> bytes;
    uint8_t chunk[65536]; size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) throw tbnn::Error{TB_E_IO, std::string("cannot read ") + path};
    return parse(bytes.data(), bytes.size());
}

} // namespace tbsr

namespace {

template <class F> int reported(char* err, uint32_t errLen, F f)
{
    auto say = [&](const std::string& m) { if (err && errLen) { snprintf(err, errLen, "%s", m.c_str()); } };
    try { return f(say); }
    catch (const tbnn::Error& e) { say(e.message); return e.code; }
    catch (const std::exception& e) { say(e.what()); return TB_E_PARSE; }
}

} // namespace

extern "C" int tb_sr_weights_info(const char* path, tb_sr_info* out, char* err, uint32_t errLen)
{
    return reported(err, errLen, [&](auto say) {
        if (!path || !out) { say("tb_sr_weights_info: null pointer"); return (int)TB_E_INVALID; }
        const tbsr::Weights w = tbsr::read(path);
        memset(out, 0, sizeof *out);
        for (uint32_t l = 0; l < tbsr::kLayers; l++) { out->in_channels[l] = w.layer[l].in; out->out_channels[l] = w.layer[l].out; out->kernel[l] = w.layer[l].kernel; }
        out->weight_bytes = w.weightBytes();
        return (int)TB_OK;
    });
}

extern "C" int tb_sr_read_layer(const char* path, uint32_t layer, uint16_t* weight, uint16_t* bias, char* err, uint32_t errLen)
{
    return reported(err, errLen, [&](auto say) {
        if (!path || !weight) { say("tb_sr_read_layer: null pointer"); return (int)TB_E_INVALID; }
        if (layer >= tbsr::kLayers) { say("tb_sr_read_layer: layer " + std::to_string(layer) + " (the network has 7)"); return (int)TB_E_INVALID; }
        const tbsr::Weights w = tbsr::read(path);
        const tbsr::Layer& L = w.layer[layer];
        memcpy(weight, L.weight.data(), L.weight.size() * sizeof(uint16_t));
        if (bias && !L.bias.empty()) memcpy(bias, L.bias.data(), L.bias.size() * sizeof(uint16_t));
        return (int)TB_OK;
    });
}
