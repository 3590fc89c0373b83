/* nn_weights.cpp -- reads the weights of the still denoiser's U-Net from a TZA container (include/tracerboy_hip.h
 * tb_nn_weights_info) and repacks a layer for the convolution kernel.  Host only: no HIP header, no context.
 *
 * The container, all values little-endian:
 *   header   u16 magic 0x41D7, u8 major version (2), u8 minor version, u64 offset of the table
 *   table    u32 tensor count, then per tensor: u16 name length, the name, u8 ndims, ndims x u32 dims, ndims layout characters ("oihw" / "x"),
 *            one character for the type ('h' binary16, 'f' binary32), u64 offset of the data
 * Every read is checked against the file's length first; nothing is trusted. */
#include "nn_weights.h"
#include "tracerboy_hip.h"

#include <cstdio>
#include <cstring>
#include <map>

namespace tbnn {

const char* const kLayerNames[kLayers] = {"enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5a", "enc_conv5b", "dec_conv4a",
    "dec_conv4b", "dec_conv3a", "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "dec_conv0"};

uint16_t halfFromFloat(float f)
{
    uint32_t u; memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    if (e == 0xffu) return (uint16_t)(sign | 0x7c00u | (m ? 0x200u | (m >> 13) : 0u)); /* infinity; NaN stays NaN (quiet) */
    if (e > 142u) return (uint16_t)(sign | 0x7c00u);                                    /* 2^16 and above */
    if (e < 102u) return (uint16_t)sign;                                                /* below 2^-25: zero (2^-25 itself ties to even = zero, below) */
    uint32_t mant, shift, base;
    if (e >= 113u) { mant = m; shift = 13u; base = (e - 112u) << 10; }                  /* normal: 10 bits kept of 23 */
    else { mant = 0x800000u | m; shift = 126u - e; base = 0u; }                         /* subnormal: the implicit one shifts in */
    uint32_t r = base + (mant >> shift);
    const uint32_t rest = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rest > half || (rest == half && (r & 1u))) r++;                                 /* a carry runs into the exponent, up to infinity, as it should */
    return (uint16_t)(sign | r);
}

float floatFromHalf(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0x1fu) u = sign | 0x7f800000u | (m << 13);
    else if (e) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (!m) u = sign;
    else { uint32_t mm = m, ee = 113u; while (!(mm & 0x400u)) { mm <<= 1; ee--; } u = sign | (ee << 23) | ((mm & 0x3ffu) << 13); }
    float f; memcpy(&f, &u, 4); return f;
}

uint64_t Weights::weightBytes() const
{
    uint64_t n = 0;
    for (const Layer& l : layer) n += (uint64_t)(l.weight.size() + l.bias.size()) * 2u;
    return n;
}

namespace {

[[noreturn]] void parseError(const std::string& m) { throw Error{TB_E_PARSE, "TZA: " + m}; }

struct Reader {
    const uint8_t* data; size_t size, pos;
    void need(size_t n, const std::string& what) const { if (n > size - pos) parseError(what + " runs past the end of the file"); }
    uint64_t uint(size_t bytes, const std::string& what)
    {
        need(bytes, what);
        uint64_t v = 0; for (size_t i = 0; i < bytes; i++) v |= (uint64_t)data[pos + i] << (8u * i);
        pos += bytes; return v;
    }
};

struct Tensor { std::vector<uint32_t> dims; std::string layout; char type; uint64_t offset, count; };

/* the tensor's values as binary16 bits */
std::vector<uint16_t> values(const uint8_t* data, const Tensor& t)
{
    std::vector<uint16_t> v((size_t)t.count);
    const uint8_t* p = data + t.offset;
    for (size_t i = 0; i < v.size(); i++) {
        if (t.type == 'h') v[i] = (uint16_t)(p[2 * i] | (p[2 * i + 1] << 8));
        else { const uint32_t u = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
            float f; memcpy(&f, &u, 4); v[i] = halfFromFloat(f); }
    }
    return v;
}

} // namespace

Weights parseTza(const uint8_t* data, size_t size)
{
    Reader r{data, size, 0};
    if (size < 12) parseError("the header runs past the end of the file (" + std::to_string(size) + " bytes)");
    const uint32_t magic = (uint32_t)r.uint(2, "header");
    if (magic != 0x41D7u) parseError("bad magic number");
    const uint32_t major = (uint32_t)r.uint(1, "header"); (void)r.uint(1, "header");
    if (major != 2u) parseError("unsupported version " + std::to_string(major) + " (the major version must be 2)");
    const uint64_t table = r.uint(8, "header");
    if (table > size || size - table < 4) parseError("the table offset " + std::to_string(table) + " runs past the end of the file");
    r.pos = (size_t)table;
    const uint64_t count = r.uint(4, "tensor count");
    const uint64_t kMinRecord = 2 + 1 + 1 + 8; /* an empty name and no dimension */
    if (count > (size - r.pos) / kMinRecord) parseError("the table of " + std::to_string(count) + " tensors runs past the end of the file");
    std::map<std::string, Tensor> tensors;
    for (uint64_t i = 0; i < count; i++) {
        const std::string which = "tensor " + std::to_string(i);
        const size_t nameLen = (size_t)r.uint(2, which + ": name length");
        r.need(nameLen, which + ": the name (" + std::to_string(nameLen) + " bytes)");
        const std::string name((const char*)data + r.pos, nameLen); r.pos += nameLen;
        Tensor t;
        const uint32_t nd = (uint32_t)r.uint(1, name + ": ndims");
        t.count = 1;
        for (uint32_t d = 0; d < nd; d++) {
            t.dims.push_back((uint32_t)r.uint(4, name + ": dims"));
            if (t.dims.back() && t.count > (1ull << 40) / t.dims.back()) parseError(name + ": the dimensions overflow");
            t.count *= t.dims.back();
        }
        r.need(nd, name + ": layout"); t.layout.assign((const char*)data + r.pos, nd); r.pos += nd;
        t.type = (char)r.uint(1, name + ": data type");
        t.offset = r.uint(8, name + ": data offset");
        if (t.type != 'h' && t.type != 'f') parseError(name + ": unknown data type (binary16 'h' and binary32 'f' are read)");
        const uint64_t bytes = t.count * (t.type == 'h' ? 2u : 4u);
        if (t.offset > size || bytes > size - t.offset) parseError(name + ": the data (" + std::to_string(bytes) + " bytes at offset " +
            std::to_string(t.offset) + ") runs past the end of the file");
        tensors[name] = t; /* a name given twice: the last one holds */
    }
    Weights w;
    for (uint32_t l = 0; l < kLayers; l++) {
        const std::string wn = std::string(kLayerNames[l]) + ".weight", bn = std::string(kLayerNames[l]) + ".bias";
        const auto wi = tensors.find(wn), bi = tensors.find(bn);
        if (wi == tensors.end()) parseError(wn + ": missing tensor");
        if (bi == tensors.end()) parseError(bn + ": missing tensor");
        const Tensor& wt = wi->second; const Tensor& bt = bi->second;
        if (wt.layout != "oihw") parseError(wn + ": wrong layout \"" + wt.layout + "\" (oihw is read)");
        if (bt.layout != "x") parseError(bn + ": wrong layout \"" + bt.layout + "\" (x is read)");
        if (wt.dims[2] != 3u || wt.dims[3] != 3u) parseError(wn + ": wrong kernel size " + std::to_string(wt.dims[2]) + " x " + std::to_string(wt.dims[3]) +
            " (3 x 3 is read)");
        Layer& L = w.layer[l];
        L.out = wt.dims[0]; L.in = wt.dims[1];
        if (L.out < 1u || L.out > kMaxFileChannels || L.in < 1u || L.in > kMaxFileChannels) parseError(wn + ": channel counts " + std::to_string(L.out) +
            " x " + std::to_string(L.in) + " are outside 1 ... " + std::to_string(kMaxFileChannels));
        if (bt.dims[0] != L.out) parseError(bn + ": " + std::to_string(bt.dims[0]) + " values for " + std::to_string(L.out) + " output channels");
        L.weight = values(data, wt); L.bias = values(data, bt);
    }
    /* the graph closes: a layer reads its predecessor, a decoder's first layer the upsampled tensor in front of the skip tensor of its size */
    enum { E0, E1, E2, E3, E4, E5A, E5B, D4A, D4B, D3A, D3B, D2A, D2B, D1A, D1B, D0 };
    const Layer* L = w.layer;
    auto expect = [&](uint32_t l, uint32_t in, const std::string& why) {
        if (L[l].in != in) parseError(std::string(kLayerNames[l]) + ".weight: the graph does not close: " + std::to_string(L[l].in) +
            " input channels, " + why + " gives " + std::to_string(in));
    };
    if (L[E0].in != 3u && L[E0].in != 9u) parseError("enc_conv0.weight: " + std::to_string(L[E0].in) + " input channels (3 or 9 are read)");
    for (uint32_t l : {E1, E2, E3, E4, E5A, E5B, D4B, D3B, D2B, D1B, D0}) expect(l, L[l - 1].out, std::string(kLayerNames[l - 1]));
    expect(D4A, L[E5B].out + L[E3].out, "enc_conv5b + enc_conv3");
    expect(D3A, L[D4B].out + L[E2].out, "dec_conv4b + enc_conv2");
    expect(D2A, L[D3B].out + L[E1].out, "dec_conv3b + enc_conv1");
    expect(D1A, L[D2B].out + L[E0].in, "dec_conv2b + the input");
    if (L[D0].out != 3u) parseError("dec_conv0.weight: " + std::to_string(L[D0].out) + " output channels (the picture has 3)");
    return w;
}

Weights readTza(const char* path)
{
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) throw Error{TB_E_IO, std::string("cannot open ") + (path ? path : "(null)")};
    std::vector<uint8_t> bytes;
    uint8_t chunk[65536]; size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) throw Error{TB_E_IO, std::string("cannot read ") + path};
    return parseTza(bytes.data(), bytes.size());
}

PackedLayer packLayer(uint32_t cA, uint32_t cB, uint32_t cOut, const uint16_t* weightOihw, const uint16_t* bias, uint32_t taps)
{
    PackedLayer p;
    p.cA = cA; p.cB = cB; p.cOut = cOut;
    const uint32_t padA = roundUp(cA, 32u), padB = roundUp(cB, 32u), cIn = cA + cB;
    p.kBlocks = (padA + padB) / 32u; p.outPadded = roundUp(cOut, 32u);
    const uint32_t outBlocks = p.outPadded / 16u;
    p.weight.assign((size_t)taps * p.kBlocks * outBlocks * 64u * 8u, 0);
    p.bias.assign(p.outPadded, 0.0f);
    for (uint32_t o = 0; bias && o < cOut; o++) p.bias[o] = floatFromHalf(bias[o]);
    for (uint32_t tap = 0; tap < taps; tap++)
        for (uint32_t kb = 0; kb < p.kBlocks; kb++)
            for (uint32_t ob = 0; ob < outBlocks; ob++)
                for (uint32_t lane = 0; lane < 64u; lane++)
                    for (uint32_t j = 0; j < 8u; j++) {
                        const uint32_t o = ob * 16u + (lane & 15u), k = kb * 32u + 8u * (lane >> 4) + j;
                        /* k counts padded channels: A's, then B's */
                        uint32_t i;
                        if (k < padA) { if (k >= cA) continue; i = k; } else { if (k - padA >= cB) continue; i = cA + (k - padA); }
                        if (o >= cOut) continue;
                        p.weight[((((size_t)tap * p.kBlocks + kb) * outBlocks + ob) * 64u + lane) * 8u + j] = weightOihw[((size_t)o * cIn + i) * taps + tap];
                    }
    return p;
}

} // namespace tbnn

extern "C" int tb_nn_weights_info(const char* path, tb_nn_info* out, char* err, uint32_t errLen)
{
    auto say = [&](const std::string& m) { if (err && errLen) { snprintf(err, errLen, "%s", m.c_str()); } };
    if (!path || !out) { say("tb_nn_weights_info: null pointer"); return TB_E_INVALID; }
    try {
        const tbnn::Weights w = tbnn::readTza(path);
        memset(out, 0, sizeof *out);
        out->in_channels = w.layer[0].in;
        for (uint32_t l = 0; l < tbnn::kLayers; l++) { out->out_channels[l] = w.layer[l].out; out->in_channels_of[l] = w.layer[l].in; }
        out->weight_bytes = w.weightBytes();
        return TB_OK;
    } catch (const tbnn::Error& e) { say(e.message); return e.code; }
    catch (const std::exception& e) { say(e.what()); return TB_E_PARSE; }
}
