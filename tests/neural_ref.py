"""The neural still denoiser restated on the CPU (include/tracerboy_hip.h, the neural section).

Three things:
  * the helper kernels around the layers: pack_input / extend16, rgba8_of (the 8-bit store) and unorm_color (its way back);
  * the layer arithmetic (conv_ref / conv_scale, from tests/nn_layer_ref.py) and the network's graph in torch: net_ref (and net_chain, the same
    graph through the library's layer seam);
  * a reader and a writer of the TZA weights container, written from its layout, independent of csrc/host/nn_weights.cpp.

Tensors are numpy float16, NHWC without a batch axis, (H, W, C); weights are (o, i, 3, 3).
"""
import os
import struct

import numpy as np
import torch

from nn_layer_ref import conv_ref, conv_scale      # the layer, restated once for both networks

LAYERS = ("enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5a", "enc_conv5b", "dec_conv4a", "dec_conv4b", "dec_conv3a",
          "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "dec_conv0")
E0, E1, E2, E3, E4, E5A, E5B, D4A, D4B, D3A, D3B, D2A, D2B, D1A, D1B, D0 = range(16)
# output channels of OIDN's rt_ldr_alb_nrm.tza / rt_ldr.tza, and of the small net the tests write
OIDN_OUT = (32, 32, 48, 64, 80, 96, 96, 112, 112, 96, 96, 64, 64, 64, 32, 3)
SMALL_OUT = (8, 8, 12, 16, 20, 24, 24, 28, 28, 24, 24, 16, 16, 16, 8, 3)


# OIDN's rt_ldr_alb_nrm.tza (1 841 160 bytes), kept under tests/golden/oidn/ as two parts that real_weights_file joins
REAL_PARTS = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oidn", "rt_ldr_alb_nrm.tza.part%d" % i) for i in range(2)]
REAL_BYTES = 1841160


def real_weights_file(directory):
    """The path of rt_ldr_alb_nrm.tza, joined from its committed parts into `directory`."""
    path = os.path.join(str(directory), "rt_ldr_alb_nrm.tza")
    data = b"".join(open(p, "rb").read() for p in REAL_PARTS)
    assert len(data) == REAL_BYTES
    with open(path, "wb") as f:
        f.write(data)
    return path


def in_channels(c_in, out):
    """The input channels of the 16 layers of a graph that closes: a layer reads its predecessor, a decoder's first layer the upsampled
    tensor in front of the skip tensor of its size (the last skip is the input itself)."""
    i = [c_in] + [out[l - 1] for l in range(1, 16)]
    i[D4A] = out[E5B] + out[E3]; i[D3A] = out[D4B] + out[E2]; i[D2A] = out[D3B] + out[E1]; i[D1A] = out[D2B] + c_in
    return i


def make_weights(c_in, out, seed):
    """{layer: (weight (o, i, 3, 3) float16, bias (o,) float16)}: He-scaled normal weights (variance 2 / fan-in, so that activations keep their
    scale through the ReLUs), small biases of both signs."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, i, o in zip(LAYERS, in_channels(c_in, out), out):
        w[name] = ((rng.standard_normal((o, i, 3, 3)) * np.sqrt(2.0 / (9 * i))).astype(np.float16), (rng.standard_normal(o) * 0.05).astype(np.float16))
    return w


# ---- the TZA container ---------------------------------------------------------------------------
# little-endian.  header: u16 magic 0x41D7, u8 major (2), u8 minor, u64 table offset.  table: u32 count, then per tensor u16 name length, name,
# u8 ndims, ndims x u32 dims, ndims layout characters, one type character ('h' binary16, 'f' binary32), u64 data offset.

def tza_bytes(tensors, magic=0x41D7, major=2, minor=0):
    """tensors: [(name, array, layout)], float16 arrays stored as 'h', float32 as 'f', in this order.  Data first (64-byte aligned), table last."""
    blob = bytearray(struct.pack("<HBBQ", magic, major, minor, 0))
    offsets = []
    for _, a, _ in tensors:
        blob += b"\0" * (-len(blob) % 64)
        offsets.append(len(blob))
        blob += np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<")).tobytes()
    table = len(blob)
    blob += struct.pack("<I", len(tensors))
    for (name, a, layout), off in zip(tensors, offsets):
        assert a.dtype in (np.float16, np.float32) and len(layout) == a.ndim
        blob += struct.pack("<H", len(name)) + name.encode() + struct.pack("<B", a.ndim) + struct.pack("<%dI" % a.ndim, *a.shape)
        blob += layout.encode() + (b"h" if a.dtype == np.float16 else b"f") + struct.pack("<Q", off)
    blob[4:12] = struct.pack("<Q", table)
    return bytes(blob)


def weight_tensors(weights, order=None, f32=()):
    """The tensor list of a weights dictionary; order: the layers' order in the file; f32: layers stored as binary32."""
    t = []
    for name in (order or LAYERS):
        w, b = weights[name]
        kind = np.float32 if name in f32 else np.float16
        t += [(name + ".weight", w.astype(kind), "oihw"), (name + ".bias", b.astype(kind), "x")]
    return t


def write_tza(path, weights, **kw):
    with open(path, "wb") as f:
        f.write(tza_bytes(weight_tensors(weights, **kw)))


def read_tza(path):
    """{tensor name: (array, layout)} of a TZA file."""
    d = open(path, "rb").read()
    magic, major, _, table = struct.unpack_from("<HBBQ", d, 0)
    assert magic == 0x41D7 and major == 2
    (n,), p, out = struct.unpack_from("<I", d, table), table + 4, {}
    for _ in range(n):
        (ln,) = struct.unpack_from("<H", d, p); p += 2
        name = d[p:p + ln].decode(); p += ln
        nd = d[p]; p += 1
        dims = struct.unpack_from("<%dI" % nd, d, p); p += 4 * nd
        layout = d[p:p + nd].decode(); p += nd
        kind = np.dtype("<f2") if d[p:p + 1] == b"h" else np.dtype("<f4"); p += 1
        (off,) = struct.unpack_from("<Q", d, p); p += 8
        out[name] = (np.frombuffer(d, kind, int(np.prod(dims)), off).reshape(dims).copy(), layout)
    return out


def weights_of(tensors):
    """read_tza's dictionary as a weights dictionary (binary32 tensors rounded to binary16, nearest even)."""
    return {name: (tensors[name + ".weight"][0].astype(np.float16), tensors[name + ".bias"][0].astype(np.float16)) for name in LAYERS}


# ---- the layer and the graph ---------------------------------------------------------------------

def pack_input(color, albedo=None, normal=None):
    """The network's input as the contract packs it: (H, W, 3 or 9) float16, channels colour.xyz, albedo.xyz, normal.xyz, rounded to nearest even."""
    planes = [np.asarray(s, np.float32)[..., :3] for s in (color, albedo, normal) if s is not None]
    with np.errstate(over="ignore"):
        return np.concatenate(planes, -1).astype(np.float16)


def rgba8_of(f):
    """The output stage's R8G8B8A8_UNORM store of an (H, W, 4) picture: NaN -> 0, clamp to [0, 1], * 255 + 0.5 in float32, truncate; alpha 255."""
    x = np.asarray(f, np.float32)[..., :3]
    x = np.where(np.isnan(x), np.float32(0), x)
    x = np.clip(x, np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0.5)
    out = np.full(np.asarray(f).shape, 255, np.uint8)
    out[..., :3] = x.astype(np.uint32)
    return out


def unorm_color(rgba8):
    """What a network loads from an R8G8B8A8_UNORM picture: k / 255 in float32 per channel, alpha 1.  (H, W, 4) uint8 -> float32."""
    out = np.ones(np.asarray(rgba8).shape, np.float32)
    out[..., :3] = np.asarray(rgba8)[..., :3].astype(np.float32) / np.float32(255)
    return out


def extend16(x):
    """zero-extended at the right and bottom to the next multiples of 16"""
    h, w = x.shape[:2]
    return np.pad(x, ((0, -h % 16), (0, -w % 16), (0, 0)))


def _graph(layer, x):
    """the 16 layers in the order they run; layer(l, in_a, in_b, upsample_a, pool) -> tensor"""
    e0 = layer(E0, x, None, False, False)
    p1 = layer(E1, e0, None, False, True)
    p2 = layer(E2, p1, None, False, True)
    p3 = layer(E3, p2, None, False, True)
    p4 = layer(E4, p3, None, False, True)
    t = layer(E5B, layer(E5A, p4, None, False, False), None, False, False)
    t = layer(D4B, layer(D4A, t, p3, True, False), None, False, False)
    t = layer(D3B, layer(D3A, t, p2, True, False), None, False, False)
    t = layer(D2B, layer(D2A, t, p1, True, False), None, False, False)
    t = layer(D1B, layer(D1A, t, x, True, False), None, False, False)
    return layer(D0, t, None, False, False)


def net_ref(weights, x, accumulate=torch.float32):
    """The network on a packed input (H, W, C) float16: zero-extended to multiples of 16, the 16 layers, cropped.  (H, W, 3) float16."""
    h, w = x.shape[:2]
    y = _graph(lambda l, a, b, up, pool: conv_ref(a, *weights[LAYERS[l]], in_b=b, upsample_a=up, pool=pool, accumulate=accumulate), extend16(x))
    return y[:h, :w]


def net_chain(tb, weights, x):
    """The same graph as 16 calls of the library's layer seam (TracerBoy.RunConv3x3) on the zero-extended packed input, cropped."""
    h, w = x.shape[:2]
    y = _graph(lambda l, a, b, up, pool: tb.RunConv3x3(a, *weights[LAYERS[l]], in_b=b, upsample_a=up, pool=pool, relu=True), extend16(x))
    return y[:h, :w]
