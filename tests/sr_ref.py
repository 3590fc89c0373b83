"""The neural 2 x super-resolution restated on the CPU (include/tracerboy_hip.h, the super-resolution section).

Three things:
  * compress: the reference's binary32 -> binary16 conversion (Float16Compressor::compress), restated from its definition in numpy integer
    arithmetic, independent of csrc/host/sr_weights.cpp; fold: a layer's batch-norm scale multiplied into its filter, then compress;
  * a writer and a reader of the weights container, written from its layout;
  * the layer arithmetic (conv_ref / conv_scale, from tests/nn_layer_ref.py) and the network's graph in torch: net_ref, and net_chain, the same
    graph through the library's seams.

Tensors are numpy float16, NHWC without a batch axis, (H, W, C); weights are (o, i, K, K).
"""
import os
import struct

import numpy as np
import torch

from nn_layer_ref import conv_ref, conv_scale      # the layer, restated once for both networks

LAYERS = ("conv1", "conv2", "conv3", "conv_up1/conv", "conv4", "conv5", "conv6")
KERNEL = (5, 3, 3, 5, 3, 3, 3)
REAL_IN = (3, 32, 64, 64, 32, 32, 32)
REAL_OUT = (32, 64, 64, 32, 32, 32, 3)
SMALL_OUT = (5, 9, 7, 11, 6, 33, 3)      # odd channel counts; one past a k-block
REAL_WEIGHTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dml_sr", "weights.bin")
REAL_BYTES = 515339


# ---- the conversion --------------------------------------------------------------------------------

def compress(values):
    """float32 array -> uint16 array of binary16 bits, as the reference converts: the sign is set aside; a magnitude below 2^-14 becomes
    trunc(|v| * 2^37) (as an integer, below 2^23), one between 65504 and infinity becomes infinity, a NaN below 0x7F802000 becomes that; then
    the bits are shifted right by 13, 0x1C000 is subtracted where they exceed 0x23BFF, and again where they (then) exceed 0x3FF."""
    v = np.ascontiguousarray(values, np.float32)
    u = v.view(np.uint32).astype(np.int64)
    sign = u & 0x80000000
    a = u ^ sign
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = (np.abs(v) * np.float32(2.0 ** 37))
        sub = np.where(a < 0x38800000, scaled, 0).astype(np.int64)          # float32 product (exact: a power of two), truncated
    a = np.where(a < 0x38800000, sub, a)
    a = np.where((a > 0x477FE000) & (a < 0x7F800000), 0x7F800000, a)
    a = np.where((a > 0x7F800000) & (a < 0x7F802000), 0x7F802000, a)
    a = a >> 13
    a = np.where(a > 0x23BFF, a - 0x1C000, a)
    a = np.where(a > 0x3FF, a - 0x1C000, a)
    return ((a | (sign >> 16)) & 0xFFFF).astype(np.uint16)


def fold(weight, scale=None, shift=None):
    """(weight (o, i, K, K) float16, bias (o,) float16 or None) of float32 tensors: filter * scale[o] as one float32 multiply, compressed"""
    w = np.asarray(weight, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if scale is not None:
            w = w * np.asarray(scale, np.float32)[:, None, None, None]
    return compress(w).view(np.float16), None if shift is None else compress(np.asarray(shift, np.float32)).view(np.float16)


# ---- the container ---------------------------------------------------------------------------------
# little-endian: int32 tensor count; per tensor u32 name length, the name, u32 element count, that many float32

def container_bytes(tensors, count=None):
    """tensors: [(name, float32 array)] in this order"""
    blob = struct.pack("<i", len(tensors) if count is None else count)
    for name, a in tensors:
        a = np.ascontiguousarray(a, "<f4")
        blob += struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", a.size) + a.tobytes()
    return blob


def raw_tensors(raw, order=None):
    """raw: {layer: (filter (o, i, K, K) float32, scale or None, shift or None)} -> the tensor list, layers in `order`"""
    t = []
    for name in (order or LAYERS):
        w, scale, shift = raw[name]
        t.append((name + "/weights", w))
        if scale is not None:
            t += [(name + "/BatchNorm/scale", scale), (name + "/BatchNorm/shift", shift)]
    return t


def write_container(path, raw, order=None):
    with open(path, "wb") as f:
        f.write(container_bytes(raw_tensors(raw, order)))


def read_container(path):
    """{tensor name: flat float32 array}"""
    d = open(path, "rb").read()
    (n,), p, out = struct.unpack_from("<i", d, 0), 4, {}
    for _ in range(n):
        (ln,) = struct.unpack_from("<I", d, p); p += 4
        name = d[p:p + ln].decode(); p += ln
        (cnt,) = struct.unpack_from("<I", d, p); p += 4
        out[name] = np.frombuffer(d, "<f4", cnt, p).copy(); p += 4 * cnt
    return out


def folded_of(tensors, c_in=REAL_IN, c_out=REAL_OUT):
    """read_container's dictionary as {layer: (weight float16, bias float16 or None)}"""
    w = {}
    for name, i, o, k in zip(LAYERS, c_in, c_out, KERNEL):
        f = tensors[name + "/weights"].reshape(o, i, k, k)
        w[name] = fold(f, tensors.get(name + "/BatchNorm/scale"), tensors.get(name + "/BatchNorm/shift"))
    return w


def in_channels(out):
    return (3,) + tuple(out[:-1])


def make_raw(out, seed):
    """float32 tensors of a net with the output channels `out`: He-scaled filters (variance 2 / fan-in), scales near 1, small shifts of both
    signs; a small last layer, since it is a residual"""
    rng = np.random.default_rng(seed)
    raw = {}
    for l, (name, i, o, k) in enumerate(zip(LAYERS, in_channels(out), out, KERNEL)):
        f = (rng.standard_normal((o, i, k, k)) * np.sqrt(2.0 / (k * k * i))).astype(np.float32)
        if l == 6:
            raw[name] = (f * np.float32(0.25), None, None)
        else:
            raw[name] = (f, (0.75 + 0.5 * rng.random(o)).astype(np.float32), (rng.standard_normal(o) * 0.05).astype(np.float32))
    return raw


def folded_raw(raw):
    return {name: fold(*raw[name]) for name in LAYERS}


# ---- the layer and the graph -----------------------------------------------------------------------

def pack_input(color):
    """The network's input: .xyz of an (H, W, 4) float32 surface rounded to binary16 (nearest even)"""
    with np.errstate(over="ignore"):
        return np.asarray(color, np.float32)[..., :3].astype(np.float16)


def upsample2(x):
    return np.repeat(np.repeat(x, 2, 0), 2, 1)


def finish_ref(residual, picture):
    """|half(residual + picture nearest-upsampled x 2)| and alpha 1 as (2 H, 2 W, 4) float32: the sum is exact in float64, and numpy rounds a
    float64 to binary16 once"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.asarray(residual, np.float16).astype(np.float64) + upsample2(np.asarray(picture, np.float16)).astype(np.float64)).astype(np.float16)
    out = np.ones(s.shape[:2] + (4,), np.float32)
    out[..., :3] = np.abs(s).astype(np.float32)
    return out


def _graph(layer, x):
    """the seven layers in the order they run; layer(l, in_a, upsample_a) -> tensor"""
    t = layer(2, layer(1, layer(0, x, False), False), False)
    t = layer(3, t, True)
    return layer(6, layer(5, layer(4, t, False), False), False)


def net_ref(weights, x, accumulate=torch.float32):
    """The network on a packed input (H, W, 3) float16 -> (2 H, 2 W, 4) float32"""
    conv6 = _graph(lambda l, a, up: conv_ref(a, *weights[LAYERS[l]], upsample_a=up, relu=l < 6, accumulate=accumulate), x)
    return finish_ref(conv6, x)


def net_chain(tb, weights, x, form=0):
    """The same graph as seven calls of the library's layer seam (TracerBoy.RunConv) and its residual add (TracerBoy.RunSrFinish); a layer of
    more than 64 input channels runs in the plain form whatever `form` says, as in the library"""
    conv6 = _graph(lambda l, a, up: tb.RunConv(a, *weights[LAYERS[l]], upsample_a=up, relu=l < 6, form=form if a.shape[2] <= 64 else 0), x)
    return tb.RunSrFinish(conv6, x)
