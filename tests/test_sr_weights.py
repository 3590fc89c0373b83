"""The weights reader of the neural 2 x super-resolution (csrc/host/sr_weights.cpp: tb_sr_weights_info, tb_sr_read_layer): host only, no device.

The file is the reference's TracerBoy/ML/weights.bin (tests/golden/dml_sr/weights.bin) or one the test writes with tests/sr_ref.py, which shares no
code with the library's reader.  The folded binary16 values are compared bit for bit with sr_ref.fold: filter * scale[o] as one float32 multiply,
then the reference's conversion, which truncates where a rounding would round and gives infinity for everything above 65504."""
import struct

import numpy as np
import pytest

import sr_ref as sr

TB_E_IO, TB_E_PARSE = -3, -4


@pytest.fixture(scope="module")
def api(built):
    from tracerboy_amd import api
    return api


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def assert_layers_equal(api, path, folded, c_in, c_out):
    info = api.SrWeightsInfo(path)
    assert tuple(info.in_channels) == tuple(c_in) and tuple(info.out_channels) == tuple(c_out) and tuple(info.kernel) == sr.KERNEL
    total = 0
    for l, name in enumerate(sr.LAYERS):
        w, b = api.SrReadLayer(path, l)
        want_w, want_b = folded[name]
        assert w.shape == want_w.shape and np.array_equal(bits(w), bits(want_w)), name
        assert (b is None) == (want_b is None) and (b is None or np.array_equal(bits(b), bits(want_b))), name
        total += 2 * (w.size + (0 if b is None else b.size))
    assert info.weight_bytes == total


def test_the_reference_file(api):
    """channels 3/32/64/64/32/32/32 -> 32/64/64/32/32/32/3, K = 5, 3, 3, 5, 3, 3, 3; every folded value against the Python fold"""
    import os
    assert os.path.getsize(sr.REAL_WEIGHTS) == sr.REAL_BYTES
    tensors = sr.read_container(sr.REAL_WEIGHTS)
    assert len(tensors) == 19
    assert_layers_equal(api, sr.REAL_WEIGHTS, sr.folded_of(tensors), sr.REAL_IN, sr.REAL_OUT)
    folded = sr.folded_of(tensors)
    # the conversion is not a rounding: some of this file's values differ from nearest-even
    w = tensors["conv2/weights"].reshape(64, 32, 3, 3) * tensors["conv2/BatchNorm/scale"][:, None, None, None]
    assert (bits(folded["conv2"][0]) != bits(w.astype(np.float16))).any()


def edge_values():
    """float32 values on, and one float32 step either side of: binary16 values and the midpoints between them (normal and subnormal), the largest
    finite binary16 and the first float32 past it, 65520 (where a rounding would start to give infinity), 2^-14, 2^-24, 2^-25, float32 denormals,
    both zeros, infinities and NaNs of three payloads"""
    f32 = np.float32
    halves = np.array([0x0001, 0x0002, 0x01ff, 0x03ff, 0x0400, 0x0401, 0x3555, 0x3bff, 0x3c00, 0x3c01, 0x4248, 0x7bfe, 0x7bff], np.uint16).view(np.float16).astype(f32)
    with np.errstate(over="ignore"):
        ups = np.nextafter(halves.astype(np.float16), np.float16(np.inf)).astype(f32)
        mids = ((halves.astype(np.float64) + ups.astype(np.float64)) / 2).astype(f32)   # exact in float32; 65520 for the last
    base = np.concatenate([halves, mids, f32([2.0 ** -25, 2.0 ** -26, 1e-30, 1e-40, 1.4e-45, 65504.0, 65520.0, 65536.0, 1e10, 3.4e38])])
    v = np.concatenate([base, np.nextafter(base, f32(np.inf)), np.nextafter(base, f32(0))])
    special = np.array([0x00000000, 0x7F800000, 0x7F800001, 0x7F801FFF, 0x7F802000, 0x7FC00000, 0x7FFFFFFF], np.uint32).view(f32)
    v = np.concatenate([v, special])
    return np.concatenate([v, -v]).astype(f32)


def test_selfcheck_compress_truncates_toward_zero():
    """A self-check of sr_ref.compress, not of the library: for finite values up to 65504 the result is the binary16 value of largest magnitude
    that does not exceed the input's; above it, infinity; a NaN stays a NaN; the sign is kept"""
    v = edge_values()
    h = sr.compress(v).view(np.float16)
    assert np.array_equal(np.signbit(h), np.signbit(v))
    assert np.array_equal(np.isnan(h), np.isnan(v))
    big = np.abs(v) > 65504
    assert np.isinf(h[big & ~np.isnan(v)]).all()
    ok = ~big & ~np.isnan(v)
    m, hm = np.abs(v[ok]).astype(np.float64), np.abs(h[ok]).astype(np.float64)
    with np.errstate(over="ignore"):
        above = np.nextafter(np.abs(h[ok]), np.float16(np.inf)).astype(np.float64)
        rounded = v.astype(np.float16)
    assert (hm <= m).all() and (above > m).all()
    assert (h.view(np.uint16) != rounded.view(np.uint16)).any()       # and that is not what a rounding gives


def edge_net(seed):
    """a net with odd channel counts whose filters and shifts are the edge values, with scales that keep (1), halve (0.5: exact, moves values into
    the subnormals), perturb (1.0000001, 0.9999999, 3) and overflow (1e30, -2) the products"""
    raw = sr.make_raw(sr.SMALL_OUT, seed)
    rng = np.random.default_rng(seed)
    v = edge_values()
    scales = np.array([1.0, 0.5, 1.0000001, 0.9999999, 3.0, 1e30, -2.0, 2.0 ** -10], np.float32)
    for name in sr.LAYERS:
        f, scale, shift = raw[name]
        flat = f.reshape(f.shape[0], -1)
        for o in range(flat.shape[0]):
            take = rng.permutation(v.size)[:flat.shape[1]]
            flat[o, :take.size] = v[take]                       # every row a different sample; rows are shorter or longer than the edge list
        if scale is not None:
            scale[:] = scales[np.arange(scale.size) % scales.size]
            shift[:] = v[rng.permutation(v.size)[:shift.size]]
    return raw


def test_written_files_edge_values_odd_channels_shuffled_order(api, tmp_path):
    raw = edge_net(seed=5)
    for n, order in enumerate((None, tuple(reversed(sr.LAYERS)), ("conv4", "conv1", "conv6", "conv_up1/conv", "conv3", "conv5", "conv2"))):
        path = str(tmp_path / ("edge%d.bin" % n))
        sr.write_container(path, raw, order)
        with np.errstate(over="ignore", invalid="ignore"):
            assert_layers_equal(api, path, sr.folded_raw(raw), sr.in_channels(sr.SMALL_OUT), sr.SMALL_OUT)
    # every edge value went through the library's conversion on its own, too: a 3 -> N -> ... net whose first filter holds them with scale 1
    v = edge_values()
    out = (-(-v.size // 75), 4, 4, 4, 4, 4, 3)
    raw = sr.make_raw(out, seed=6)
    f = raw["conv1"][0].reshape(-1); f[:v.size] = v
    raw["conv1"] = (raw["conv1"][0], np.ones(out[0], np.float32), raw["conv1"][2])
    path = str(tmp_path / "all_edges.bin")
    sr.write_container(path, raw)
    w, _ = api.SrReadLayer(path, 0)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(w).reshape(-1)[:v.size], sr.compress(v * np.float32(1)))      # the multiply by the scale quiets a signalling NaN
    assert_layers_equal(api, path, sr.folded_raw(raw), sr.in_channels(out), out)


def refused(api, path, code, *words):
    with pytest.raises(api.TracerBoyError) as e:
        api.SrWeightsInfo(str(path))
    assert e.value.code == code and all(w in str(e.value) for w in words), (code, words, e.value.code, str(e.value))
    with pytest.raises(api.TracerBoyError) as e2:
        api.SrReadLayer(str(path), 0)
    assert e2.value.code == code


def test_malformed_files_are_refused_with_the_tensor_and_the_cause(api, tmp_path):
    raw = sr.make_raw(sr.SMALL_OUT, seed=7)
    tensors = sr.raw_tensors(raw)
    good = sr.container_bytes(tensors)

    def put(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        return p

    assert api.SrWeightsInfo(str(put("good.bin", good))).out_channels[5] == 33
    refused(api, tmp_path / "absent.bin", TB_E_IO, "cannot open")
    refused(api, put("negative.bin", sr.container_bytes(tensors, count=-1)), TB_E_PARSE, "negative")
    refused(api, put("more.bin", sr.container_bytes(tensors, count=len(tensors) + 1)), TB_E_PARSE, "tensor 19", "past the end")
    # a name length of 256; 255 is read (and then misses, as a name of that length is none of the network's)
    head = struct.pack("<i", 1)
    refused(api, put("name256.bin", head + struct.pack("<I", 256) + b"n" * 256 + struct.pack("<I", 0)), TB_E_PARSE, "256")
    refused(api, put("name255.bin", head + struct.pack("<I", 255) + b"n" * 255 + struct.pack("<I", 0)), TB_E_PARSE, "missing tensor")
    # an element count past the end
    first = "conv1/weights"
    count_at = 4 + 4 + len(first)
    huge = bytearray(good); huge[count_at:count_at + 4] = struct.pack("<I", 0xFFFFFFFF)
    refused(api, put("huge.bin", bytes(huge)), TB_E_PARSE, first, "past the end")
    one_more = bytearray(good[:count_at + 4 + 4 * raw["conv1"][0].size]); one_more[0:4] = struct.pack("<i", 1)
    one_more[count_at:count_at + 4] = struct.pack("<I", raw["conv1"][0].size + 1)
    refused(api, put("one_more.bin", bytes(one_more)), TB_E_PARSE, first, "past the end")
    # truncation inside each field: the count, a name length, a name, an element count, the data, and after any whole tensor
    for cut, word in ((0, "count"), (3, "count"), (4, "name length"), (6, "name length"), (8 + 3, "name"), (count_at + 2, "element count"),
                      (count_at + 4 + 10, "data"), (len(good) - 1, "data"), (len(good) - 4 * raw["conv6"][0].size, "data"),
                      (len(good) - 4 * raw["conv6"][0].size - 2, "element count")):
        refused(api, put("cut%d.bin" % cut, good[:cut]), TB_E_PARSE, word, "past the end")
    # a missing tensor of each kind
    for missing in ("conv3/weights", "conv_up1/conv/BatchNorm/scale", "conv5/BatchNorm/shift", "conv6/weights"):
        refused(api, put("missing.bin", sr.container_bytes([t for t in tensors if t[0] != missing])), TB_E_PARSE, missing, "missing")

    def with_tensor(name, array):
        return sr.container_bytes([(n, array if n == name else a) for n, a in tensors])

    # a count that does not divide by out * K^2
    refused(api, put("divide.bin", with_tensor("conv2/weights", np.zeros(9 * 5 * 9 + 1, np.float32))), TB_E_PARSE, "conv2/weights", "divide")
    refused(api, put("divide6.bin", with_tensor("conv6/weights", np.zeros(3 * 9 * 33 - 1, np.float32))), TB_E_PARSE, "conv6/weights", "divide")
    # a chain that does not close: a first layer of 4 inputs, a layer that reads more than its predecessor wrote
    refused(api, put("first4.bin", with_tensor("conv1/weights", np.zeros(5 * 4 * 25, np.float32))), TB_E_PARSE, "conv1/weights", "does not close")
    refused(api, put("chain.bin", with_tensor("conv3/weights", np.zeros(7 * 10 * 9, np.float32))), TB_E_PARSE, "conv3/weights", "does not close", "conv2")
    # shift and scale disagree; channel counts outside 1 ... 256
    refused(api, put("shift.bin", with_tensor("conv4/BatchNorm/shift", np.zeros(7, np.float32))), TB_E_PARSE, "conv4/BatchNorm/shift")
    refused(api, put("out0.bin", with_tensor("conv4/BatchNorm/scale", np.zeros(0, np.float32))), TB_E_PARSE, "conv4/BatchNorm/scale", "256")
    refused(api, put("out257.bin", with_tensor("conv4/BatchNorm/scale", np.zeros(257, np.float32))), TB_E_PARSE, "conv4/BatchNorm/scale", "256")
    refused(api, put("in0.bin", with_tensor("conv4/weights", np.zeros(0, np.float32))), TB_E_PARSE, "conv4/weights", "256")
    # trailing bytes after the last tensor are not read
    assert api.SrWeightsInfo(str(put("trailing.bin", good + b"xyz"))).in_channels[0] == 3


def test_null_arguments_and_layer_index(api, tmp_path):
    import ctypes as C
    L = api.lib()
    err = C.create_string_buffer(256)
    assert L.tb_sr_weights_info(None, None, err, 256) == -1 and b"null" in err.value
    w = np.empty(32 * 3 * 25, np.float16)
    assert L.tb_sr_read_layer(sr.REAL_WEIGHTS.encode(), 7, w.ctypes.data_as(C.c_void_p), None, err, 256) == -1 and b"layer 7" in err.value
    assert L.tb_sr_read_layer(sr.REAL_WEIGHTS.encode(), 0, w.ctypes.data_as(C.c_void_p), None, None, 0) == 0    # no bias asked, no message buffer
