"""The TZA weights reader of the neural still denoiser (csrc/host/nn_weights.cpp, tb_nn_weights_info): host only, no device.

The fixture is OIDN's rt_ldr_alb_nrm.tza (tests/golden/oidn/, joined from its two parts); the other files come from the writer of
tests/neural_ref.py, which shares no code with the library's reader."""
import struct

import numpy as np
import pytest

import neural_ref as nr

TB_E_IO, TB_E_PARSE = -3, -4


@pytest.fixture(scope="module")
def api(built):
    from tracerboy_amd import api
    return api


@pytest.fixture(scope="module")
def small():
    return nr.make_weights(9, nr.SMALL_OUT, seed=5)


def info_of(api, tmp_path, data, name="w.tza"):
    p = tmp_path / name
    p.write_bytes(data)
    return api.NeuralWeightsInfo(str(p))


def refused(api, tmp_path, data, *words):
    with pytest.raises(api.TracerBoyError) as e:
        info_of(api, tmp_path, data)
    assert e.value.code == TB_E_PARSE, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def test_the_fixture_has_oidn_channel_counts(api, tmp_path):
    """tb_nn_weights_info on rt_ldr_alb_nrm.tza; the Python reader agrees on every tensor's shape and on the largest weight"""
    path = nr.real_weights_file(tmp_path)
    i = api.NeuralWeightsInfo(path)
    assert i.in_channels == 9 and tuple(i.out_channels) == nr.OIDN_OUT == (32, 32, 48, 64, 80, 96, 96, 112, 112, 96, 96, 64, 64, 64, 32, 3)
    assert list(i.in_channels_of) == nr.in_channels(9, nr.OIDN_OUT) == [9, 32, 32, 48, 64, 80, 96, 160, 112, 160, 96, 128, 64, 73, 64, 32]
    w = nr.weights_of(nr.read_tza(path))
    assert [w[n][0].shape for n in nr.LAYERS] == [(o, c, 3, 3) for o, c in zip(i.out_channels, i.in_channels_of)]
    assert i.weight_bytes == sum(a.nbytes + b.nbytes for a, b in w.values()) == 1839622
    assert float(np.abs(w["enc_conv0"][0].astype(np.float32)).max()) == 18.5
    # cut anywhere, it is a parse error, not a crash
    data = open(path, "rb").read()
    for c in (11, 4096, len(data) // 2, len(data) - 1):
        refused(api, tmp_path, data[:c], "past the end")


def test_a_file_with_oidn_channel_counts_reads_back(api, tmp_path):
    """the channel counts of the reference's two files: 9 or 3 inputs, nr.OIDN_OUT"""
    for c_in in (9, 3):
        w = nr.make_weights(c_in, nr.OIDN_OUT, seed=c_in)
        i = info_of(api, tmp_path, nr.tza_bytes(nr.weight_tensors(w)))
        assert i.in_channels == c_in and tuple(i.out_channels) == nr.OIDN_OUT
        assert list(i.in_channels_of) == nr.in_channels(c_in, nr.OIDN_OUT)
        assert list(i.in_channels_of)[nr.D4A:nr.D1A + 1:2] == [160, 160, 128, 64 + c_in]
        assert i.weight_bytes == sum(a.nbytes + b.nbytes for a, b in w.values())
    assert i.weight_bytes == 1829254   # rt_ldr.tza's; rt_ldr_alb_nrm.tza has 6 x 32 x 9 more weights


def test_odd_channel_counts_f32_tensors_and_shuffled_order(api, tmp_path):
    out = (5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 255, 3)
    w = nr.make_weights(3, out, seed=11)
    order = list(nr.LAYERS); np.random.default_rng(3).shuffle(order)
    i = info_of(api, tmp_path, nr.tza_bytes(nr.weight_tensors(w, order=order, f32=("enc_conv2", "dec_conv0", "dec_conv3a"))))
    assert i.in_channels == 3 and tuple(i.out_channels) == out and list(i.in_channels_of) == nr.in_channels(3, out)
    assert i.weight_bytes == sum(a.nbytes + b.nbytes for a, b in w.values())   # binary32 tensors count as the binary16 they become
    # bias before weight, and an extra tensor the reader has no use for
    t = nr.weight_tensors(w)
    t = t[1::2] + t[0::2] + [("extra.scale", np.ones(4, np.float32), "x")]
    assert tuple(info_of(api, tmp_path, nr.tza_bytes(t)).out_channels) == out
    # and the Python reader, which the GPU tests take the fixture's weights from, reads back what the writer wrote (binary32 rounded to binary16)
    back = nr.weights_of(nr.read_tza(str(tmp_path / "w.tza")))
    assert all(np.array_equal(back[n][0], w[n][0]) and np.array_equal(back[n][1], w[n][1]) for n in nr.LAYERS)


def test_missing_file_is_an_io_error(api, tmp_path):
    with pytest.raises(api.TracerBoyError) as e:
        api.NeuralWeightsInfo(str(tmp_path / "absent.tza"))
    assert e.value.code == TB_E_IO


def test_wrong_magic_and_version(api, tmp_path, small):
    t = nr.weight_tensors(small)
    refused(api, tmp_path, nr.tza_bytes(t, magic=0x41D8), "magic")
    refused(api, tmp_path, nr.tza_bytes(t, major=3), "version", "3")
    assert info_of(api, tmp_path, nr.tza_bytes(t, minor=7)).in_channels == 9   # the minor version is free


def test_offsets_past_the_end(api, tmp_path, small):
    good = bytearray(nr.tza_bytes(nr.weight_tensors(small)))
    (table,) = struct.unpack_from("<Q", good, 4)
    for off in (len(good), len(good) - 3, len(good) + 1000, 2 ** 64 - 2):
        bad = bytearray(good); struct.pack_into("<Q", bad, 4, off)
        refused(api, tmp_path, bytes(bad), "table offset", "past the end")
    # the first tensor's data offset is the last 8 bytes of its record
    first = "enc_conv0.weight"
    rec_end = table + 4 + 2 + len(first) + 1 + 16 + 4 + 1 + 8
    for off in (len(good) - 10, len(good), 2 ** 63, 2 ** 64 - 1):
        bad = bytearray(good); struct.pack_into("<Q", bad, rec_end - 8, off)
        refused(api, tmp_path, bytes(bad), first, "past the end")
    # a name length that runs past the end
    bad = bytearray(good); struct.pack_into("<H", bad, table + 4, 0xffff)
    refused(api, tmp_path, bytes(bad), "name", "past the end")
    # a tensor count that the file cannot hold (count x record would overflow 32 bits)
    bad = bytearray(good); struct.pack_into("<I", bad, table, 0xffffffff)
    refused(api, tmp_path, bytes(bad), "4294967295 tensors", "past the end")
    # dimensions whose product overflows
    bad = bytearray(good); struct.pack_into("<4I", bad, table + 4 + 2 + len(first) + 1, 0xffffffff, 0xffffffff, 3, 3)
    refused(api, tmp_path, bytes(bad), first)


def test_wrong_tensors(api, tmp_path, small):
    t = nr.weight_tensors(small)
    refused(api, tmp_path, nr.tza_bytes([x for x in t if x[0] != "dec_conv2a.bias"]), "dec_conv2a.bias", "missing")
    five = [(n, np.zeros(a.shape[:2] + (5, 5), np.float16), l) if n == "enc_conv3.weight" else (n, a, l) for n, a, l in t]
    refused(api, tmp_path, nr.tza_bytes(five), "enc_conv3.weight", "kernel size", "5 x 5")
    ohwi = [(n, a, "ohwi") if n == "enc_conv4.weight" else (n, a, l) for n, a, l in t]
    refused(api, tmp_path, nr.tza_bytes(ohwi), "enc_conv4.weight", "layout", "ohwi")
    short_bias = [(n, a[:-1], l) if n == "enc_conv4.bias" else (n, a, l) for n, a, l in t]
    refused(api, tmp_path, nr.tza_bytes(short_bias), "enc_conv4.bias")


def test_graphs_that_do_not_close(api, tmp_path, small):
    def with_weight(name, shape):
        return nr.tza_bytes([(n, np.zeros(shape, np.float16), l) if n == name + ".weight" else
                             (n, np.zeros(shape[0], np.float16), l) if n == name + ".bias" else (n, a, l) for n, a, l in nr.weight_tensors(small)])
    i = nr.in_channels(9, nr.SMALL_OUT)
    refused(api, tmp_path, with_weight("dec_conv1a", (16, i[nr.D1A] + 1, 3, 3)), "dec_conv1a", "does not close")
    refused(api, tmp_path, with_weight("dec_conv1a", (16, i[nr.D1A] - 1, 3, 3)), "dec_conv1a", "does not close")
    refused(api, tmp_path, with_weight("dec_conv0", (4, 8, 3, 3)), "dec_conv0", "4 output channels")
    refused(api, tmp_path, with_weight("enc_conv2", (12, 9, 3, 3)), "enc_conv2", "does not close")
    refused(api, tmp_path, with_weight("enc_conv5a", (257, 20, 3, 3)), "enc_conv5a", "256")
    four = nr.make_weights(4, nr.SMALL_OUT, seed=1)
    refused(api, tmp_path, nr.tza_bytes(nr.weight_tensors(four)), "enc_conv0", "3 or 9")


def test_truncated_files(api, tmp_path, small):
    """cut at 12 byte counts spread over the header, the data and the table: each is a parse error that names what ran past the end"""
    good = nr.tza_bytes(nr.weight_tensors(small))
    (table,) = struct.unpack_from("<Q", good, 4)
    n = len(good)
    cuts = [0, 1, 3, 11, 12, 64, table // 2, table - 1, table, table + 3, table + 4 + 7, (table + n) // 2, n - 9, n - 1]
    assert len(set(cuts)) >= 12 and all(0 <= c < n for c in cuts)
    for c in cuts:
        refused(api, tmp_path, good[:c], "past the end")
