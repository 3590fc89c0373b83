"""The layers and networks of both neural stages give the bits they gave before nn_conv3x3 was retired.

Since the U-Net moved onto nn_convk, "tb_run_conv3x3 equals tb_run_conv with K = 3" holds by construction and proves nothing, so the outcome is
pinned against the code that was deleted: tests/golden/nn_parent_bits.json holds SHA-256 digests of the output bits of every case below, recorded
on an MI355X with the library of the commit before the move (scripts/record_nn_parent_bits.py, which runs these same cases -- cases() makes the
seeded inputs for the recording and for the test, so the two cannot drift).  The test asserts equal digests and nothing else.

The cases (shapes are width x height of the convolution's output):
  tb_run_conv3x3  9 -> 32 at 17 x 33; 32 -> 48 at 34 x 18 with pool; 64 upsampled + 9 -> 64 at 18 x 34; 96 upsampled + 64 -> 112 at 4 x 6;
                  32 -> 3 at 17 x 33 with and without ReLU; 5 -> 7 at 6 x 10; 3 -> 32 at 34 x 6 with pool (17 x 3 once pooled)
  tb_run_conv     K = 3 and 5, plain and staged: 3 -> 32 at 33 x 5; 64 -> 32 upsampled at 18 x 6; 32 -> 3 at 17 x 2 without bias and ReLU
  tb_run_neural   the small 9-input net of neural_ref.make_weights at 16 x 16 and 40 x 24
  tb_run_sr       the small net of sr_ref.make_raw at 17 x 9, plain and staged"""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import neural_ref as nr
import sr_ref as sr

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_parent_bits.json")


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _tensor(rng, w, h, c):
    return rng.random((h, w, c)).astype(np.float16)    # [0, 1)


def _he(rng, c_out, c_in, k):
    return (rng.standard_normal((c_out, c_in, k, k)) * np.sqrt(2.0 / (k * k * c_in))).astype(np.float16), (rng.standard_normal(c_out) * 0.1).astype(np.float16)


def _surfaces(rng, w, h, planes):
    return [np.concatenate([rng.random((h, w, 3), np.float32), np.ones((h, w, 1), np.float32)], -1) for _ in range(planes)]


def _layer(name, w, h, c_a, c_out, k=3, c_b=0, upsample_a=False, bias=True, **kw):
    """the seeded inputs of one layer case: (in_a, weight, bias or None, keywords of RunConv3x3 / RunConv)"""
    rng = _rng(name)
    a = _tensor(rng, w // 2, h // 2, c_a) if upsample_a else _tensor(rng, w, h, c_a)
    weight, b = _he(rng, c_out, c_a + c_b, k)
    return a, weight, b if bias else None, dict(kw, upsample_a=upsample_a, in_b=_tensor(rng, w, h, c_b) if c_b else None)


def cases():
    """[(name, run)]: run(tb, directory) -> the case's output array; directory is where a network's weights file is written"""
    out = []

    def conv3x3(name, *shape, **kw):
        def run(tb, directory):
            a, w, b, k = _layer(name, *shape, **kw)
            return tb.RunConv3x3(a, w, b, **k)
        out.append((name, run))

    def conv(name, *shape, **kw):
        for form in (0, 1):
            def run(tb, directory, form=form):
                a, w, b, k = _layer(name, *shape, **kw)      # the same inputs in both forms
                return tb.RunConv(a, w, b, form=form, **k)
            out.append(("%s_form%d" % (name, form), run))

    conv3x3("conv3x3_9_32_17x33", 17, 33, 9, 32)
    conv3x3("conv3x3_32_48_34x18_pool", 34, 18, 32, 48, pool=True)
    conv3x3("conv3x3_up64_9_64_18x34", 18, 34, 64, 64, c_b=9, upsample_a=True)
    conv3x3("conv3x3_up96_64_112_4x6", 4, 6, 96, 112, c_b=64, upsample_a=True)
    conv3x3("conv3x3_32_3_17x33_relu", 17, 33, 32, 3, relu=True)
    conv3x3("conv3x3_32_3_17x33_norelu", 17, 33, 32, 3, relu=False)
    conv3x3("conv3x3_5_7_6x10", 6, 10, 5, 7)
    conv3x3("conv3x3_3_32_34x6_pool", 34, 6, 3, 32, pool=True)
    for k in (3, 5):
        conv("conv_k%d_3_32_33x5" % k, 33, 5, 3, 32, k=k)
        conv("conv_k%d_up64_32_18x6" % k, 18, 6, 64, 32, k=k, upsample_a=True)
        conv("conv_k%d_32_3_17x2_nobias" % k, 17, 2, 32, 3, k=k, bias=False, relu=False)

    def neural(name, w, h):
        def run(tb, directory):
            path = os.path.join(str(directory), "parent_bits_small9.tza")
            nr.write_tza(path, nr.make_weights(9, nr.SMALL_OUT, seed=22))
            tb.LoadNeuralWeights(path)
            return tb.RunNeural(*_surfaces(_rng(name), w, h, 3))
        out.append((name, run))

    def upscale(name, w, h, form):
        def run(tb, directory):
            path = os.path.join(str(directory), "parent_bits_small.bin")
            sr.write_container(path, sr.make_raw(sr.SMALL_OUT, 41))
            tb.LoadUpscaleWeights(path)
            before = tb.GetOption("sr_conv_form")
            tb.SetOption("sr_conv_form", form)
            try:
                return tb.RunUpscaleNeural(_surfaces(_rng("sr_%dx%d" % (w, h)), w, h, 1)[0])      # the same picture in both forms
            finally:
                tb.SetOption("sr_conv_form", before)
        out.append((name, run))

    neural("neural_small9_16x16", 16, 16)
    neural("neural_small9_40x24", 40, 24)
    upscale("sr_small_17x9_form0", 17, 9, 0)
    upscale("sr_small_17x9_form1", 17, 9, 1)
    return out


CASES = dict(cases())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_bits_are_the_parents(gpu_tb, tmp_path, name):
    with open(FIXTURE) as f:
        recorded = json.load(f)["digests"]
    assert digest(CASES[name](gpu_tb, tmp_path)) == recorded[name]
