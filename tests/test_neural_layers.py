"""nn_convk with K = 3 in its plain form (+ the max-pool) at the layer seam, tb_run_conv3x3, against the torch restatement of the layer contract
(tests/nn_layer_ref.py, which also holds the check).

The bound is derived, not measured: |y - ref| <= 2^-10 |ref| + 2^-12 S + 2^-24, S = conv(|x|, |w|) + |b| at the same element before pooling (the
maximum over the 2 x 2 window with pool).  The first term is one binary16 rounding step, for a flip of the last bit; the second is above any fp32
summation-order difference of <= 4 608 terms; evaluating the layer with fp64 accumulation instead of fp32 uses 0.13 of it.  Where the reference
is infinite or NaN the result must be of the same kind."""
import numpy as np
import pytest
import torch

import neural_ref as nr
from nn_layer_ref import check as check_layer

gpu = pytest.mark.gpu

TB_E_INVALID = -1


def tensor(rng, w, h, c):
    return rng.random((h, w, c)).astype(np.float16)    # [0, 1)


def he(rng, c_out, c_in):
    return (rng.standard_normal((c_out, c_in, 3, 3)) * np.sqrt(2.0 / (9 * c_in))).astype(np.float16), (rng.standard_normal(c_out) * 0.1).astype(np.float16)


def check(tb, a, w, b, **kw):
    return check_layer(tb.RunConv3x3(a, w, b, **kw), a, w, b, **kw)


@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (16, 16), (17, 33)])
def test_first_layer_9_to_32(gpu_tb, w, h):
    """fewer pixels than one tile, tile remainders in x, input channels below one k-block"""
    rng = np.random.default_rng(w * 100 + h)
    y, ref = check(gpu_tb, tensor(rng, w, h, 9), *he(rng, 32, 9))
    assert float(ref.astype(np.float32).max()) > 0.1   # the test means something: the layer is not dead


@gpu
@pytest.mark.parametrize("w,h", [(16, 16), (34, 18)])
def test_32_to_48_with_pool(gpu_tb, w, h):
    rng = np.random.default_rng(w + h)
    y, _ = check(gpu_tb, tensor(rng, w, h, 32), *he(rng, 48, 32), pool=True)
    assert y.shape == (h // 2, w // 2, 48)


@gpu
def test_upsampled_64_and_9_to_64(gpu_tb):
    """73 input channels: K is no multiple of 32, source A is read upsampled, source B starts a k-block of its own"""
    rng = np.random.default_rng(7)
    check(gpu_tb, tensor(rng, 9, 17, 64), *he(rng, 64, 73), in_b=tensor(rng, 18, 34, 9), upsample_a=True)


@gpu
def test_upsampled_96_and_64_to_112(gpu_tb):
    """112 output channels: padded to 128, four accumulator blocks per wave"""
    rng = np.random.default_rng(8)
    check(gpu_tb, tensor(rng, 2, 3, 96), *he(rng, 112, 160), in_b=tensor(rng, 4, 6, 64), upsample_a=True)


@gpu
@pytest.mark.parametrize("relu", [False, True])
def test_last_layer_32_to_3(gpu_tb, relu):
    rng = np.random.default_rng(9)
    y, ref = check(gpu_tb, tensor(rng, 17, 33, 32), *he(rng, 3, 32), relu=relu)
    assert (ref.astype(np.float32).min() < 0) == (not relu)


@gpu
def test_channel_counts_below_one_fragment(gpu_tb):
    rng = np.random.default_rng(10)
    check(gpu_tb, tensor(rng, 6, 10, 5), *he(rng, 7, 5))
    check(gpu_tb, tensor(rng, 3, 5, 6), *he(rng, 10, 9), in_b=tensor(rng, 6, 10, 3), upsample_a=True)


@gpu
def test_96_to_96_at_2x2(gpu_tb):
    rng = np.random.default_rng(11)
    check(gpu_tb, tensor(rng, 2, 2, 96), *he(rng, 96, 96))


@gpu
def test_real_first_layer_weights(gpu_tb, tmp_path):
    """enc_conv0 of OIDN's rt_ldr_alb_nrm.tza: weights up to 18.5 in magnitude"""
    t = nr.read_tza(nr.real_weights_file(tmp_path))
    w, b = t["enc_conv0.weight"][0], t["enc_conv0.bias"][0]
    assert float(np.abs(w.astype(np.float32)).max()) == 18.5
    rng = np.random.default_rng(12)
    check(gpu_tb, tensor(rng, 17, 33, 9), w, b)


@gpu
def test_overflow_gives_infinity_and_nan_is_propagated(gpu_tb):
    rng = np.random.default_rng(13)
    x = tensor(rng, 17, 9, 9); w, b = he(rng, 32, 9)
    w[3, 4, 1, 1] = 60000.0; x[5, 6, 4] = 2.0          # 120 000 is past binary16: infinity at (5, 6) of channel 3
    w[5, 4, 1, 1] = -60000.0                            # minus infinity without ReLU, 0 with
    for relu in (True, False):
        y, ref = check(gpu_tb, x, w, b, relu=relu)
        assert np.isposinf(ref[5, 6, 3]) and np.isposinf(y[5, 6, 3])
        assert (y[5, 6, 5] == 0) if relu else np.isneginf(y[5, 6, 5])
    x[2, 15, 1] = np.nan                                # in the last tile's row end: every output whose 3 x 3 window holds it
    y, ref = check(gpu_tb, x, w, b)
    assert np.isnan(y[1:4, 14:17]).all() and np.isnan(y).sum() == 9 * 32
    y, _ = check(gpu_tb, x, w, b, pool=False, relu=False)
    assert np.isnan(y).sum() == 9 * 32


@gpu
def test_pool_takes_the_rounded_values_and_keeps_nan(gpu_tb):
    rng = np.random.default_rng(14)
    x = tensor(rng, 6, 4, 5); w, b = he(rng, 7, 5)
    x[1, 1, 0] = np.nan
    y, ref = check(gpu_tb, x, w, b, pool=True)
    assert np.isnan(y[:2, :2]).all() and np.isnan(y).sum() == 4 * 7 and not np.isnan(y[:, 2]).any()


@gpu
def test_misuse_is_refused(gpu_tb):
    from tracerboy_amd import api, _ctypes_abi as abi
    import ctypes as C
    tb, L = gpu_tb, api.lib()
    rng = np.random.default_rng(15)
    a = tensor(rng, 4, 4, 3); w, b = he(rng, 4, 3); out = np.empty((4, 4, 4), np.float16)
    p = lambda v: v.ctypes.data_as(C.c_void_p)

    def rc(desc, in_a=a, in_b=None, weight=w, bias=b, result=out):
        d = abi.tb_conv3x3_desc(*desc)
        code = L.tb_run_conv3x3(tb._ctx, C.byref(d), *[None if v is None else p(v) for v in (in_a, in_b, weight, bias, result)])
        return code, (L.tb_last_error(tb._ctx) or b"").decode()

    good = (4, 4, 3, 0, 4, 0, 0, 1)
    assert rc(good)[0] == 0
    for kw in ({"in_a": None}, {"weight": None}, {"bias": None}, {"result": None}):
        code, msg = rc(good, **kw); assert code == TB_E_INVALID and "null" in msg
    assert L.tb_run_conv3x3(tb._ctx, None, p(a), None, p(w), p(b), p(out)) == TB_E_INVALID
    for desc, word in (((0, 4, 3, 0, 4, 0, 0, 1), "0"), ((4, 0, 3, 0, 4, 0, 0, 1), "0"), ((4, 4, 0, 0, 4, 0, 0, 1), "0"), ((4, 4, 3, 0, 0, 0, 0, 1), "0"),
                       ((5, 4, 3, 0, 4, 0, 1, 1), "even"), ((4, 5, 3, 0, 4, 1, 0, 1), "even"),
                       ((4, 4, 513, 0, 4, 0, 0, 1), "512"), ((4, 4, 3, 0, 513, 0, 0, 1), "512"),
                       ((4097, 4096, 3, 0, 4, 0, 0, 1), "2^24")):
        code, msg = rc(desc); assert code == TB_E_INVALID and word in msg, (desc, code, msg)
    code, msg = rc((4, 4, 3, 513, 4, 0, 0, 1), in_b=a); assert code == TB_E_INVALID and "512" in msg
    code, msg = rc((4, 4, 3, 2, 4, 0, 0, 1)); assert code == TB_E_INVALID and "source B" in msg      # c_b without in_b
    code, msg = rc((4, 4, 3, 0, 4, 0, 0, 1), in_b=a); assert code == TB_E_INVALID and "source B" in msg


def test_selfcheck_of_the_reference_fp64_sits_well_inside_the_bound():
    """A self-check of tests/neural_ref.py, not of the library (it needs no GPU and no build): what the docstring says of the bound -- the
    reference accumulated in fp64 against the reference accumulated in fp32 uses a small part of it."""
    rng = np.random.default_rng(16)
    a, b2 = tensor(rng, 9, 17, 64), tensor(rng, 18, 34, 9); w, b = he(rng, 64, 73)
    r32 = nr.conv_ref(a, w, b, in_b=b2, upsample_a=True).astype(np.float64)
    r64 = nr.conv_ref(a, w, b, in_b=b2, upsample_a=True, accumulate=torch.float64).astype(np.float64)
    s = nr.conv_scale(a, w, b, in_b=b2, upsample_a=True)
    assert float((np.abs(r64 - r32) / (2.0 ** -10 * np.abs(r32) + 2.0 ** -12 * s + 2.0 ** -24)).max()) < 0.5
