"""nn_convk in its plain form and nn_sr_finish at their seams, tb_run_conv and tb_run_sr_finish.

Against torch (tests/nn_layer_ref.py, which also holds the check) the bound is section 15's, derived, not measured: |y - ref| <= 2^-10 |ref| + 2^-12 S + 2^-24 with
S = conv(|x|, |w|) + |b| at the same element.  The first term is one binary16 rounding step; the second is above any fp32 summation-order
difference while taps x channels <= 4096 (this network's largest layer has 25 x 64 = 1600; the largest here 25 x 96 = 2400).  Where the reference
is infinite or NaN the result must be of the same kind.  The delta filters, the NaN neighbourhood and the residual add are bit-for-bit statements."""
import ctypes as C

import numpy as np
import pytest

import sr_ref as sr
from nn_layer_ref import check as check_layer

pytestmark = pytest.mark.gpu

TB_E_INVALID = -1


def tensor(rng, w, h, c):
    return rng.random((h, w, c)).astype(np.float16)    # [0, 1)


def he(rng, c_out, c_in, k):
    return (rng.standard_normal((c_out, c_in, k, k)) * np.sqrt(2.0 / (k * k * c_in))).astype(np.float16), (rng.standard_normal(c_out) * 0.1).astype(np.float16)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def check(tb, a, w, b, **kw):
    return check_layer(tb.RunConv(a, w, b, **kw), a, w, b, **kw)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (15, 1), (16, 2), (17, 3), (16, 4), (33, 5)])
def test_first_layer_3_to_32(gpu_tb, k, w, h):
    """fewer pixels than a tile and than a filter, tile remainders in x, heights 1 ... 5 (every row within the 5 x 5 halo of an edge)"""
    rng = np.random.default_rng(w * 100 + h + k)
    y, ref = check(gpu_tb, tensor(rng, w, h, 3), *he(rng, 32, 3, k))
    assert float(ref.astype(np.float32).max()) > 0.1   # the layer is not dead


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("c_a,c_out,w,h", [(32, 64, 17, 5), (33, 16, 5, 7), (64, 48, 16, 3), (96, 112, 5, 4), (64, 3, 17, 2)])
def test_channel_counts(gpu_tb, k, c_a, c_out, w, h):
    """k-blocks: one, one and a padded one, two, three; output blocks: below one, padded to 32, 64 (four per wave), 112 padded to 128"""
    rng = np.random.default_rng(c_a * 7 + c_out + k)
    check(gpu_tb, tensor(rng, w, h, c_a), *he(rng, c_out, c_a, k))


@pytest.mark.parametrize("k", [3, 5])
def test_upsampled_source_and_two_sources(gpu_tb, k):
    rng = np.random.default_rng(20 + k)
    check(gpu_tb, tensor(rng, 1, 1, 64), *he(rng, 32, 64, k), upsample_a=True)                      # 2 x 2 from a 1 x 1 source
    check(gpu_tb, tensor(rng, 9, 3, 64), *he(rng, 32, 64, k), upsample_a=True)                      # conv_up1's shape
    check(gpu_tb, tensor(rng, 9, 2, 33), *he(rng, 16, 36, k), in_b=tensor(rng, 18, 4, 3), upsample_a=True)   # B starts a k-block of its own
    check(gpu_tb, tensor(rng, 17, 5, 32), *he(rng, 32, 96, k), in_b=tensor(rng, 17, 5, 64))


@pytest.mark.parametrize("k", [3, 5])
def test_without_bias_and_without_relu(gpu_tb, k):
    rng = np.random.default_rng(30 + k)
    x = tensor(rng, 17, 5, 32); w, b = he(rng, 3, 32, k)
    y, ref = check(gpu_tb, x, w, None, relu=False)
    assert ref.astype(np.float32).min() < 0
    y_bias, _ = check(gpu_tb, x, w, b, relu=False)
    assert not np.array_equal(bits(y), bits(y_bias))
    check(gpu_tb, x, w, None, relu=True)


@pytest.mark.parametrize("c,w,h", [(3, 7, 6), (32, 17, 5), (40, 5, 7)])
def test_delta_filters_shift_the_input_exactly(gpu_tb, c, w, h):
    """For each of the K x K taps a one-hot filter (channel i -> output i): the output is the input shifted by that tap with zero fill, exactly --
    a flipped or transposed tap order shows here.  No bias, no ReLU; the inputs hold no -0 (the sum of +0 and -0 is +0)."""
    rng = np.random.default_rng(c)
    x = (rng.random((h, w, c)) - 0.5).astype(np.float16)
    x[x == 0] = np.float16(0.25)
    for k in (3, 5):
        r = (k - 1) // 2
        for ky in range(k):
            for kx in range(k):
                f = np.zeros((c, c, k, k), np.float16)
                f[np.arange(c), np.arange(c), ky, kx] = 1.0
                want = np.zeros_like(x)                      # out[y, x] = in[y + ky - r, x + kx - r]
                dy, dx = ky - r, kx - r
                ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
                src_y, src_x = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
                want[ys, xs] = x[src_y, src_x]
                got = gpu_tb.RunConv(x, f, None, relu=False)
                assert np.array_equal(bits(got), bits(want)), (k, ky, kx)


@pytest.mark.parametrize("k", [3, 5])
def test_overflow_gives_infinity_and_a_nan_spreads_over_its_neighbourhood_alone(gpu_tb, k):
    rng = np.random.default_rng(40 + k)
    x = tensor(rng, 21, 9, 35); w, b = he(rng, 32, 35, k)
    r = (k - 1) // 2
    w[3, 4, r, r] = 60000.0; x[5, 6, 4] = 2.0          # 120 000 is past binary16: infinity at (5, 6) of channel 3
    w[5, 4, r, r] = -60000.0                            # minus infinity without ReLU, 0 with
    for relu in (True, False):
        y, ref = check(gpu_tb, x, w, b, relu=relu)
        assert np.isposinf(ref[5, 6, 3]) and np.isposinf(y[5, 6, 3])
        assert (y[5, 6, 5] == 0) if relu else np.isneginf(y[5, 6, 5])
    poisoned = x.copy(); poisoned[1, 16, 1] = np.nan    # around a tile seam, its neighbourhood cut by the top edge for K = 5
    y, _ = check(gpu_tb, poisoned, w, b)
    clean, _ = check(gpu_tb, x, w, b)                   # afterwards, on the same sizes
    mask = np.zeros(y.shape[:2], bool); mask[max(0, 1 - r):2 + r, 16 - r:17 + r] = True
    assert np.isnan(y[mask]).all() and not np.isnan(y[~mask]).any() and int(mask.sum()) == {3: 9, 5: 20}[k]
    assert np.array_equal(bits(y[~mask]), bits(clean[~mask]))


def test_misuse_is_refused(gpu_tb):
    from tracerboy_amd import api, _ctypes_abi as abi
    tb, L = gpu_tb, api.lib()
    rng = np.random.default_rng(15)
    a = tensor(rng, 4, 4, 3); w, b = he(rng, 4, 3, 5); out = np.empty((4, 4, 4), np.float16)
    p = lambda v: v.ctypes.data_as(C.c_void_p)

    def rc(desc, in_a=a, in_b=None, weight=w, bias=b, result=out):
        d = abi.tb_conv_desc(*desc)
        code = L.tb_run_conv(tb._ctx, C.byref(d), *[None if v is None else p(v) for v in (in_a, in_b, weight, bias, result)])
        return code, (L.tb_last_error(tb._ctx) or b"").decode()

    #       width height c_a c_b c_out kernel upsample relu form
    good = (4, 4, 3, 0, 4, 5, 0, 1, 0)
    assert rc(good)[0] == 0 and rc(good, bias=None)[0] == 0
    for kw in ({"in_a": None}, {"weight": None}, {"result": None}):
        code, msg = rc(good, **kw); assert code == TB_E_INVALID and "null" in msg
    assert L.tb_run_conv(tb._ctx, None, p(a), None, p(w), p(b), p(out)) == TB_E_INVALID
    for desc, word in (((0, 4, 3, 0, 4, 5, 0, 1, 0), "0"), ((4, 0, 3, 0, 4, 5, 0, 1, 0), "0"), ((4, 4, 0, 0, 4, 5, 0, 1, 0), "0"), ((4, 4, 3, 0, 0, 5, 0, 1, 0), "0"),
                       ((5, 4, 3, 0, 4, 5, 1, 1, 0), "even"), ((4, 5, 3, 0, 4, 5, 1, 1, 0), "even"),
                       ((4, 4, 513, 0, 4, 5, 0, 1, 0), "512"), ((4, 4, 3, 0, 513, 5, 0, 1, 0), "512"),
                       ((4097, 4096, 3, 0, 4, 5, 0, 1, 0), "2^24"),
                       ((4, 4, 3, 0, 4, 4, 0, 1, 0), "kernel 4"), ((4, 4, 3, 0, 4, 7, 0, 1, 0), "kernel 7"), ((4, 4, 3, 0, 4, 1, 0, 1, 0), "kernel 1"),
                       ((4, 4, 3, 0, 4, 0, 0, 1, 0), "kernel 0"), ((4, 4, 3, 0, 4, 5, 0, 1, 2), "form 2")):
        code, msg = rc(desc); assert code == TB_E_INVALID and word in msg, (desc, code, msg)
    code, msg = rc((4, 4, 3, 513, 4, 5, 0, 1, 0), in_b=a); assert code == TB_E_INVALID and "512" in msg
    code, msg = rc((4, 4, 3, 2, 4, 5, 0, 1, 0)); assert code == TB_E_INVALID and "source B" in msg      # c_b without in_b
    code, msg = rc((4, 4, 3, 0, 4, 5, 0, 1, 0), in_b=a); assert code == TB_E_INVALID and "source B" in msg
    assert rc((4, 4, 3, 0, 4, 5, 0, 1, 1))[0] == 0
    wide = np.zeros((4, 4, 65), np.float16); w65 = np.zeros((4, 65, 5, 5), np.float16)
    assert rc((4, 4, 65, 0, 4, 5, 0, 1, 0), in_a=wide, weight=w65)[0] == 0
    code, msg = rc((4, 4, 65, 0, 4, 5, 0, 1, 1), in_a=wide, weight=w65); assert code == TB_E_INVALID and "staged" in msg     # three k-blocks
    code, msg = rc((4, 4, 33, 3, 4, 5, 0, 1, 1), in_a=wide, in_b=a, weight=w65); assert code == TB_E_INVALID and "staged" in msg   # 64 + 32 padded
    assert rc(good)[0] == 0                                                                              # and the context still works


def finish_cases():
    """(residual, picture) pairs whose sums tie, overflow, cancel, are negative, -0 and NaN"""
    f16 = np.float16
    return [(f16(2048.0), f16(1.0)),          # 2049 ties between 2048 and 2050: even
             (f16(2050.0), f16(1.0)),          # 2051 ties between 2050 and 2052: up to the even 2052
             (f16(1.0), f16(2.0 ** -11)),      # ties to 1
             (f16(1.0), f16(2.0 ** -11 + 2.0 ** -21)),  # just past the tie: the exact sum decides, 1 + 2^-10
             (f16(65504.0), f16(65504.0)),     # overflows to infinity
             (f16(65504.0), f16(15.0)),        # 65519 rounds to 65504
             (f16(65504.0), f16(16.0)),        # 65520 ties to infinity
             (f16(-65504.0), f16(-65504.0)),   # |-inf| = inf
             (f16(0.3), f16(-0.3)),            # cancels to +0
             (f16(-0.0), f16(-0.0)),           # -0, |-0| = +0
             (f16(-0.75), f16(0.25)),          # negative: the abs
             (f16(2.0 ** -24), f16(2.0 ** -24)),   # subnormals
             (f16(-6.1e-5), f16(5.96e-8)),
             (f16(np.nan), f16(1.0)), (f16(1.0), f16(np.nan)), (f16(np.inf), f16(-np.inf))]


def finish_inputs(rng, w, h, cases):
    """residual (2 h, 2 w, 3) and picture (h, w, 3): random values, and the cases at the first values of the picture, each at one of the four
    output pixels of its input pixel"""
    res = ((rng.random((2 * h, 2 * w, 3)) - 0.5) * 0.5).astype(np.float16)
    pic = rng.random((h, w, 3)).astype(np.float16)
    for i, (a, b) in enumerate(cases):
        y, x, c = np.unravel_index(i, pic.shape)
        pic[y, x, c] = b
        res[2 * y + (i & 1), 2 * x + ((i >> 1) & 1), c] = a
    return res, pic


@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (17, 3)])
def test_finish_against_numpy_bit_for_bit(gpu_tb, w, h):
    cases = finish_cases()
    for n, chunk in enumerate([cases[i:i + 3] for i in range(0, len(cases), 3)] if w == 1 else [cases]):     # a 1 x 1 picture holds three values
        res, pic = finish_inputs(np.random.default_rng(w + n), w, h, chunk)
        got, want = gpu_tb.RunSrFinish(res, pic), sr.finish_ref(res, pic)
        assert got.shape == (2 * h, 2 * w, 4) and np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, got.view(np.uint32))        # no sign bit anywhere
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
        if w > 1:
            assert nan.sum() == 6 and np.isinf(want).sum() == 6 and (want[..., 3] == 1).all()      # a NaN or an infinity of the picture reaches its four pixels


def test_finish_misuse_is_refused(gpu_tb):
    from tracerboy_amd import api
    tb, L = gpu_tb, api.lib()
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    res, pic, out = np.zeros((4, 4, 3), np.float16), np.zeros((2, 2, 3), np.float16), np.empty((4, 4, 4), np.float32)
    assert L.tb_run_sr_finish(tb._ctx, 2, 2, p(res), p(pic), p(out)) == 0
    for args in ((None, p(pic), p(out)), (p(res), None, p(out)), (p(res), p(pic), None)):
        assert L.tb_run_sr_finish(tb._ctx, 2, 2, *args) == TB_E_INVALID and b"null" in L.tb_last_error(tb._ctx)
    assert L.tb_run_sr_finish(tb._ctx, 0, 2, p(res), p(pic), p(out)) == TB_E_INVALID
    assert L.tb_run_sr_finish(tb._ctx, 2049, 2048, p(res), p(pic), p(out)) == TB_E_INVALID and b"2^24" in L.tb_last_error(tb._ctx)
