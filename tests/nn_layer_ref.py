"""The convolution layer of both neural networks restated in torch, once (DESIGN.md sections 15 and 16), and the one check of a layer against it.

Tensors are numpy float16, NHWC without a batch axis, (H, W, C); weights are (o, i, K, K) with K odd.  tests/neural_ref.py and tests/sr_ref.py
pass conv_ref and conv_scale on under their own names.

The bound of check is derived, not measured: |y - ref| <= 2^-10 |ref| + 2^-12 S + 2^-24, S = conv(|x|, |w|) + |b| at the same element before
pooling (the maximum over the 2 x 2 window with pool).  The first term is one binary16 rounding step, for a flip of the last bit; the second is
above any fp32 summation-order difference while taps x channels <= 4 608; evaluating the layer with fp64 accumulation instead of fp32 uses 0.13 of
it.  Where the reference is infinite or NaN the result must be of the same kind."""
import numpy as np
import torch
import torch.nn.functional as F


def _nchw(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, np.float16).astype(np.float32)).to(dtype).permute(2, 0, 1)[None]


def _gather(in_a, in_b, upsample_a, dtype):
    a = _nchw(in_a, dtype)
    if upsample_a:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    return a if in_b is None else torch.cat([a, _nchw(in_b, dtype)], 1)


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float16).astype(np.float32)).to(dtype)


def conv_ref(in_a, weight, bias=None, in_b=None, upsample_a=False, pool=False, relu=True, accumulate=torch.float32):
    """One layer: cross-correlation in `accumulate` precision on the binary16 inputs with zero padding (K - 1) / 2, + bias where there is one,
    ReLU where asked, one rounding to binary16, then the max-pool where asked.  (H, W, c_out) float16 -- halved with pool."""
    k = np.asarray(weight).shape[2]
    y = F.conv2d(_gather(in_a, in_b, upsample_a, accumulate), _t(weight, accumulate), _t(bias, accumulate), padding=(k - 1) // 2)
    if relu:
        y = F.relu(y)
    y = y.to(torch.float16)
    if pool:
        y = F.max_pool2d(y.float(), 2).to(torch.float16)  # on the rounded values; the maximum of binary16 numbers is one of them
    return y[0].permute(1, 2, 0).contiguous().numpy()


def conv_scale(in_a, weight, bias=None, in_b=None, upsample_a=False, pool=False):
    """S of the layer tolerance: conv(|x|, |w|) + |b| at the same element in float64, the maximum over the 2 x 2 window with pool."""
    k = np.asarray(weight).shape[2]
    b = _t(bias, torch.float64)
    s = F.conv2d(_gather(in_a, in_b, upsample_a, torch.float64).abs(), _t(weight, torch.float64).abs(), None if b is None else b.abs(), padding=(k - 1) // 2)
    if pool:
        s = F.max_pool2d(s, 2)
    return s[0].permute(1, 2, 0).contiguous().numpy()


def check(y, a, w, b, in_b=None, upsample_a=False, pool=False, relu=True):
    """y, what the library made of the layer, against conv_ref: the derived bound, and the same kind where the reference is infinite or NaN.
    Returns (y, ref)."""
    ref = conv_ref(a, w, b, in_b=in_b, upsample_a=upsample_a, pool=pool, relu=relu)
    s = conv_scale(a, w, b, in_b=in_b, upsample_a=upsample_a, pool=pool)
    assert y.shape == ref.shape == s.shape and y.dtype == np.float16
    y64, r64 = y.astype(np.float64), ref.astype(np.float64)
    finite = np.isfinite(r64)
    assert np.array_equal(np.isnan(y64), np.isnan(r64)) and np.array_equal(np.isinf(y64), np.isinf(r64))
    assert np.array_equal(np.sign(y64[np.isinf(r64)]), np.sign(r64[np.isinf(r64)]))
    with np.errstate(invalid="ignore"):
        err = np.abs(y64 - r64)[finite]
    bound = (2.0 ** -10 * np.abs(r64) + 2.0 ** -12 * s + 2.0 ** -24)[finite]
    worst = float((err / bound).max()) if err.size else 0.0
    print("  %s K %d: max |y - ref| = %.3e, %.3f of the bound, %d of %d elements differ" % (y.shape, np.asarray(w).shape[2], err.max() if err.size else 0.0, worst,
                                                                                           int((err > 0).sum()), err.size))
    assert worst <= 1.0
    return y, ref
