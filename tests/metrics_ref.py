"""NumPy restatement of the image-quality metrics (include/tracerboy_hip.h tb_run_compare / tb_compare), written from the
contract in the header, not from the kernels: fp64 for the pointwise part, explicit fp32 steps for SSIM, the eleven weights as literals.

compare(test, ref, ...) returns the result's fields, both maps, and for every fp64 sum what the any-order bound needs: the sum itself, the number
of its terms and the sum of their magnitudes.  ssim_fp64 evaluates the same definition in fp64, for the check of the fp32 error."""
import numpy as np

F32, F64 = np.float32, np.float64
WEIGHTS = np.array([0x3a86cab6, 0x3bf8ff01, 0x3d13758c, 0x3ddff87f, 0x3e5a1e20, 0x3e8832b0, 0x3e5a1e20, 0x3ddff87f, 0x3d13758c, 0x3bf8ff01, 0x3a86cab6],
                   np.uint32).view(F32)
TAPS = 11
TB_COMPARE_SSIM, TB_COMPARE_SUMS = 1, 2
U = 2.0 ** -53      # unit roundoff of binary64


def split(test, ref, sums=False):
    """(A.rgb, R.rgb, excluded, unsampled): A = sum.rgb / sum.w in fp32 where test holds sums; alpha is otherwise ignored."""
    t, r = np.ascontiguousarray(test, F32), np.ascontiguousarray(ref, F32)
    assert t.shape == r.shape and t.ndim == 3 and t.shape[2] == 4
    with np.errstate(all="ignore"):
        a = (t[..., :3] / t[..., 3:4]).astype(F32) if sums else t[..., :3]
    unsampled = (t[..., 3] == 0) if sums else np.zeros(t.shape[:2], bool)
    excluded = unsampled | ~(np.isfinite(a).all(-1) & np.isfinite(r[..., :3]).all(-1))
    return a, r[..., :3], excluded, unsampled


def pointwise(a, r, excluded, rel_epsilon):
    """per included pixel and channel in fp64; the three channels of a pixel added in the order r, g, b"""
    inc = ~excluded
    A, R = a[inc].astype(F64), r[inc].astype(F64)
    d = A - R
    se, ae = d * d, np.abs(d)
    re = se / (R * R + F64(F32(rel_epsilon)))
    per_pixel = [(x[:, 0] + x[:, 1]) + x[:, 2] for x in (se, ae, re)]
    sq_map = np.zeros(excluded.shape, F32)
    with np.errstate(over="ignore"):
        sq_map[inc] = (per_pixel[0] / 3.0).astype(F32)
    return per_pixel, (float(ae.max()) if ae.size else float("nan")), sq_map


def clamp(x, peak):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, F32(0), np.where(x > peak, peak, x)).astype(x.dtype)


def filter_valid(x, weights):
    """rows, then columns; each pass acc = 0; acc = acc + w[i] * x[i], taps ascending, in x's own precision"""
    h, w = x.shape
    acc = np.zeros((h, w - TAPS + 1), x.dtype)
    for i in range(TAPS):
        acc = acc + weights[i] * x[:, i:i + w - TAPS + 1]
    out = np.zeros((h - TAPS + 1, w - TAPS + 1), x.dtype)
    for i in range(TAPS):
        out = out + weights[i] * acc[i:i + h - TAPS + 1, :]
    return out


def window_skipped(excluded):
    """a window holds an excluded pixel"""
    h, w = excluded.shape
    rows = np.zeros((h, w - TAPS + 1), bool)
    for i in range(TAPS):
        rows |= excluded[:, i:i + w - TAPS + 1]
    out = np.zeros((h - TAPS + 1, w - TAPS + 1), bool)
    for i in range(TAPS):
        out |= rows[i:i + h - TAPS + 1, :]
    return out


U32 = 2.0 ** -24    # unit roundoff of binary32


def ssim_windows(a, r, excluded, peak, dtype=F32, error_bound=False):
    """(fp64 window values, skipped) of the (h - 10) x (w - 10) windows, or (None, None) without one.  dtype = float64: the same definition
    evaluated in fp64 on the same clamped fp32 inputs.

    error_bound (with float64): a third array, how far the fp32 evaluation's value of a window may lie from this one.  With u = 2^-24: a moment
    is two passes of eleven multiply-adds over non-negative terms, so it carries a relative error of at most 44 u; va = Eaa - ma ma then has an
    absolute error of at most 45 u Eaa + 89 u ma^2 + u va <= 135 u Eaa (ma^2 <= Eaa), vr likewise, and c = Ear - ma mr at most
    67.5 u (Eaa + Err), since Ear and ma mr are at most (Eaa + Err) / 2.  So N2 = 2 c + C2 and D2 = va + vr + C2 are each off by at most
    B = 135 u (Eaa + Err), which does not shrink with them -- the cancellation that makes flat windows inexact -- and everything else (N1, D1, the
    last additions, the two products, the division) adds relative errors below 210 u.  s = N1 N2 / (D1 D2) is therefore within
    (|N1| B / D1 + |s| B) / (D2 - B) + 220 u |s| of the exact value; the fp64 evaluation's own error is nine orders smaller.  The window's value
    is the mean of three such and is rounded to fp32 once more."""
    h, w = excluded.shape
    if w < TAPS or h < TAPS:
        return (None, None, None) if error_bound else (None, None)
    peak = F32(peak)
    c1 = dtype((0.01 * F64(peak)) * (0.01 * F64(peak))); c2 = dtype((0.03 * F64(peak)) * (0.03 * F64(peak)))
    weights = WEIGHTS.astype(dtype)
    two = dtype(2)
    total = None
    bound = 0.0
    with np.errstate(all="ignore"):
        for c in range(3):
            x = clamp(a[..., c].astype(F32), peak); x[excluded] = 0
            y = clamp(r[..., c].astype(F32), peak); y[excluded] = 0
            x, y = x.astype(dtype), y.astype(dtype)
            ma, mr, eaa, err, ear = (filter_valid(p, weights) for p in (x, y, x * x, y * y, x * y))
            va, vr, cov = eaa - ma * ma, err - mr * mr, ear - ma * mr
            s = (((two * ma) * mr + c1) * (two * cov + c2)) / (((ma * ma + mr * mr) + c1) * ((va + vr) + c2))
            assert s.dtype == dtype
            total = s.astype(F64) if total is None else total + s.astype(F64)
            if error_bound:
                assert dtype == F64
                n1, d1, d2 = (two * ma) * mr + c1, (ma * ma + mr * mr) + c1, (va + vr) + c2
                b = 135.0 * U32 * (eaa + err)
                assert (d2 - b > 0).all()
                bound = bound + (np.abs(n1) * b / d1 + np.abs(s) * b) / (d2 - b) + 220.0 * U32 * np.abs(s)
        if error_bound:
            return total / 3.0, window_skipped(excluded), bound / 3.0 + U32 * np.abs(total / 3.0)
        return total / 3.0, window_skipped(excluded)


def compare(test, ref, peak=1.0, rel_epsilon=0.01, flags=TB_COMPARE_SSIM):
    a, r, excluded, unsampled = split(test, ref, bool(flags & TB_COMPARE_SUMS))
    (se, ae, re), max_abs, sq_map = pointwise(a, r, excluded, rel_epsilon)
    pixels = int((~excluded).sum())
    out = dict(pixels=pixels, excluded=int(excluded.sum()), unsampled=int(unsampled.sum()), max_abs=max_abs, sq_err_map=sq_map)
    sums = {}
    for name, terms in (("mse", se), ("mae", ae), ("rel_mse", re)):
        total = float(np.sum(terms))
        sums[name] = dict(sum=total, terms=pixels, magnitude=total, divisor=3.0 * pixels)        # every term is >= 0
        out[name] = total / (3.0 * pixels) if pixels else float("nan")
    with np.errstate(divide="ignore"):
        out["psnr"] = float("nan") if not pixels else float("inf") if out["mse"] == 0 else float(10.0 * np.log10(F64(F32(peak)) * F64(F32(peak)) / out["mse"]))
    values, skipped = ssim_windows(a, r, excluded, peak) if flags & TB_COMPARE_SSIM else (None, None)
    h, w = excluded.shape
    out["ssim_map"] = np.zeros((max(h - 10, 0), max(w - 10, 0)), F32)
    if values is None:
        out.update(ssim_windows=0, ssim_windows_skipped=0, ssim=float("nan"))
        sums["ssim"] = dict(sum=0.0, terms=0, magnitude=0.0, divisor=0.0)
    else:
        counted = values[~skipped]
        total = float(np.sum(counted))
        out.update(ssim_windows=int(counted.size), ssim_windows_skipped=int(skipped.sum()), ssim=total / counted.size if counted.size else float("nan"))
        with np.errstate(all="ignore"):
            out["ssim_map"] = np.where(skipped, F32(0), values.astype(F32)).astype(F32)
        sums["ssim"] = dict(sum=total, terms=int(counted.size), magnitude=float(np.sum(np.abs(counted))), divisor=float(counted.size))
    out["sums"] = sums
    return out


def mean_bound(info, mean_a, mean_b):
    """How far two evaluations of mean = S / divisor may lie apart: each S is within terms * 2^-53 * sum|term| of the exact sum whatever the
    order of its additions (Higham, Accuracy and Stability of Numerical Algorithms, (4.3)), so the two are within twice that of each other; each
    division then rounds once, a relative 2^-53 of its own quotient."""
    if not info["terms"]:
        return 0.0
    return 2.0 * info["terms"] * U * info["magnitude"] / info["divisor"] + U * (abs(mean_a) + abs(mean_b)) * (1.0 + 2.0 * U)


def ssim_fp64(test, ref, peak=1.0, flags=TB_COMPARE_SSIM):
    """(window values in fp64, skipped, the bound of ssim_windows on the fp32 evaluation's distance from them)"""
    a, r, excluded, _ = split(test, ref, bool(flags & TB_COMPARE_SUMS))
    return ssim_windows(a, r, excluded, peak, F64, error_bound=True)
