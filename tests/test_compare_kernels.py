"""Image-quality metrics on the GPU: cmp_kernels.hip through the kernel seam tb_run_compare against the NumPy restatement
(tests/metrics_ref.py) on the cases of tests/compare_cases.py.  Both maps bit for bit (a NaN for a NaN); the five counts and the largest error
equal; every mean within the any-order bound of metrics_ref.mean_bound, which is derived, not tuned; psnr from mse; the same bits on a second
call; every refusal with its code."""
import ctypes as C

import numpy as np
import pytest

import compare_cases as cases
import metrics_ref as ref

F32 = np.float32
TB_E_INVALID = -1
COUNTS = ("pixels", "excluded", "unsampled", "ssim_windows", "ssim_windows_skipped")
MEANS = ("mse", "mae", "rel_mse", "ssim")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def settings_of(kw):
    from tracerboy_amd import api
    s = api.GetDefaultCompareSettings()
    s.peak = kw.get("peak", s.peak); s.rel_epsilon = kw.get("rel_epsilon", s.rel_epsilon); s.flags = kw.get("flags", s.flags)
    return s


def equal_or_both_nan(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def check(got, want, what, peak=1.0):
    for k in COUNTS:
        assert got[k] == want[k], "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    assert equal_or_both_nan(got["max_abs"], want["max_abs"]), "%s: max_abs %r, restatement %r" % (what, got["max_abs"], want["max_abs"])
    for k in MEANS:
        info = want["sums"][k]
        if not info["terms"]:
            assert np.isnan(got[k]) and np.isnan(want[k]), "%s: %s = %r without a term" % (what, k, got[k])
            continue
        bound = ref.mean_bound(info, got[k], want[k])
        print("%s: %s %.17g, restatement %.17g, apart %.3g, bound %.3g" % (what, k, got[k], want[k], abs(got[k] - want[k]), bound))
        assert abs(got[k] - want[k]) <= bound, "%s: %s = %.17g, restatement %.17g: apart %.3g, bound %.3g" % (what, k, got[k], want[k], abs(got[k] - want[k]), bound)
    if not got["pixels"]:
        assert np.isnan(got["psnr"])
    elif got["mse"] == 0:
        assert got["psnr"] == float("inf")
    else:
        assert got["psnr"] == pytest.approx(10.0 * np.log10(float(F32(peak)) ** 2 / got["mse"]), rel=1e-13), what
    assert same_bits(got["sq_err_map"], want["sq_err_map"]), "%s: the squared-error map differs in %d pixels" % (
        what, int((got["sq_err_map"].view(np.uint32) != want["sq_err_map"].view(np.uint32)).sum()))
    assert same_bits(got["ssim_map"], want["ssim_map"]), "%s: the SSIM map differs in %d windows" % (
        what, int((got["ssim_map"].view(np.uint32) != want["ssim_map"].view(np.uint32)).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("size", cases.SIZES, ids=cases.SIZE_IDS)
def test_gpu_metrics_match_the_restatement(gpu_tb, size):
    w, h = size
    for name in cases.names(w, h):
        test, refi, kw, want = cases.restated(name, w, h)
        s = settings_of(kw)
        got = gpu_tb.RunCompare(test, refi, s, maps=True)
        check(got, want, "%dx%d %s" % (w, h, name), s.peak)
        again = gpu_tb.RunCompare(test, refi, s, maps=True)
        for k in COUNTS + MEANS + ("max_abs", "psnr"):
            assert np.float64(got[k]).view(np.uint64) == np.float64(again[k]).view(np.uint64), "%dx%d %s: %s differs between two calls" % (w, h, name, k)
        assert same_bits(got["sq_err_map"], again["sq_err_map"]) and same_bits(got["ssim_map"], again["ssim_map"])
        assert got["gpu_us"] > 0
        without = gpu_tb.RunCompare(test, refi, s)                  # no map asked for: the same record
        assert all(equal_or_both_nan(without[k], got[k]) for k in COUNTS + MEANS + ("max_abs",)) and "sq_err_map" not in without


@pytest.mark.gpu
def test_gpu_identical_pair_is_exact_and_alpha_changes_nothing(gpu_tb):
    test, refi, kw, want = cases.restated("identical", 75, 33)
    got = gpu_tb.RunCompare(test, refi, maps=True)
    assert got["mse"] == 0 and got["max_abs"] == 0 and got["psnr"] == float("inf") and got["ssim"] == 1.0
    assert (got["ssim_map"].view(np.uint32) == F32(1).view(np.uint32)).all()
    test, refi, kw, want = cases.restated("random", 75, 33)
    plain = gpu_tb.RunCompare(test, refi, maps=True)
    t2, r2 = test.copy(), refi.copy()
    t2[::2, ::3, 3] = np.nan; r2[1::2, :, 3] = np.inf; t2[5, 5, 3] = 0.0          # (a zero alpha is a weight only under TB_COMPARE_SUMS)
    alpha = gpu_tb.RunCompare(t2, r2, maps=True)
    for k in COUNTS + MEANS + ("max_abs", "psnr"):
        assert plain[k] == alpha[k], k
    assert same_bits(plain["sq_err_map"], alpha["sq_err_map"]) and same_bits(plain["ssim_map"], alpha["ssim_map"])


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_leave_the_seam_usable(gpu_tb):
    from tracerboy_amd import _ctypes_abi as abi, api
    L, ctx = gpu_tb._L, gpu_tb._ctx
    a = np.zeros((4, 4, 4), F32); pa = a.ctypes.data_as(C.c_void_p)
    out = abi.tb_compare_result()

    def refused(rc, word):
        message = L.tb_last_error(ctx).decode()
        assert rc == TB_E_INVALID and word in message, (rc, message)

    def settings(**kw):
        s = api.GetDefaultCompareSettings()
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)

    refused(L.tb_run_compare(ctx, 4, 4, None, pa, None, C.byref(out), None, None), "null")
    refused(L.tb_run_compare(ctx, 4, 4, pa, None, None, C.byref(out), None, None), "null")
    refused(L.tb_run_compare(ctx, 4, 4, pa, pa, None, None, None, None), "null")
    refused(L.tb_run_compare(ctx, 0, 4, pa, pa, None, C.byref(out), None, None), "dimension is 0")
    refused(L.tb_run_compare(ctx, 4, 0, pa, pa, None, C.byref(out), None, None), "dimension is 0")
    refused(L.tb_run_compare(ctx, 8193, 8192, pa, pa, None, C.byref(out), None, None), "2^26")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(L.tb_run_compare(ctx, 4, 4, pa, pa, settings(peak=bad), C.byref(out), None, None), "peak")
        refused(L.tb_run_compare(ctx, 4, 4, pa, pa, settings(rel_epsilon=bad), C.byref(out), None, None), "rel_epsilon")
    refused(L.tb_run_compare(ctx, 4, 4, pa, pa, settings(flags=4), C.byref(out), None, None), "unknown flags")
    refused(L.tb_set_reference(ctx, 0, 4, pa), "dimension is 0")
    refused(L.tb_set_reference(ctx, 8193, 8192, pa), "2^26")
    refused(L.tb_compare(ctx, 0, None, None, None, None), "null")
    refused(L.tb_compare(ctx, 2, None, C.byref(out), None, None), "unknown surface")
    refused(L.tb_compare(ctx, 0, settings(flags=3), C.byref(out), None, None), "TB_COMPARE_SUMS")
    test, refi, kw, want = cases.restated("random", 12, 13)
    check(gpu_tb.RunCompare(test, refi, maps=True), want, "after the refusals")
