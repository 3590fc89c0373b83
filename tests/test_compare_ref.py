"""Image-quality metrics, the part that needs no GPU: the NumPy restatement (tests/metrics_ref.py) against known answers,
the error of its fp32 SSIM against an fp64 evaluation on the inputs the GPU tests use, the planted exclusion counts, the four entry points
through every layer, and the command-line tool's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compare_cases as cases
import metrics_ref as ref
from conftest import ROOT

F32 = np.float32
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
ENTRY_POINTS = ("tb_default_compare_settings", "tb_run_compare", "tb_set_reference", "tb_compare")


def image(rgb, h=24, w=31):
    out = np.ones((h, w, 4), F32)
    out[..., :3] = rgb
    return out


# ---- the restatement against known answers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (11, 11), (31, 24), (75, 33)], ids=lambda s: "%dx%d" % s)
def test_identical_images_have_no_error_and_every_window_is_exactly_one(size):
    w, h = size
    a = image(np.random.default_rng(w).random((h, w, 3)) * 1.5 - 0.25, h, w)      # some values outside the clamp, too
    r = ref.compare(a, a.copy())
    assert r["mse"] == 0 and r["mae"] == 0 and r["rel_mse"] == 0 and r["max_abs"] == 0 and r["psnr"] == float("inf")
    assert r["pixels"] == w * h and r["excluded"] == 0 and not r["sq_err_map"].any()
    assert r["ssim_windows"] == max(w - 10, 0) * max(h - 10, 0) and r["ssim_windows_skipped"] == 0
    if r["ssim_windows"]:
        assert (r["ssim_map"].view(np.uint32) == F32(1).view(np.uint32)).all() and r["ssim"] == 1.0
    else:
        assert np.isnan(r["ssim"])


@pytest.mark.parametrize("delta", [0.125, -0.03, 1e-3])
def test_a_constant_offset_gives_its_square_its_magnitude_and_its_maximum(delta):
    base = np.random.default_rng(5).random((24, 31, 3)).astype(F32)
    r_img = image(base)
    a_img = image(base + F32(delta))
    d = a_img[..., :3].astype(np.float64) - r_img[..., :3].astype(np.float64)       # delta up to the rounding of R + delta
    assert np.abs(d - delta).max() <= 2.0 ** -24 * 2.0                             # half an ulp of a value below 2
    r = ref.compare(a_img, r_img)
    assert r["mse"] == pytest.approx(float((d * d).mean()), rel=1e-13) and r["mse"] == pytest.approx(delta * delta, rel=1e-3 if abs(delta) < 0.01 else 1e-5)
    assert r["mae"] == pytest.approx(float(np.abs(d).mean()), rel=1e-13) and r["mae"] == pytest.approx(abs(delta), rel=1e-4)
    assert r["max_abs"] == float(np.abs(d).max()) and r["max_abs"] == pytest.approx(abs(delta), rel=1e-3)
    assert r["psnr"] == pytest.approx(10.0 * np.log10(1.0 / r["mse"]), rel=1e-14)
    assert r["rel_mse"] == pytest.approx(float((d * d / (r_img[..., :3].astype(np.float64) ** 2 + np.float64(F32(0.01)))).mean()), rel=1e-13)


@pytest.mark.parametrize("ar", [(0.37, 0.52), (0.0, 1.0), (0.9, 0.9), (0.25, 0.75)])
@pytest.mark.parametrize("peak", [1.0, 2.5])
def test_flat_images_give_the_closed_form(ar, peak):
    a, r = ar
    out = ref.compare(image(a), image(r), peak=peak)
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    fa, fr = float(F32(a)), float(F32(r))
    want = ((2 * fa * fr + c1) * c2) / ((fa * fa + fr * fr + c1) * c2)
    # fp32 rounding: the variances of a flat field are a few ulps of a^2 instead of 0, against C2 = 9e-4 peak^2; twenty-odd roundings of 2^-24 elsewhere
    assert max(np.abs(out["ssim_map"].astype(np.float64) - want).max(), abs(out["ssim"] - want)) <= 4 * 2.0 ** -23 / c2 * max(fa * fa, fr * fr, 1e-3) * want + 32 * 2.0 ** -24


def test_exclusion_follows_the_contract():
    a = image(0.5, 12, 12); r = image(0.25, 12, 12)
    a[0, 0, 3] = np.nan; r[3, 3, 3] = np.inf                       # alpha: ignored
    assert ref.compare(a, r)["excluded"] == 0
    a[5, 5, 1] = np.nan; r[11, 0, 2] = -np.inf
    out = ref.compare(a, r)
    assert (out["pixels"], out["excluded"], out["unsampled"]) == (142, 2, 0)
    assert out["sq_err_map"][5, 5] == 0 and out["sq_err_map"][11, 0] == 0 and out["sq_err_map"][0, 0] == F32(0.0625)
    assert out["ssim_windows"] == 0 and out["ssim_windows_skipped"] == 4 and np.isnan(out["ssim"])     # (5, 5) lies in all four windows
    sums = image(0.5, 12, 12) * F32(3); sums[2, 7] = 0             # an accumulation with one pixel never sampled
    out = ref.compare(sums, r, flags=ref.TB_COMPARE_SSIM | ref.TB_COMPARE_SUMS)
    assert (out["pixels"], out["excluded"], out["unsampled"]) == (142, 2, 1)
    empty = ref.compare(np.full((4, 4, 4), np.nan, F32), image(0.0, 4, 4))
    assert empty["pixels"] == 0 and all(np.isnan(empty[k]) for k in ("mse", "mae", "rel_mse", "max_abs", "psnr", "ssim"))


# ---- the GPU cases, looked at on the CPU --------------------------------------------------------------------------------------------------------
SMALL = [s for s in cases.SIZES if s != (640, 360)]


@pytest.mark.parametrize("size", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_cases_keep_pixels_and_windows_and_hold_the_planted_counts(size):
    w, h = size
    windows = max(w - 10, 0) * max(h - 10, 0)
    for name in cases.names(w, h):
        test, refi, kw, out = cases.restated(name, w, h)
        assert out["pixels"] + out["excluded"] == w * h
        if name == cases.ALL_EXCLUDED:
            assert out["pixels"] == 0 and out["excluded"] == w * h and out["ssim_windows"] == 0 and out["ssim_windows_skipped"] == windows
            continue
        assert out["pixels"] >= 1, name
        if name in ("no_ssim", "sums_no_ssim"):
            assert out["ssim_windows"] == 0 and out["ssim_windows_skipped"] == 0 and np.isnan(out["ssim"])
        else:
            assert out["ssim_windows"] + out["ssim_windows_skipped"] == windows and (out["ssim_windows"] >= 1 or windows == 0), name
        if name.startswith("nonfinite"):
            assert out["excluded"] == len(set(cases.planted_positions(w, h))) and out["unsampled"] == 0, name
            assert windows == 0 or out["ssim_windows_skipped"] >= 1, name
        elif name in ("sums", "sums_no_ssim"):
            assert out["unsampled"] >= (1 if w * h > 1 and (w, h) != (11, 11) else 0)
            assert out["excluded"] == out["unsampled"] == int((test[..., 3] == 0).sum()), name
        else:
            assert out["excluded"] == 0 and out["unsampled"] == 0, name
        if name == "identical":
            assert out["mse"] == 0 and (windows == 0 or (out["ssim"] == 1.0 and (out["ssim_map"] == 1).all()))


FP64_PATTERNS = ["random", "constant", "flat_bright", "identical", "step", "ramp", "checker", "outside", "denormal", "huge", "nan_alpha", "sums", "peak", "nonfinite2",
                 "nonfinite3"]


@pytest.mark.parametrize("name", FP64_PATTERNS)
def test_fp32_ssim_is_close_to_an_fp64_evaluation(name):
    """The fp32 SSIM within 1e-5 of the same definition evaluated in fp64 on the same inputs, and every window within the bound that the
    arithmetic allows it (metrics_ref.ssim_windows: derived from the roundings, not from what the code gives).  A window alone is not held to
    1e-5: where it is flat or nearly so, va = Eaa - ma ma cancels to a few ulps of a^2 and stands beside C2 = 9e-4.  Measured (the test prints
    them): the flat halves of a step up to 7.6e-5 in a window, a ramp up to 8.7e-5, their means 1.2e-6 and 1.7e-6; every other pattern 1.4e-6
    at most in a window and 6e-8 in the mean.  flat_bright (0.37 against 0.52) is the one case whose mean cannot meet 1e-5 in this arithmetic --
    every window is 1.58e-5 off -- and is held to the windows' bound alone, mean included."""
    for (w, h) in ((75, 33), (73, 73), (257, 19)):
        test, refi, kw, out = cases.restated(name, w, h)
        values, skipped, bound = ref.ssim_fp64(test, refi, kw.get("peak", 1.0), kw.get("flags", 1))
        keep = ~skipped
        assert keep.any()
        apart = np.abs(out["ssim_map"].astype(np.float64) - values)
        mean = abs(out["ssim"] - float(values[keep].mean()))
        print("%s %dx%d: fp32 against fp64: largest difference of a window %.3g (largest bound %.3g), of the mean %.3g" % (
            name, w, h, float(apart[keep].max()), float(bound[keep].max()), mean))
        assert mean <= (1e-5 if name != "flat_bright" else float(bound[keep].mean())), (name, w, h, mean)
        assert (apart[keep] <= bound[keep]).all(), (name, w, h, float((apart - bound)[keep].max()))


# ---- every layer declares, exports, binds and wraps the entry points ------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_bound_and_wrapped(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracerboy_hip.h")).read(), flags=re.S)
    L = api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for symbol in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % symbol, header), symbol
        assert hasattr(raw, symbol) and symbol in L._tb_exports, symbol
    assert C.sizeof(abi.tb_compare_settings) == 12 and C.sizeof(abi.tb_compare_result) == 96
    assert abi.tb_compare_result.mse.offset == 40 and abi.tb_compare_result.gpu_us.offset == 88
    assert (abi.TB_COMPARE_SSIM, abi.TB_COMPARE_SUMS, abi.TB_COMPARE_MEAN, abi.TB_COMPARE_DENOISED) == (1, 2, 0, 1)
    s = api.GetDefaultCompareSettings()
    assert (s.peak, s.rel_epsilon, s.flags) == (1.0, F32(0.01), abi.TB_COMPARE_SSIM)
    for method in ("RunCompare", "SetReference", "Compare"):
        assert callable(getattr(api.TracerBoy, method))
    assert api.COMPARE_FIELDS == ("pixels", "excluded", "unsampled", "ssim_windows", "ssim_windows_skipped", "mse", "mae", "rel_mse", "max_abs", "psnr",
                                  "ssim", "gpu_us")


# ---- the command-line tool's refusals, all before any device call ---------------------------------------------------------------------------------
def run_cli(*args):
    """with a scene that does not exist: status 2 can only come from the argument checks, which stand before the first device call"""
    return subprocess.run([CLI, os.path.join(ROOT, "tests", "no-such-scene.pbrt")] + list(args), capture_output=True, text=True, timeout=60)


def test_cli_refuses_metrics_flags_that_do_not_fit(built, tmp_path):
    from tracerboy_amd import api
    reference = str(tmp_path / "reference.pfm")
    api.WriteImage(reference, image(0.5, 6, 8))
    for flags in (("--metrics-every", "2"), ("--metrics-out", str(tmp_path / "m.jsonl")), ("--error-map", str(tmp_path / "e.pfm"))):
        r = run_cli(*flags)
        assert r.returncode == 2 and "need --reference" in r.stderr, (flags, r)
    r = run_cli("--reference", reference, "--width", "16", "--height", "6")
    assert r.returncode == 2 and "is 8x6, the render 16x6" in r.stderr, r
    r = run_cli("--reference", reference, "--metrics-every", "2", "--ranks", "2")
    assert r.returncode == 2 and "--metrics-every does not go with --ranks" in r.stderr, r
    r = run_cli("--reference", reference, "--metrics-every", "0")
    assert r.returncode == 2 and "--metrics-every N needs N >= 1" in r.stderr, r
    r = run_cli("--reference", str(tmp_path / "missing.pfm"))
    assert r.returncode == 2 and "cannot be read as an image" in r.stderr, r
    r = run_cli("--reference", reference, "--error-map", str(tmp_path / "e.png"))
    assert r.returncode == 2 and "--error-map writes a .pfm" in r.stderr, r
    other = str(tmp_path / "other.pfm")
    api.WriteImage(other, image(0.5, 6, 9))
    r = subprocess.run([CLI, "--compare", reference, other], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "is 8x6" in r.stderr and "is 9x6" in r.stderr, r
    r = subprocess.run([CLI, "--compare", reference], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "two image files" in r.stderr, r
    usage = subprocess.run([CLI], capture_output=True, text=True, timeout=60).stderr
    assert "--reference FILE" in usage and "--compare A B" in usage
