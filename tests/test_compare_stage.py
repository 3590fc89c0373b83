"""Image-quality metrics, the stage on the GPU: tb_set_reference / tb_compare on the cornell box at 64 x 48 against a reference
rendered with another time seed.  The stage equals the kernel seam on host copies of the same surfaces, bit for bit; unsampled pixels are counted
and left out; nothing the context holds is written; the metric does what it is for; the refusals give their codes."""
import copy

import numpy as np
import pytest

import metrics_ref as ref
from conftest import CORNELL

F32 = np.float32
W, H = 64, 48
REFERENCE_FRAMES = 4096
TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6
FIELDS = ("pixels", "excluded", "unsampled", "ssim_windows", "ssim_windows_skipped", "mse", "mae", "rel_mse", "max_abs", "psnr", "ssim")


@pytest.fixture(scope="module")
def s4(built, settings):
    s = copy.copy(settings); s.MaxBounces = 4; s.EnableBlueNoise = 0
    return s


def mean_of(acc):
    out = np.ones_like(acc)
    with np.errstate(all="ignore"):
        out[..., :3] = acc[..., :3] / acc[..., 3:4]
    return out


@pytest.fixture(scope="module")
def reference(built, s4):
    """the mean of 4096 frames under another time seed, rendered once for the module"""
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(W, H, REFERENCE_FRAMES, s4, 7.0)
        return mean_of(tb.ReadAccumulation())


def bits(v):
    return np.float64(v).view(np.uint64)


def assert_equal_results(got, want, what):
    for k in FIELDS:
        assert bits(got[k]) == bits(want[k]) or (np.isnan(got[k]) and np.isnan(want[k])), "%s: %s = %r, the seam %r" % (what, k, got[k], want[k])
    for k in ("sq_err_map", "ssim_map"):
        assert got[k].shape == want[k].shape and (got[k].view(np.uint32) == want[k].view(np.uint32)).all(), "%s: %s differs" % (what, k)


def refused(call, code, word):
    from tracerboy_amd import api
    with pytest.raises(api.TracerBoyError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.mark.gpu
def test_gpu_stage_equals_the_seam_on_the_mean_and_on_the_denoised_picture(reference, s4):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.SetOption("aov", 1)
        tb.LoadScene(CORNELL)
        tb.Render(W, H, 4, s4, 0.0)
        tb.SetReference(reference)
        got = tb.Compare(0, maps=True)
        assert_equal_results(got, tb.RunCompare(mean_of(tb.ReadAccumulation()), reference, maps=True), "the mean")
        assert got["pixels"] == W * H and got["excluded"] == 0 and got["ssim_windows"] == (W - 10) * (H - 10) and got["gpu_us"] > 0
        assert 0 < got["mse"] and 0 < got["ssim"] < 1 and np.isfinite(got["psnr"])
        s = api.GetDefaultCompareSettings(); s.peak = 2.0; s.rel_epsilon = 0.25; s.flags = 0
        assert_equal_results(tb.Compare(0, s, maps=True), tb.RunCompare(mean_of(tb.ReadAccumulation()), reference, s, maps=True), "the mean, other settings")
        tb.Denoise(read=False)
        denoised = tb.Compare(1, maps=True)
        assert_equal_results(denoised, tb.RunCompare(tb.ReadDenoiseStage(3), reference, maps=True), "the denoised picture")
        assert denoised["mse"] != got["mse"]
        assert_equal_results(tb.Compare(0, maps=True), got, "the mean again")


@pytest.mark.gpu
def test_gpu_unsampled_pixels_are_counted_and_left_out(reference, s4):
    from tracerboy_amd import api
    x0, y0, x1, y1 = 9, 5, 51, 40
    budget = np.zeros((H, W), np.uint32); budget[y0:y1, x0:x1] = 0xffffffff
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.SetSampleBudget(budget)
        tb.Render(W, H, 4, s4, 0.0)
        tb.SetReference(reference)
        got = tb.Compare(0, maps=True)
        acc = tb.ReadAccumulation()
        outside = W * H - (x1 - x0) * (y1 - y0)
        assert (got["pixels"], got["excluded"], got["unsampled"]) == ((x1 - x0) * (y1 - y0), outside, outside)
        s = api.GetDefaultCompareSettings(); s.flags |= 2       # TB_COMPARE_SUMS: the seam on the raw sums
        assert_equal_results(got, tb.RunCompare(acc, reference, s, maps=True), "the window")
        assert got["ssim_windows"] == (x1 - x0 - 10) * (y1 - y0 - 10) and got["ssim_windows_skipped"] == (W - 10) * (H - 10) - got["ssim_windows"]
        assert not got["sq_err_map"][:y0].any() and not got["sq_err_map"][:, x1:].any() and got["sq_err_map"][y0:y1, x0:x1].any()
        # the metrics are the window's: the restatement on the cropped pictures
        want = ref.compare(mean_of(acc)[y0:y1, x0:x1], reference[y0:y1, x0:x1])
        assert got["max_abs"] == want["max_abs"] and got["ssim_windows"] == want["ssim_windows"]
        for k in ("mse", "mae", "rel_mse", "ssim"):
            assert abs(got[k] - want[k]) <= ref.mean_bound(want["sums"][k], got[k], want[k]), k
        assert (got["sq_err_map"][y0:y1, x0:x1].view(np.uint32) == want["sq_err_map"].view(np.uint32)).all()
        assert (got["ssim_map"][y0:y1 - 10, x0:x1 - 10].view(np.uint32) == want["ssim_map"].view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_comparison_writes_nothing_the_context_holds(reference, s4):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(W, H, 8, s4, 0.0)
        uninterrupted = tb.AccumDigest()
        tb.InvalidateHistory()
        tb.Render(W, H, 4, s4, 0.0)
        digest, frames = tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()
        tb.SetReference(reference)
        first = tb.Compare(0, maps=True)
        assert tb.AccumDigest() == digest and tb.GetNumberOfSamplesSinceLastInvalidate() == frames
        tb.Render(W, H, 4, s4, 0.0)
        assert tb.AccumDigest() == uninterrupted, "frames rendered after a comparison are not those of the uninterrupted render"
        assert tb.Compare(0)["mse"] != first["mse"]
        held = tb.GetOption("debug_live_device_bytes")
        tb.Compare(0, maps=True); tb.Compare(0)
        assert tb.GetOption("debug_live_device_bytes") == held, "a comparison of the same size allocated again"
        tb.SetReference(None)
        assert tb.GetOption("debug_live_device_bytes") < held
        refused(lambda: tb.Compare(0), TB_E_INVALID, "no reference")


@pytest.mark.gpu
def test_gpu_more_frames_bring_the_relative_error_down(reference, s4):
    """Variance falls as 1 / n and the reference's own noise adds 1 / 4096 to both: the expected ratio of relMSE at 4 and at 64 frames is
    (1/4 + 1/4096) / (1/64 + 1/4096) = 15.8.  The factor 4 is margin, not a tolerance."""
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.SetReference(reference)
        tb.Render(W, H, 4, s4, 0.0)
        at4 = tb.Compare(0)
        tb.Render(W, H, 60, s4, 0.0)
        at64 = tb.Compare(0)
        print("relMSE at 4 frames %.6g, at 64 frames %.6g: ratio %.2f; PSNR %.2f -> %.2f dB, SSIM %.4f -> %.4f" % (
            at4["rel_mse"], at64["rel_mse"], at4["rel_mse"] / at64["rel_mse"], at4["psnr"], at64["psnr"], at4["ssim"], at64["ssim"]))
        assert at64["rel_mse"] < at4["rel_mse"] / 4.0


@pytest.mark.gpu
def test_gpu_stage_refusals_give_their_codes(reference, s4):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.SetOption("aov", 1)
        tb.LoadScene(CORNELL)
        tb.SetReference(reference)
        refused(lambda: tb.Compare(0), TB_E_INVALID, "nothing rendered")
        tb.Render(W, H, 2, s4, 0.0)
        refused(lambda: tb.Compare(1), TB_E_INVALID, "no valid denoised surface")
        tb.Denoise(read=False)
        tb.Compare(1)
        tb.Render(W, H, 1, s4, 0.0)                             # the accumulation has changed: the denoised surface is stale
        refused(lambda: tb.Compare(1), TB_E_INVALID, "no valid denoised surface")
        refused(lambda: tb.Compare(2), TB_E_INVALID, "unknown surface")
        for bad in (0.0, -1.0, float("nan"), float("inf")):        # the settings' refusals through the stage as through the seam
            s = api.GetDefaultCompareSettings(); s.peak = bad
            refused(lambda: tb.Compare(0, s), TB_E_INVALID, "peak")
            s = api.GetDefaultCompareSettings(); s.rel_epsilon = bad
            refused(lambda: tb.Compare(0, s), TB_E_INVALID, "rel_epsilon")
        s = api.GetDefaultCompareSettings(); s.flags = 4
        refused(lambda: tb.Compare(0, s), TB_E_INVALID, "unknown flags")
        s.flags = 3
        refused(lambda: tb.Compare(0, s), TB_E_INVALID, "TB_COMPARE_SUMS")
        tb.SetReference(reference[:-1])
        refused(lambda: tb.Compare(0), TB_E_INVALID, "the reference is 64 x 47")
        tb.SetReference(reference)
        assert tb.Compare(0)["pixels"] == W * H                  # and the context still works
    with api.TracerBoy(devices=[0, 0]) as g:                     # a two-member group on one device
        g.LoadScene(CORNELL)
        g.Render(W, H, 1, s4, 0.0)
        refused(lambda: g.SetReference(reference), TB_E_UNSUPPORTED, "group")
        refused(lambda: g.Compare(0), TB_E_UNSUPPORTED, "group")
