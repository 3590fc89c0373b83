"""The CLI's image-quality flags on the GPU: --reference, --metrics-out, --metrics-every, --error-map and --compare A B, against
the Python API on the same render.  (The refusals need no GPU: tests/test_compare_ref.py.)"""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, ROOT
from test_render_state import read_pfm

F32 = np.float32
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
W, H = 64, 48
COMMON = ["--width", str(W), "--height", str(H), "--depth", "3", "--blue-noise", "0"]
FIELDS = ("pixels", "excluded", "unsampled", "ssim_windows", "ssim_windows_skipped", "mse", "mae", "rel_mse", "max_abs", "psnr", "ssim")


def run(*args):
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def lines_of(path):
    with open(path) as f:
        return [json.loads(line) for line in f.read().splitlines()]


def assert_line_is(line, result, frames, surface):
    assert line["frames"] == frames and line["surface"] == surface, line
    for k in FIELDS:
        want = result[k]
        if isinstance(want, float) and not np.isfinite(want):
            assert line[k] is None, (k, line[k], want)
        else:
            assert line[k] == want, (k, line[k], want)          # %.17g reads back as the same double
    assert line["gpu_us"] > 0


@pytest.fixture(scope="module")
def rendered(built, settings, tmp_path_factory):
    """a reference file (32 frames under another time seed, written by the tool itself) and the API's results on the render the tests repeat"""
    from tracerboy_amd import api
    d = tmp_path_factory.mktemp("compare_cli")
    reference = str(d / "reference.pfm")
    run(CORNELL, *COMMON, "--spp", 32, "--seed-time", 5, "--out", reference)
    ref_image = api.DecodeImage(reference)[0]
    s = copy.copy(settings); s.MaxBounces = 3; s.EnableBlueNoise = 0
    with api.TracerBoy(0) as tb:
        tb.SetOption("aov", 1)               # as --denoise renders; the accumulation does not depend on it
        tb.LoadScene(CORNELL)
        tb.Render(W, H, 6, s, 0.0)
        tb.SetReference(ref_image)
        mean = tb.Compare(0, maps=True)
        tb.Denoise(read=False)
        denoised = tb.Compare(1, maps=True)
    return dict(dir=d, reference=reference, ref_image=ref_image, mean=mean, denoised=denoised)


@pytest.mark.gpu
def test_gpu_cli_writes_the_convergence_curve_and_changes_no_pixel(rendered):
    d = rendered["dir"]
    plain, curve, out = str(d / "plain.pfm"), str(d / "curve.pfm"), str(d / "curve.jsonl")
    run(CORNELL, *COMMON, "--spp", 6, "--out", plain)
    run(CORNELL, *COMMON, "--spp", 6, "--out", curve, "--reference", rendered["reference"], "--metrics-every", 2, "--metrics-out", out)
    lines = lines_of(out)
    assert [l["frames"] for l in lines] == [2, 4, 6] and all(l["surface"] == "mean" for l in lines)      # the final line is the last call's: not repeated
    assert_line_is(lines[-1], rendered["mean"], 6, "mean")
    assert lines[0]["rel_mse"] > lines[1]["rel_mse"] > lines[2]["rel_mse"]
    assert open(plain, "rb").read() == open(curve, "rb").read(), "the metrics flags changed the picture"
    # without --metrics-every: one line, on standard output without --metrics-out
    r = run(CORNELL, *COMMON, "--spp", 6, "--out", curve, "--reference", rendered["reference"])
    printed = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(printed) == 1
    assert_line_is(printed[0], rendered["mean"], 6, "mean")
    assert open(plain, "rb").read() == open(curve, "rb").read()


@pytest.mark.gpu
def test_gpu_cli_error_map_and_the_denoised_line(rendered):
    d = rendered["dir"]
    out, emap, picture = str(d / "final.jsonl"), str(d / "error.pfm"), str(d / "final.pfm")
    run(CORNELL, *COMMON, "--spp", 6, "--out", picture, "--reference", rendered["reference"], "--metrics-out", out, "--error-map", emap)
    lines = lines_of(out)
    assert len(lines) == 1
    assert_line_is(lines[0], rendered["mean"], 6, "mean")
    got = read_pfm(emap)
    want = rendered["mean"]["sq_err_map"]
    assert got.shape == (H, W, 3) and all((got[..., c].view(np.uint32) == want.view(np.uint32)).all() for c in range(3))
    run(CORNELL, *COMMON, "--spp", 6, "--out", picture, "--denoise", "--reference", rendered["reference"], "--metrics-out", out, "--error-map", emap)
    lines = lines_of(out)
    assert len(lines) == 2
    assert_line_is(lines[0], rendered["mean"], 6, "mean")
    assert_line_is(lines[1], rendered["denoised"], 6, "denoised")
    got = read_pfm(emap)
    assert (got[..., 1].view(np.uint32) == rendered["denoised"]["sq_err_map"].view(np.uint32)).all()     # the last line's map


@pytest.mark.gpu
def test_gpu_cli_compares_two_files(rendered, gpu_tb):
    from tracerboy_amd import api
    d = rendered["dir"]
    a, b, out = str(d / "a.pfm"), str(d / "b.pfm"), str(d / "files.jsonl")
    rng = np.random.default_rng(11)
    img_a = np.ones((33, 75, 4), F32); img_a[..., :3] = rng.random((33, 75, 3))
    img_b = np.ones((33, 75, 4), F32); img_b[..., :3] = rng.random((33, 75, 3)); img_b[4, 9, 1] = np.nan
    api.WriteImage(a, img_a); api.WriteImage(b, img_b)
    want = gpu_tb.RunCompare(api.DecodeImage(a)[0], api.DecodeImage(b)[0])
    assert want["excluded"] == 1
    r = run("--compare", a, b)
    printed = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(printed) == 1
    assert_line_is(printed[0], want, 0, "files")
    run("--compare", a, b, "--metrics-out", out)
    assert_line_is(lines_of(out)[0], want, 0, "files")
