"""The CLI's sample-budget flags: --crop, --spp-map, --noise-target.  The refusals run without a GPU, on a scene path that
does not exist: status 2 can only come from the argument checks, which stand before the first device call."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, ROOT
from test_render_state import read_pfm

CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
W, H = 64, 48
COMMON = ["--width", str(W), "--height", str(H), "--depth", "3", "--blue-noise", "0"]


def write_pfm(path, red):
    """An RGB .pfm whose red channel is `red` (H, W), row 0 = top (the format stores the bottom row first)."""
    rgb = np.zeros(red.shape + (3,), "<f4"); rgb[..., 0] = red
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (red.shape[1], red.shape[0])); f.write(rgb[::-1].tobytes())


def run(scene, *args):
    return subprocess.run([CLI, scene] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_refusals_before_any_device_call(built, tmp_path):
    absent = os.path.join(ROOT, "tests", "no-such-scene.pbrt")
    small = str(tmp_path / "small.pfm"); write_pfm(small, np.ones((8, 8), np.float32))
    many = str(tmp_path / "many.pfm"); write_pfm(many, (np.arange(W * H, dtype=np.float32) / (W * H)).reshape(H, W))
    write_pfm(str(tmp_path / "ok.pfm"), np.ones((H, W), np.float32))
    cases = [
        (["--crop", "1,2,3"], "--crop is X0,Y0,X1,Y1"), (["--crop", "1,2,3,x"], "--crop is X0,Y0,X1,Y1"), (["--crop", "-1,0,4,4"], "--crop is X0,Y0,X1,Y1"),
        (["--crop", "4,4,4,8"], "--crop is X0,Y0,X1,Y1"), (["--crop", "0,8,4,8"], "--crop is X0,Y0,X1,Y1"),
        (COMMON + ["--crop", "0,0,65,10"], "lies outside the 64x48 frame"), (COMMON + ["--crop", "0,40,10,49"], "lies outside the 64x48 frame"),
        (COMMON + ["--spp-map", small], "is 8x8, the frame 64x48"), (["--spp-map", str(tmp_path / "absent.pfm")], "cannot be read"),
        (COMMON + ["--spp", "4096", "--spp-map", many], "distinct sample counts"),
        (["--noise-target", "0"], "--noise-target is"), (["--noise-target", "-0.1"], "--noise-target is"), (["--noise-target", "nan"], "--noise-target is"),
        (["--noise-target", "inf"], "--noise-target is"), (["--noise-target", "x"], "--noise-target is"),
        (["--noise-target", "0.1", "--noise-chunk", "0"], "--noise-chunk must be at least 1"),
        (["--crop", "0,0,4,4", "--adaptive", "0.5"], "--adaptive-test call"), (["--noise-target", "0.1", "--adaptive", "0.5", "--adaptive-test", "frame"], "--adaptive-test call"),
        (["--crop", "0,0,4,4", "--upscale-neural", str(tmp_path / "absent.bin")], "do not go with --upscale-neural"),
        (["--noise-target", "0.1", "--render-scale", "0.5"], "do not go with --render-scale"),
        (COMMON + ["--spp-map", str(tmp_path / "ok.pfm"), "--frames", "8:16"], "--spp-map does not go with --frames"),
        (["--crop", "0,0,4,4", "--upscale", "128x96", "--out", "x.pfm"], "go with --upscale only for a .png"),
    ]
    for args, message in cases:
        r = run(absent, *args)
        assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and all(f in r.stderr for f in ("--crop", "--spp-map", "--noise-target", "--noise-after", "--noise-chunk"))


@pytest.mark.gpu
def test_crop_equals_the_uncropped_run_inside_and_zero_outside(built, tmp_path):
    full, crop = str(tmp_path / "full.pfm"), str(tmp_path / "crop.pfm")
    assert run(CORNELL, *COMMON, "--spp", 6, "--out", full).returncode == 0
    r = run(CORNELL, *COMMON, "--spp", 6, "--crop", "9,5,41,30", "--out", crop)
    assert r.returncode == 0 and "budget: 6 frames, %d live pixels" % ((41 - 9) * (30 - 5)) in r.stdout, r.stdout + r.stderr
    a, b = read_pfm(full), read_pfm(crop)
    inside = np.zeros((H, W), bool); inside[5:30, 9:41] = True
    assert np.array_equal(a.view(np.uint32)[inside], b.view(np.uint32)[inside]) and not b.view(np.uint32)[~inside].any()
    assert a[inside].max() > 0


@pytest.mark.gpu
def test_spp_map_gives_every_pixel_its_count(built, tmp_path):
    """Three counts (0, 3 and 8 of --spp 8); the state's output surface holds sum w, which the box filter makes the sample count."""
    from tracerboy_amd import api
    red = np.zeros((H, W), np.float32); red[:, 20:40] = 3.0 / 8.0; red[:, 40:] = 2.0     # (saturate: 2 is 1)
    path, state, out = str(tmp_path / "map.pfm"), str(tmp_path / "s.tbs"), str(tmp_path / "m.pfm")
    write_pfm(path, red)
    r = run(CORNELL, *COMMON, "--spp", 8, "--spp-map", path, "--save-state", state, "--out", out)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [(int(f), int(l)) for f, l in re.findall(r"budget: (\d+) frames, (\d+) live pixels", r.stdout)]
    assert lines == [(3, 44 * H), (8, 24 * H)], r.stdout
    info, o, q = api.ReadStateFile(state)
    want = np.zeros((H, W), np.float32); want[:, 20:40] = 3; want[:, 40:] = 8
    assert np.array_equal(o[..., 3], want)
    pic = read_pfm(out)
    assert not pic.view(np.uint32)[:, :20].any() and pic[:, 20:].max() > 0


@pytest.mark.gpu
def test_noise_target_ends_early_and_prints_its_calls(built, tmp_path):
    """The lower half of the frame: the pixels next to the light's edge keep a neighbour's variance in their prefiltered estimate and do not stop
    within thousands of frames -- the window leaves them out, and the flags combine."""
    out = str(tmp_path / "n.pfm")
    r = run(CORNELL, *COMMON, "--spp", 4096, "--crop", "0,24,64,48", "--noise-target", "0.5", "--noise-after", 16, "--noise-chunk", 16, "--out", out)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [(int(f), int(l)) for f, l in re.findall(r"budget: (\d+) frames, (\d+) live pixels", r.stdout)]
    assert lines[0] == (16, W * 24) and [f for f, _ in lines] == list(range(16, 16 * len(lines) + 1, 16)), r.stdout
    live = [l for _, l in lines]
    assert all(a >= b for a, b in zip(live, live[1:])) and lines[-1][0] < 4096, r.stdout[-1500:]     # (measured: every pixel of the window stops at frame 16)
    assert "every pixel has stopped" in r.stdout and os.path.exists(out)
    taken = re.search(r"budget: (\d+) samples taken of the (\d+)", r.stdout)
    assert taken and int(taken.group(1)) == sum(l for _, l in lines) * 16 and int(taken.group(2)) == W * H * lines[-1][0], r.stdout[-600:]
    # one job of an spp split: the noise target is first asked after this run's own first call
    r = run(CORNELL, *COMMON, "--frames", "32:64", "--crop", "0,24,64,48", "--noise-target", "0.5", "--noise-after", 16, "--noise-chunk", 16,
            "--save-state", str(tmp_path / "job.tbs"), "--out", out)
    assert r.returncode == 0 and "budget: 48 frames, %d live pixels" % (W * 24) in r.stdout, r.stdout + r.stderr
    # crop, map-free, with the reference's test per call as well: the flags combine
    r = run(CORNELL, *COMMON, "--spp", 64, "--crop", "0,0,32,48", "--noise-target", "0.5", "--noise-after", 16, "--noise-chunk", 16, "--adaptive", "0.5",
            "--adaptive-after", 16, "--adaptive-chunk", 16, "--adaptive-test", "call", "--out", out)
    assert r.returncode == 0 and "budget: 16 frames, %d live pixels" % (32 * 48) in r.stdout, r.stdout + r.stderr
    assert not read_pfm(out).view(np.uint32)[:, 32:].any()
