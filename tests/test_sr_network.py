"""The neural 2 x super-resolution as a network and as a stage: tb_run_sr, tb_upscale_neural, --upscale-neural.

The weights are the reference's (tests/golden/dml_sr/weights.bin) and two small nets with odd channel counts that the test writes (tests/sr_ref.py).

Composition and the stage are bit-for-bit statements.  The stage's input is what the reference's network reads: the output stage's 8-bit picture,
uint8 / 255, never its float picture.  Against torch the tolerance is measured in the test itself, as section 15 does it: net_ref accumulated in
fp64 and in fp32 are both legitimate evaluations of the layer contract, so e_max = max |ref32 - ref64| and e_rms, its RMS, are what the
accumulation order alone does to this network on this input.  The GPU is compared with the fp64 evaluation -- the same yardstick the fp32 one is
judged by -- and must stay within 4 e_max (floored at one binary16 step of the reference value) and 2 e_rms.

Measured on an MI355X with the reference's weights (GPU max, GPU RMS, e_max, e_rms; every maximum is one binary16 step of an output in 0.5 ... 1):
    24 x 16:   4.88e-04  4.81e-05  4.88e-04  4.50e-05     (the picture spans 0.00 ... 1.04; 3.2 % of ref32 differs from ref64, 3.2 % of the GPU's values)
    5 x 7:     4.88e-04  2.38e-05  4.88e-04  2.38e-05     (0.22 ... 1.02; 0.2 %, 0.2 %)
    17 x 9:    4.88e-04  4.38e-05  4.88e-04  4.92e-05     (0.06 ... 1.07; 1.4 %, 1.3 %)"""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch

import neural_ref as nr
import sr_ref as sr
from conftest import CORNELL, ROOT

pytestmark = pytest.mark.gpu

TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
F32 = np.float32


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    """{name: (folded weights, path of its file)}"""
    d = tmp_path_factory.mktemp("sr_nets")
    out = {"real": (sr.folded_of(sr.read_container(sr.REAL_WEIGHTS)), sr.REAL_WEIGHTS)}
    for name, channels, seed in (("small", sr.SMALL_OUT, 41), ("small2", (33, 3, 70, 5, 1, 7, 3), 42)):
        raw = sr.make_raw(channels, seed)
        p = str(d / (name + ".bin"))
        sr.write_container(p, raw, order=tuple(reversed(sr.LAYERS)) if name == "small2" else None)
        out[name] = (sr.folded_raw(raw), p)
    return out


@pytest.fixture(scope="module")
def s3(built, settings):
    s = copy.copy(settings); s.MaxBounces = 3; s.EnableBlueNoise = 0
    return s


def picture(w, h, seed):
    """(H, W, 4) float32: a smooth field plus 0.1 sigma noise, clamped and quantised to k / 255, alpha 1"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    smooth = np.stack([0.5 + 0.4 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1).astype(F32)
    color = np.clip(smooth + 0.1 * rng.standard_normal((h, w, 3)).astype(F32), 0, 1)
    k = (color * F32(255) + F32(0.5)).astype(np.uint8)
    out = np.ones((h, w, 4), F32)
    out[..., :3] = k.astype(F32) / F32(255)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- composition: bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1], ids=["plain", "staged"])
@pytest.mark.parametrize("net,w,h", [("real", 5, 7), ("small", 17, 9), ("small2", 6, 5), ("real", 1, 1)])
def test_network_is_the_chain_of_its_seams(gpu_tb, nets, net, w, h, form):
    """tb_run_sr against the pack, seven tb_run_conv calls and tb_run_sr_finish, in either form of the convolutions (small2 has a layer of 70
    input channels, more than the staged form holds: it runs in the plain form); and the two forms give the same picture"""
    weights, path = nets[net]
    gpu_tb.LoadUpscaleWeights(path)
    default = gpu_tb.GetOption("sr_conv_form")
    color = picture(w, h, seed=w * 131 + h)
    try:
        gpu_tb.SetOption("sr_conv_form", form)
        assert gpu_tb.GetOption("sr_loaded") == 1 and gpu_tb.GetOption("sr_conv_form") == form
        got = gpu_tb.RunUpscaleNeural(color)
        assert gpu_tb.GetOption("last_sr_us") > 0
        gpu_tb.SetOption("sr_conv_form", 1 - form)
        other = gpu_tb.RunUpscaleNeural(color)
    finally:
        gpu_tb.SetOption("sr_conv_form", default)
    want = sr.net_chain(gpu_tb, weights, sr.pack_input(color), form=form)
    assert got.shape == (2 * h, 2 * w, 4) and same_bits(got, want) and same_bits(got, other) and (got[..., 3] == 1).all()
    with pytest.raises(Exception):
        gpu_tb.SetOption("sr_conv_form", 2)


# ---- against torch: a tolerance measured from the reference's own spread -------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(24, 16), (5, 7), (17, 9)])
def test_network_against_torch(gpu_tb, nets, w, h):
    weights, path = nets["real"]
    gpu_tb.LoadUpscaleWeights(path)
    color = picture(w, h, seed=w + h)
    x = sr.pack_input(color)
    r32 = sr.net_ref(weights, x)[..., :3].astype(np.float64)
    r64 = sr.net_ref(weights, x, accumulate=torch.float64)[..., :3].astype(np.float64)
    gpu = gpu_tb.RunUpscaleNeural(color)[..., :3].astype(np.float64)
    e_max, e_rms = float(np.abs(r32 - r64).max()), float(np.sqrt(np.mean((r32 - r64) ** 2)))
    g_err = np.abs(gpu - r64)
    g_max, g_rms = float(g_err.max()), float(np.sqrt(np.mean(g_err ** 2)))
    step = np.spacing(np.abs(r64).astype(np.float16)).astype(np.float64)        # one binary16 step of the reference value
    print("  %d x %d: GPU max %.3e rms %.3e; e_max %.3e e_rms %.3e; picture in [%.3f, %.3f], %.1f %% of the reference's values differ between fp64 and fp32, "
          "%.1f %% of the GPU's from fp64" % (w, h, g_max, g_rms, e_max, e_rms, r64.min(), r64.max(), 100 * float(np.mean(r64 != r32)), 100 * float(np.mean(gpu != r64))))
    assert np.isfinite(r64).all() and r64.max() > 0.5, "a dead or overflowing network shows nothing"
    assert e_max > 0 and e_rms > 0
    assert (g_err <= np.maximum(4 * e_max, step)).all() and g_rms <= 2 * e_rms


# ---- the stage -----------------------------------------------------------------------------------------------------------------------
def reinhard():
    from tracerboy_amd import api
    ps = api.GetDefaultPostProcessSettings(); ps.TonemapType = 0
    return ps


def stage_color(tb, ps=None):
    """what the network reads: the output stage's 8-bit picture as uint8 -> float32 / float32(255), alpha 1"""
    _, color8 = tb.PostProcess(ps)
    return nr.unorm_color(color8)


def assert_stage(tb, ps=None):
    """tb_upscale_neural = tb_run_sr on the 8-bit picture / 255, bit for bit; its 8-bit picture is the 8-bit store of its float one.  Returns it."""
    got_f, got_b = tb.UpscaleNeural(ps)
    want = tb.RunUpscaleNeural(stage_color(tb, ps))
    assert np.isfinite(got_f).all()
    assert got_f.shape == (2 * tb.height, 2 * tb.width, 4) and same_bits(got_f, want)
    assert np.array_equal(got_b, nr.rgba8_of(got_f)) and float(got_f[..., :3].max()) > 0.05
    return got_f


def test_stage_is_the_network_on_the_8_bit_picture_and_changes_nothing_else(gpu_tb, s3, nets):
    from tracerboy_amd import api
    before = gpu_tb.GetOption("debug_live_device_bytes")
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(64, 48, 8, s3, 0.0)
        uninterrupted = tb.AccumDigest()
        tb.InvalidateHistory()
        tb.Render(64, 48, 4, s3, 0.0)
        tb.LoadUpscaleWeights(nets["real"][1])
        digest, frames = tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()
        f_reinhard = assert_stage(tb, reinhard())
        assert tb.GetOption("last_sr_us") > 0
        assert np.isnan(tb.PostProcess()[0]).any()             # the default AgX: NaN in the float picture where a pixel is black, 0 in the 8-bit one
        f_agx = assert_stage(tb)
        assert not same_bits(f_reinhard, f_agx)
        only_f, none = tb.UpscaleNeural(reinhard(), rgba8=False)
        assert none is None and same_bits(only_f, f_reinhard)
        assert tb.AccumDigest() == digest and tb.GetNumberOfSamplesSinceLastInvalidate() == frames
        held = gpu_tb.GetOption("debug_live_device_bytes")
        tb.UpscaleNeural()                                     # the same size: the buffers are kept
        assert gpu_tb.GetOption("debug_live_device_bytes") == held
        tb.LoadUpscaleWeights(nets["small"][1])                # other weights replace them
        assert_stage(tb, reinhard())
        tb.Render(64, 48, 4, s3, 0.0)
        assert tb.AccumDigest() == uninterrupted, "frames rendered after the network are not those of the uninterrupted render"
        tb.LoadUpscaleWeights(nets["real"][1])
        held = gpu_tb.GetOption("debug_live_device_bytes")
        tb.Render(40, 24, 2, s3, 0.0)                          # another size: the buffers follow
        assert assert_stage(tb, reinhard()).shape == (48, 80, 4)
        assert gpu_tb.GetOption("debug_live_device_bytes") < held
    assert gpu_tb.GetOption("debug_live_device_bytes") == before


def test_refusals(built, s3, nets):
    import ctypes as C
    from tracerboy_amd import api

    def refused(call, code, word):
        with pytest.raises(api.TracerBoyError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        assert tb.GetOption("sr_loaded") == 0
        refused(tb.UpscaleNeural, TB_E_INVALID, "no weights")
        refused(lambda: tb.RunUpscaleNeural(picture(8, 8, 1)), TB_E_INVALID, "no weights")
        tb.width, tb.height = 32, 16
        tb.LoadUpscaleWeights(nets["real"][1])
        refused(tb.UpscaleNeural, TB_E_INVALID, "nothing rendered")
        tb.Render(32, 16, 2, s3, 0.0)
        ps = api.GetDefaultPostProcessSettings()
        assert tb._L.tb_upscale_neural(tb._ctx, C.byref(ps), None, None) == TB_E_INVALID and b"null" in tb._L.tb_last_error(tb._ctx)
        tb.SetOption("post_denoised", 1)
        refused(tb.UpscaleNeural, TB_E_INVALID, "post_denoised")     # what tb_post_process refuses
        tb.SetOption("post_denoised", 0)
        with pytest.raises(api.TracerBoyError) as e:
            tb.LoadUpscaleWeights(os.path.join(ROOT, "README.md"))
        assert e.value.code == -4
        with pytest.raises(api.TracerBoyError) as e:
            tb.LoadUpscaleWeights(os.path.join(ROOT, "no-such-file.bin"))
        assert e.value.code == -3
        assert tb.UpscaleNeural()[0].shape == (32, 64, 4)            # the weights loaded before are still there, and the context works
        out = np.empty(4, F32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert tb._L.tb_run_sr(tb._ctx, 2049, 2048, p(out), p(out)) == TB_E_INVALID and b"2^24" in tb._L.tb_last_error(tb._ctx)   # refused before anything is read
        assert tb._L.tb_run_sr(tb._ctx, 0, 4, p(out), p(out)) == TB_E_INVALID
        assert tb._L.tb_run_sr(tb._ctx, 1, 1, None, p(out)) == TB_E_INVALID and b"null" in tb._L.tb_last_error(tb._ctx)
        tb.Render(2049, 2048, 1, s3, 0.0)                            # more than 2^24 output pixels
        refused(lambda: tb._check(tb._L.tb_upscale_neural(tb._ctx, C.byref(ps), p(out), None)), TB_E_INVALID, "2^24")
    with api.TracerBoy(devices=[0, 0]) as g:                         # a two-member group on one device
        g.LoadScene(CORNELL)
        g.Render(64, 64, 1, s3, 0.0)
        refused(g.UpscaleNeural, TB_E_UNSUPPORTED, "group")


# ---- the command-line tool -----------------------------------------------------------------------------------------------------------
def test_cli_writes_the_picture_of_the_python_path(built, nets, tmp_path):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        s = api.GetDefaultOutputSettings(); s.MaxBounces = 3; s.EnableBlueNoise = 0
        tb.LoadScene(CORNELL)
        tb.Render(64, 48, 4, s, 0.0)
        tb.LoadUpscaleWeights(nets["real"][1])
        want_f, want_b = tb.UpscaleNeural()
    out = str(tmp_path / "up.png")
    r = subprocess.run([CLI, CORNELL, "--width", "64", "--height", "48", "--spp", "4", "--depth", "3", "--blue-noise", "0", "--upscale-neural", nets["real"][1],
                        "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "neural upscale: 64x48 -> 128x96" in r.stdout and "not finite" not in r.stderr, r
    img, _, _ = api.DecodeImage(out)
    assert img.shape == (96, 128, 4)
    assert np.array_equal(np.rint(img[..., :3] * 255).astype(np.uint8), want_b[..., :3]) and int(want_b[..., :3].max()) > 100
    from test_render_state import read_pfm
    out = str(tmp_path / "up.pfm")
    r = subprocess.run([CLI, CORNELL, "--width", "64", "--height", "48", "--spp", "4", "--depth", "3", "--blue-noise", "0", "--upscale-neural", nets["real"][1],
                        "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r
    got = np.ascontiguousarray(read_pfm(out), F32)
    assert got.shape == (96, 128, 3) and same_bits(got, np.ascontiguousarray(want_f[..., :3]))


def test_cli_refuses_combinations_before_any_device_call(built, nets, tmp_path):
    def run(*args):   # a scene that does not exist: status 2 can only come from the argument checks, which stand before the first device call
        return subprocess.run([CLI, os.path.join(ROOT, "tests", "no-such-scene.pbrt")] + list(args), capture_output=True, text=True, timeout=60)
    real = nets["real"][1]
    tza = nr.real_weights_file(tmp_path)
    for extra in (["--upscale", "128x96"], ["--render-scale", "0.5"], ["--denoise-neural", tza], ["--ranks", "2"]):
        r = run("--upscale-neural", real, *extra)
        assert r.returncode == 2 and "--upscale-neural does not go with" in r.stderr, (extra, r)
    r = run("--upscale-neural", str(tmp_path / "absent.bin"))
    assert r.returncode == 2 and "cannot open" in r.stderr, r
    r = run("--upscale-neural", os.path.join(ROOT, "README.md"))
    assert r.returncode == 2 and "--upscale-neural" in r.stderr, r
    assert run("--upscale-neural", real).returncode == 1             # the arguments are fine: the scene is what is missing
    assert "--upscale-neural" in subprocess.run([CLI], capture_output=True, text=True, timeout=60).stderr   # the usage text
