"""The neural still denoiser as a network and as a stage: tb_run_neural, tb_denoise_neural, --denoise-neural.

The weights are OIDN's rt_ldr_alb_nrm.tza (tests/golden/oidn/, joined from its two parts) and two small nets the test writes
(tests/neural_ref.py), He-scaled so that activations keep their scale through the 16 layers.

Composition, padding and the stage are bit-for-bit statements.  The stage's colour input is what the reference's network reads: the output stage's
8-bit picture, uint8 / 255 (stage_color), never its float picture.  Against torch the tolerance is measured in the test itself: net_ref accumulated
in fp64 and in fp32 are both legitimate evaluations of the layer contract, so e_max = max |ref64 - ref32| and e_rms, its RMS, are what the
accumulation order alone does to this network on this input -- single rounding steps of the binary16 outputs.  The GPU must stay within 4 e_max
(e_max is a sample maximum of single-step flips, and a second flip can stack) and 2 e_rms (a wiring or layout error moves the RMS by orders of
magnitude, not by a factor).

Measured on an MI355X (GPU max, GPU RMS, e_max, e_rms), OIDN's weights:
    synthetic 48 x 32:                        9.77e-04  1.95e-04  9.77e-04  2.04e-04     (the picture spans 0.32 ... 1.04; 19 % of ref64 differs from ref32)
    cornell box 64 x 48, 4 spp, Reinhard:     4.88e-04  9.61e-05  9.77e-04  9.94e-05     (0 ... 1.03; 27 %; colour = the 8-bit picture / 255)
    320 x 16 with a NaN or +inf at (160, 8),
    the 2336 pixels outside the mask:         9.77e-04  1.90e-04  9.77e-04  1.89e-04
A step of the binary16 outputs is 2^-11 between 0.5 and 1 and 2^-10 between 1 and 2: each maximum is one step."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch

import neural_ref as nr
import still_guides_ref as guides_ref
from conftest import CORNELL, ROOT

pytestmark = pytest.mark.gpu

TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
F32 = np.float32


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    """{name: (weights, path of its TZA file)}"""
    d = tmp_path_factory.mktemp("nets")
    made = {"small9": nr.make_weights(9, nr.SMALL_OUT, seed=22), "small3": nr.make_weights(3, nr.SMALL_OUT, seed=23)}
    real = nr.real_weights_file(d)
    out = {"real": (nr.weights_of(nr.read_tza(real)), real)}
    for name, w in made.items():
        p = str(d / (name + ".tza"))
        nr.write_tza(p, w, f32=("enc_conv3",) if name == "small9" else ())
        out[name] = (w, p)
    return out


@pytest.fixture(scope="module")
def s3(built, settings):
    s = copy.copy(settings); s.MaxBounces = 3; s.EnableBlueNoise = 0
    return s


def surfaces(w, h, seed, planes=3):
    """colour, albedo, normal as (H, W, 4) float32: a smooth field plus 0.3 sigma colour noise clamped to [0, 1], a smooth albedo, unit normals"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    smooth = np.stack([0.5 + 0.4 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1).astype(F32)
    color = np.clip(smooth + 0.3 * rng.standard_normal((h, w, 3)).astype(F32), 0, 1)
    albedo = np.stack([0.5 + 0.3 * np.cos(x / 11.0 + 2 * c) * np.sin(y / 9.0 + c) for c in range(3)], -1).astype(F32)
    n = np.stack([np.sin(x / 6.0), np.cos(y / 8.0), np.ones_like(x)], -1).astype(F32)
    n /= np.sqrt((n * n).sum(-1, keepdims=True))
    rgba = lambda a: np.concatenate([a, np.ones((h, w, 1), F32)], -1).astype(F32)
    return [rgba(color), rgba(albedo), rgba(n)][:planes]


def halves(rgba):
    """the picture tb_run_neural returns as the binary16 values it holds"""
    assert np.all(rgba[..., 3] == 1.0)
    h = rgba[..., :3].astype(np.float16)
    assert np.array_equal(h.astype(F32), rgba[..., :3], equal_nan=True), "the result is not a picture of binary16 values"
    return h


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


# ---- composition and padding: bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,w,h", [("real", 16, 16), ("real", 48, 32), ("small9", 32, 48), ("small3", 16, 32), ("real", 21, 19), ("real", 1, 1)],
                         ids=["real-16x16", "real-48x32", "small-32x48", "small3-16x32", "real-21x19-padded", "real-1x1-padded"])
def test_network_is_the_chain_of_its_layers(gpu_tb, nets, net, w, h):
    """tb_run_neural against 16 tb_run_conv3x3 calls on the packed, zero-extended input, cropped (16 x 16: the deepest level is 1 x 1)"""
    weights, path = nets[net]
    gpu_tb.LoadNeuralWeights(path)
    planes = surfaces(w, h, seed=w * 131 + h, planes=1 if net == "small3" else 3)
    assert gpu_tb.GetOption("neural_inputs") == 3 * len(planes)
    got = halves(gpu_tb.RunNeural(*planes))
    want = nr.net_chain(gpu_tb, weights, nr.pack_input(*planes))
    assert got.shape == (h, w, 3) and float(want.astype(F32).max()) > 0, "a dead network shows nothing"
    assert same_bits(got, want)
    assert gpu_tb.GetOption("last_neural_us") > 0


def test_padding_is_zero_extension(gpu_tb, nets):
    """21 x 19 equals the 32 x 32 picture that holds it in its corner and zeros elsewhere, cropped"""
    weights, path = nets["real"]
    gpu_tb.LoadNeuralWeights(path)
    planes = surfaces(21, 19, seed=5)
    big = [np.pad(p, ((0, 13), (0, 11), (0, 0))) for p in planes]
    assert same_bits(halves(gpu_tb.RunNeural(*planes)), np.ascontiguousarray(halves(gpu_tb.RunNeural(*big))[:19, :21]))


# ---- against torch: a tolerance measured from the reference's own spread ---------------------------------------------------------------
def against_torch(tb, weights, planes, label):
    x = nr.pack_input(*planes)
    r32 = nr.net_ref(weights, x).astype(np.float64)
    r64 = nr.net_ref(weights, x, accumulate=torch.float64).astype(np.float64)
    gpu = halves(tb.RunNeural(*planes)).astype(np.float64)
    e_max, e_rms = float(np.abs(r64 - r32).max()), float(np.sqrt(np.mean((r64 - r32) ** 2)))
    g_max, g_rms = float(np.abs(gpu - r32).max()), float(np.sqrt(np.mean((gpu - r32) ** 2)))
    print("  %s: GPU max %.3e rms %.3e; e_max %.3e e_rms %.3e; picture in [%.3f, %.3f], %d %% of the reference's elements differ between fp64 and fp32" % (
        label, g_max, g_rms, e_max, e_rms, r32.min(), r32.max(), round(100 * float(np.mean(r64 != r32)))))
    assert np.isfinite(r32).all() and r32.max() > 0.05, "a dead or overflowing network shows nothing"
    assert e_max > 0 and e_rms > 0
    assert g_max <= 4 * e_max and g_rms <= 2 * e_rms


def test_network_against_torch_on_a_synthetic_picture(gpu_tb, nets):
    weights, path = nets["real"]
    gpu_tb.LoadNeuralWeights(path)
    against_torch(gpu_tb, weights, surfaces(48, 32, seed=9), "synthetic 48 x 32")


@pytest.fixture(scope="module")
def cornell(built, s3, nets):
    """a context with a 64 x 48 cornell box at 4 spp, 4 guide frames and OIDN's weights"""
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(64, 48, 4, s3, 0.0)
        tb.RenderGuides(0, 4)
        tb.LoadNeuralWeights(nets["real"][1])
        yield tb


def reinhard():
    """Post settings whose float picture is finite.  The default tonemapper, AgX punchy, raises a negative number to a power where a pixel is
    black (agxDefaultContrastApproximation(0) = -0.00232), as the reference's does: NaN in the float picture, 0 in the 8-bit one, which is what
    the network reads (test_stage_at_the_default_post_settings_is_finite)."""
    from tracerboy_amd import api
    ps = api.GetDefaultPostProcessSettings(); ps.TonemapType = 0
    return ps


def stage_color(tb, ps=None):
    """what the reference's network reads (its post-process surface is R8G8B8A8_UNORM: TracerBoy.cpp:3817-3829, D3D12App.cpp:3, :3309-3318,
    ImageToTensorCS.hlsl:22-32): the output stage's 8-bit picture as uint8 -> float32 / float32(255), alpha 1"""
    _, color8 = tb.PostProcess(ps)
    return nr.unorm_color(color8)


def stage_inputs(tb, ps=None):
    """host copies of what tb_denoise_neural reads: the output stage's 8-bit picture / 255, albedo = A.xyz / A.w, the normals of denoise_guides = 1"""
    A, N, P = (tb.ReadGuide(i) for i in range(3))
    albedo = np.ones_like(A); albedo[..., :3] = A[..., :3] / A[..., 3:4]
    normal, _ = guides_ref.resolve(N, P)
    return stage_color(tb, ps), albedo.astype(F32), normal.astype(F32)


def test_network_against_torch_on_a_render(cornell, nets):
    against_torch(cornell, nets["real"][0], stage_inputs(cornell, reinhard()), "cornell box 64 x 48")


# ---- a non-finite input stays in its receptive field -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field(nets):
    """320 x 16 surfaces, and the reference's clean results in fp32 and fp64 accumulation"""
    weights = nets["real"][0]
    clean = surfaces(320, 16, seed=31)
    x = nr.pack_input(*clean)
    return clean, nr.net_ref(weights, x), nr.net_ref(weights, x, accumulate=torch.float64)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_input_stays_in_its_receptive_field(gpu_tb, nets, field, bad):
    """One colour channel of pixel (160, 8) of 320 x 16 is NaN or +inf.  The network's receptive field is about 95 pixels each way: the reference
    (net_ref) turns columns 81 ... 254 of every row into NaN -- an infinity too: no infinity survives -- and leaves 45.6 % of the picture as it was.
    The GPU must lose exactly those pixels, and give the others as in its own clean run made AFTERWARDS in the same context (the ping-pong and
    skip buffers are reused: a stale NaN would show), and within the 4 e_max / 2 e_rms statement of against_torch."""
    weights, path = nets["real"]
    clean, ref_clean, ref64_clean = field
    poisoned = [p.copy() for p in clean]; poisoned[0][8, 160, 1] = bad
    x = nr.pack_input(*poisoned)
    r32, r64 = nr.net_ref(weights, x), nr.net_ref(weights, x, accumulate=torch.float64)
    mask = np.isnan(r32).any(-1)
    ok = ~mask
    print("  %s at (160, 8): the reference loses %d of %d pixels, columns %d ... %d; %.1f %% stay" % (
        bad, mask.sum(), mask.size, np.flatnonzero(mask.any(0)).min(), np.flatnonzero(mask.any(0)).max(), 100 * ok.mean()))
    # the condition: the reference alone leaves enough of the picture, untouched, to show anything
    assert mask[8, 160] and ok.mean() >= 0.40 and not np.isinf(r32.astype(F32)).any()
    assert same_bits(r32[ok], ref_clean[ok]) and np.array_equal(np.isnan(r64).any(-1), mask) and same_bits(r64[ok], ref64_clean[ok])
    gpu_tb.LoadNeuralWeights(path)
    got = halves(gpu_tb.RunNeural(*poisoned))
    got_clean = halves(gpu_tb.RunNeural(*clean))                      # after the poisoned run, on the same activation buffers
    assert np.isfinite(got_clean.astype(F32)).all()
    lost = np.isnan(got).any(-1)
    assert np.array_equal(lost, mask), "the GPU loses %d pixels, the reference %d; %d differ" % (lost.sum(), mask.sum(), (lost != mask).sum())
    assert same_bits(got[ok], got_clean[ok])
    r32, r64, g = (a[ok].astype(np.float64) for a in (r32, r64, got))
    e_max, e_rms = float(np.abs(r64 - r32).max()), float(np.sqrt(np.mean((r64 - r32) ** 2)))
    g_max, g_rms = float(np.abs(g - r32).max()), float(np.sqrt(np.mean((g - r32) ** 2)))
    print("  outside the mask: GPU max %.3e rms %.3e; e_max %.3e e_rms %.3e" % (g_max, g_rms, e_max, e_rms))
    assert e_max > 0 and e_rms > 0 and g_max <= 4 * e_max and g_rms <= 2 * e_rms


# ---- the stage -------------------------------------------------------------------------------------------------------------------------
def assert_stage(tb, ps=None):
    """tb_denoise_neural = tb_run_neural on the stage inputs, bit for bit; its 8-bit picture is the 8-bit store of its float one.  Returns it."""
    got_f, got_b = tb.DenoiseNeural(ps)
    want = tb.RunNeural(*stage_inputs(tb, ps)) if tb.GetOption("neural_inputs") == 9 else tb.RunNeural(stage_color(tb, ps))
    bad = int((~np.isfinite(got_f)).sum())
    print("  stage %d x %d: %d of %d values are not finite" % (got_f.shape[1], got_f.shape[0], bad, got_f.size))
    assert bad == 0, "%d of %d values of the stage's picture are not finite" % (bad, got_f.size)
    assert got_f.shape == (tb.height, tb.width, 4) and np.array_equal(got_f.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_b, nr.rgba8_of(got_f)) and float(got_f[..., :3].max()) > 0.05
    return got_f


def test_stage_at_the_default_post_settings_is_finite(cornell):
    """AgX punchy on the cornell box: the float picture holds NaN where a pixel is black, the 8-bit one 0 -- and the 8-bit one is what goes in"""
    f, b = cornell.PostProcess()
    nan = np.isnan(f[..., :3])
    assert nan.any(), "no NaN in the float picture: this test shows nothing"
    assert (b[..., :3][nan] == 0).all()
    assert_stage(cornell)


def test_stage_with_one_guide_frame_and_at_a_ragged_size(built, s3, nets):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.LoadNeuralWeights(nets["real"][1])
        tb.Render(64, 48, 4, s3, 0.0)
        tb.RenderGuides(0, 1)                                  # one frame: hits is 0 or 1, the normals are divided and not brought to length 1
        hits = tb.ReadGuide(1)[..., 3]
        assert hits.max() == 1
        for ps in (reinhard(), None):
            assert_stage(tb, ps)
        tb.Render(45, 27, 2, s3, 0.0)                          # ragged against 16 both ways: 48 x 32 inside
        tb.RenderGuides(0, 2)
        assert tb.ReadGuide(1)[..., 3].max() == 2
        for ps in (reinhard(), None):
            assert assert_stage(tb, ps).shape == (27, 45, 4)


def test_stage_is_the_network_on_the_stage_inputs_and_changes_nothing_else(gpu_tb, s3, nets):
    from tracerboy_amd import api
    before = gpu_tb.GetOption("debug_live_device_bytes")
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(64, 48, 8, s3, 0.0)
        uninterrupted = tb.AccumDigest()
        tb.InvalidateHistory()
        tb.Render(64, 48, 4, s3, 0.0)
        tb.RenderGuides(0, 4)
        tb.LoadNeuralWeights(nets["real"][1])
        digest, frames = tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()
        guides = [tb.ReadGuide(i) for i in range(3)]
        ps = reinhard()
        got_f, got_b = tb.DenoiseNeural(ps)
        assert tb.GetOption("last_neural_us") > 0 and tb.GetOption("neural_inputs") == 9
        want = tb.RunNeural(*stage_inputs(tb, ps))
        assert np.array_equal(got_f.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got_b, nr.rgba8_of(got_f))
        assert float(got_f[..., :3].max()) > 0.05
        only_f, none = tb.DenoiseNeural(ps, rgba8=False)
        assert none is None and np.array_equal(only_f.view(np.uint32), want.view(np.uint32))
        assert_stage(tb)                                       # the default post settings: NaN in the float picture, none in the result
        assert tb.AccumDigest() == digest and tb.GetNumberOfSamplesSinceLastInvalidate() == frames
        assert all(np.array_equal(tb.ReadGuide(i), g) for i, g in enumerate(guides))
        held = gpu_tb.GetOption("debug_live_device_bytes")
        tb.DenoiseNeural()                                     # the same size: the activation buffers are kept
        assert gpu_tb.GetOption("debug_live_device_bytes") == held
        # 3-input weights replace the others: no guides are read
        tb.LoadNeuralWeights(nets["small3"][1])
        got3, _ = tb.DenoiseNeural(ps)
        assert np.array_equal(got3.view(np.uint32), tb.RunNeural(stage_color(tb, ps)).view(np.uint32)) and np.isfinite(got3).all()
        tb.Render(64, 48, 4, s3, 0.0)
        assert tb.AccumDigest() == uninterrupted, "frames rendered after the network are not those of the uninterrupted render"
        # another size: the buffers follow
        tb.Render(40, 24, 2, s3, 0.0)
        got, _ = tb.DenoiseNeural(ps)
        assert got.shape == (24, 40, 4) and np.array_equal(got.view(np.uint32), tb.RunNeural(stage_color(tb, ps)).view(np.uint32))
    assert gpu_tb.GetOption("debug_live_device_bytes") == before


def test_stage_refusals(built, s3, nets):
    from tracerboy_amd import api

    def refused(call, code, word):
        with pytest.raises(api.TracerBoyError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        refused(tb.DenoiseNeural, TB_E_INVALID, "no weights")
        tb.width, tb.height = 32, 16
        tb.LoadNeuralWeights(nets["real"][1])
        refused(tb.DenoiseNeural, TB_E_INVALID, "nothing rendered")
        tb.Render(32, 16, 2, s3, 0.0)
        refused(tb.DenoiseNeural, TB_E_INVALID, "tb_render_guides")
        ps = api.GetDefaultPostProcessSettings()
        import ctypes as C
        assert tb._L.tb_denoise_neural(tb._ctx, C.byref(ps), None, None) == TB_E_INVALID and b"null" in tb._L.tb_last_error(tb._ctx)
        tb.RenderGuides(0, 2)
        tb.SetOption("post_denoised", 1)
        refused(tb.DenoiseNeural, TB_E_INVALID, "post_denoised")     # what tb_post_process refuses
        tb.SetOption("post_denoised", 0)
        color, albedo, normal = surfaces(32, 16, seed=1)
        refused(lambda: tb.RunNeural(color), TB_E_INVALID, "9 inputs")
        with pytest.raises(api.TracerBoyError) as e:
            tb.LoadNeuralWeights(os.path.join(ROOT, "README.md"))
        assert e.value.code == -4 and "magic" in str(e.value)
        assert tb.DenoiseNeural()[0].shape == (16, 32, 4)            # the weights loaded before are still there, and the context works
        tb.LoadNeuralWeights(nets["small3"][1])
        refused(lambda: tb.RunNeural(color, albedo, normal), TB_E_INVALID, "3 inputs")
    with api.TracerBoy(0) as tb:
        refused(lambda: tb.RunNeural(*surfaces(8, 8, seed=2)), TB_E_INVALID, "no weights")
    with api.TracerBoy(devices=[0, 0]) as g:                         # a two-member group on one device
        g.LoadScene(CORNELL)
        g.Render(64, 64, 1, s3, 0.0)
        refused(g.DenoiseNeural, TB_E_UNSUPPORTED, "group")


# ---- the command-line tool -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_picture_of_the_python_path(built, nets, tmp_path):
    from tracerboy_amd import api
    from test_render_state import read_pfm
    with api.TracerBoy(0) as tb:
        s = api.GetDefaultOutputSettings(); s.MaxBounces = 3; s.EnableBlueNoise = 0
        tb.LoadScene(CORNELL)
        tb.Render(64, 48, 4, s, 0.0)
        tb.RenderGuides(0, 4)
        tb.LoadNeuralWeights(nets["real"][1])
        wants = [tb.DenoiseNeural(ps, rgba8=False)[0] for ps in (reinhard(), None)]
        assert np.isnan(tb.PostProcess()[0]).any()              # the default tonemapper's float picture is not finite: the network's is
    for tonemap, want in zip((["--tonemap", "0"], []), wants):   # Reinhard, and the tool's defaults
        out = str(tmp_path / ("neural%d.pfm" % len(tonemap)))
        r = subprocess.run([CLI, CORNELL, "--width", "64", "--height", "48", "--spp", "4", "--depth", "3", "--blue-noise", "0", "--denoise-neural", nets["real"][1],
                            "--denoise-guides", "4"] + tonemap + ["--out", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "neural denoise: 9 input channels" in r.stdout and "not finite" not in r.stderr, r
        assert np.isfinite(want).all() and float(want[..., :3].max()) > 0.05
        got = np.ascontiguousarray(read_pfm(out), F32)
        assert got.shape == (48, 64, 3) and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))


def test_cli_refuses_combinations_before_any_device_call(built, nets, tmp_path):
    def run(*args):   # a scene that does not exist: status 2 can only come from the argument checks, which stand before the first device call
        return subprocess.run([CLI, os.path.join(ROOT, "tests", "no-such-scene.pbrt")] + list(args), capture_output=True, text=True, timeout=60)
    nine, three = nets["real"][1], nets["small3"][1]
    for extra in (["--upscale", "128x96"], ["--render-scale", "0.5"], ["--denoise"], ["--denoise-iterations", "2"], ["--ranks", "2"]):
        r = run("--denoise-neural", nine, *extra)
        assert r.returncode == 2 and "--denoise-neural does not go with" in r.stderr, (extra, r)
    r = run("--denoise-neural", three, "--denoise-guides", "4")
    assert r.returncode == 2 and "3 inputs" in r.stderr, r
    r = run("--denoise-neural", str(tmp_path / "absent.tza"))
    assert r.returncode == 2 and "cannot open" in r.stderr, r
    r = run("--denoise-neural", os.path.join(ROOT, "README.md"))
    assert r.returncode == 2 and "magic" in r.stderr, r
    assert run("--denoise-neural", nine).returncode == 1             # the arguments are fine: the scene is what is missing
    assert "--denoise-neural" in subprocess.run([CLI], capture_output=True, text=True, timeout=60).stderr   # the usage text
