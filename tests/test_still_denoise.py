"""The denoise of a progressive render: dual-buffer variance -> 3x3 prefilter -> a-trous passes -> (rgb, 1).

CPU part (-m "not gpu"): the NumPy restatement (tests/still_denoise_ref.py) on halves that are equal, on a seeded Gaussian experiment (the variance
estimate is unbiased) and on the oracle's cornell-box at 16 spp against its own frames [4096, 5120) (relMSE at least halves).
GPU part (-m gpu): dn_kernels.hip and the chain of tb_denoise against the restatement fed with the device's own surfaces and AOVs, bit for bit,
through the C ABI; the invariants and refusals of include/tracerboy_hip.h; the command-line tool."""
import copy
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import still_denoise_ref as ref
from conftest import CORNELL, ROOT

F32 = np.float32
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    """bit-equal, a NaN for a NaN (a host and a device NaN may differ in sign and payload, as in tests/test_math.py)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def denoiser(iterations=5):
    from tracerboy_amd import api
    dn = api.GetDefaultDenoiserSettings()
    dn.WaveletIterations = iterations
    return dn


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------
def test_constant_halves_have_no_variance_and_the_mean_passes_through(built):
    """q = o / 2 exactly (a halving is exact away from the denormals): m = r = n / 2 and o - q = q, so both halves' means have the same bits,
    d = 0, v = 0; without a filter pass final is the mean."""
    rng = np.random.default_rng(5)
    o = np.empty((9, 13, 4), F32)
    o[..., :3] = rng.uniform(0.01, 30.0, (9, 13, 3)); o[..., 3] = rng.integers(1, 40, (9, 13)) * 2
    q = o * F32(0.5)
    prepared = ref.prepare(o, q)
    assert np.all(prepared[..., 3] == 0.0)
    assert same(prepared[..., :3], o[..., :3] / o[..., 3:4])
    z = np.zeros_like(o)
    stages = ref.chain(o, q, z, z, 8, denoiser(0))
    assert stages[2] is None
    assert same(stages[3][..., :3], o[..., :3] / o[..., 3:4]) and np.all(stages[3][..., 3] == 1.0)


def test_prefilter_keeps_a_constant_field(built):
    """The nine weights are 1/16, 1/8 and 1/4 and add up to 1.  For a value whose significand has two bits to spare every partial sum k/16 * c
    is exact, so the field comes back bit for bit; for any other value each of the nine additions rounds once (half a unit in the last place of
    a partial sum no larger than c), so the result is within 9 * 2^-24 of c, relatively -- and clamping makes border pixels no different."""
    for c in (0.0, 0.75, 3.0, 2.0 ** -20, 1.5e10):
        p = np.zeros((6, 7, 4), F32); p[..., 3] = c; p[..., :3] = 0.3
        out = ref.prefilter(p)
        assert same(out, p), c
    for c in (0.1, 1.0 / 3.0, 7.7e-5, 123456.789):
        p = np.zeros((6, 7, 4), F32); p[..., 3] = c; p[..., :3] = 0.3
        out = ref.prefilter(p)
        assert same(out[..., :3], p[..., :3])
        assert np.all(out[..., 3] == out[0, 0, 3]), "border pixels differ from inner ones"
        assert abs(float(out[0, 0, 3]) - float(F32(c))) <= 9 * 2.0 ** -24 * float(F32(c))


def test_variance_estimate_is_unbiased(built):
    """256 x 256 pixels, n = 32 grey samples N(1, 0.5^2), coin 0.5, sample 0 always in the jittered half.  Given m, v = (s^2 / n) * chi^2_1, so
    the mean of v over the pixels with 0 < m < n estimates 0.25 / 32; its relative standard deviation is sqrt(2 / 65536) = 0.55 %, and the
    bound of 3 % is about five of those."""
    rng = np.random.default_rng(1234)
    n, side = 32, 256
    s = rng.normal(1.0, 0.5, (side, side, n))
    coin = rng.uniform(0.0, 1.0, (side, side, n)) < 0.5
    coin[..., 0] = True
    o = np.empty((side, side, 4), F32); q = np.empty_like(o)
    o[..., :3] = s.sum(-1)[..., None]; o[..., 3] = n
    q[..., :3] = (s * coin).sum(-1)[..., None]; q[..., 3] = coin.sum(-1)
    v = ref.prepare(o, q)[..., 3].astype(np.float64)
    both = (q[..., 3] > 0) & (q[..., 3] < n)
    assert both.sum() > 0.999 * side * side                      # m = n needs 31 coins below 0.5
    assert np.all(v[~both] == 0.0)
    mean, want = v[both].mean(), 0.25 / n
    print("mean of v %.6g, sigma^2 / n %.6g, ratio %.4f" % (mean, want, mean / want))
    assert abs(mean - want) <= 0.03 * want


def test_denoised_oracle_render_at_least_halves_the_relative_error(built, cornell_host, settings):
    """cornell-box 128 x 96, MaxBounces 4, blue noise off, time seed 0: the oracle's frames [0, 16) with AOVs and the jittered surface, the chain
    with the default filter settings, against the oracle's frames [4096, 5120).  relMSE(denoised) <= 0.5 * relMSE(raw mean); the ratio measured
    with this restatement is in DESIGN.md section 12."""
    from tracerboy_amd import api
    w, h, spp = 128, 96, 16
    s = copy.copy(settings); s.MaxBounces = 4; s.EnableBlueNoise = 0
    view, pf = cornell_host.view(), cornell_host.frame_constants(s, 0, 0.0)
    low = ol.render(view, pf, w, h, spp, first_frame=0, threads=8, jittered=True, aovs=True)
    truth = ol.render(view, pf, w, h, 1024, first_frame=4096, threads=8)["output"]
    truth = truth[..., :3] / truth[..., 3:4]
    positions = low["worldpos1"] if (spp - 1) % 2 else low["worldpos0"]
    stages = ref.chain(low["output"], low["jittered"], low["normals"], positions, spp, api.GetDefaultDenoiserSettings())
    raw, den = ref.rel_mse(stages[0], truth), ref.rel_mse(stages[3], truth)
    print("relMSE raw %.5f, denoised %.5f, ratio %.3f" % (raw, den, den / raw))
    assert np.all(np.isfinite(stages[3]))
    assert den <= 0.5 * raw


# ---- GPU: tb_denoise against the restatement --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s3(built, settings):
    s = copy.copy(settings); s.MaxBounces = 3; s.EnableBlueNoise = 0
    return s


@pytest.fixture(scope="module")
def aov_tb(built):
    """A context of its own with option "aov" on from the start (the option resets the history; a state that is begun moves the camera's owner)."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    try:
        tb.SetOption("aov", 1)
        tb.LoadScene(CORNELL)
        yield tb
    finally:
        tb.close()


def device_chain(tb, dn):
    """the restatement fed with the device's own surfaces and the AOVs of the last frame"""
    frames = tb.GetNumberOfSamplesSinceLastInvalidate()
    o, q = tb.ReadAccumulation(jittered=True)
    return ref.chain(o, q, tb.ReadAOV(2), tb.ReadAOV(3 + (frames - 1) % 2), frames, dn), o, q


def assert_stages(tb, want, what):
    for stage in range(4):
        if want[stage] is None:
            continue
        got = tb.ReadDenoiseStage(stage)
        bad = ~((bits(got) == bits(want[stage])) | (np.isnan(got) & np.isnan(want[stage])))
        assert not bad.any(), "%s: stage %d differs in %d pixels, first at %s: %s, restatement %s" % (
            what, stage, int(bad.any(-1).sum()), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0][:2])], want[stage][tuple(np.argwhere(bad)[0][:2])])


@pytest.mark.gpu
def test_gpu_chain_is_bit_exact_at_a_ragged_size(aov_tb, s3):
    """100 x 70: ragged against the filter's 8 x 8 tiles and the 256-pixel workgroups of dn_kernels.hip in both directions; the fifth pass's taps
    at +-32 stay inside the frame for some pixels and leave it for others."""
    from tracerboy_amd import _ctypes_abi as abi
    tb, dn = aov_tb, denoiser(5)
    W, H, F = 100, 70, 16
    tb.Render(W, H, F, s3, 0.0)
    final = tb.Denoise(dn)
    want, o, q = device_chain(tb, dn)
    assert_stages(tb, want, "100 x 70")
    assert same(final, want[3]) and np.all(final[..., 3] == 1.0)
    assert tb.GetOption("last_denoise_us") > 0
    halves = (q[..., 3] > 0) & (q[..., 3] < o[..., 3])
    print("pixels with two non-empty halves: %d of %d; largest variance %.4g" % (int(halves.sum()), W * H, float(want[0][..., 3].max())))
    assert halves.sum() > 0.9 * W * H and want[0][..., 3].max() > 0
    # camera rays that missed: no normal, the mean passes through
    miss = ~tb.ReadAOV(2)[..., :3].any(-1)
    print("pixels without a normal: %d" % int(miss.sum()))
    assert same(final[miss][:, :3], tb.ReadDenoiseStage(0)[miss][:, :3])
    # the output stage on the denoised surface, and untouched with the option at 0
    for auto in (0, 1):
        ps = abi.tb_post_settings(1.3, 1, auto, 6, 1.0)
        tb.SetOption("post_denoised", 1)
        try:
            f, b = tb.PostProcess(ps)
            p = ol.post_process(final, ps)
            assert same(f, p["rgba"]) and np.array_equal(b, p["rgba8"])
            if auto:
                assert F32(tb.AveragedLuminance()).view(np.uint32) == F32(p["averaged"]).view(np.uint32)
            tb.PostProcess(ps, outputType=5)                     # LUMINANCE ignores the option
        finally:
            tb.SetOption("post_denoised", 0)
        f, b = tb.PostProcess(ps)
        p = ol.post_process(o, ps, frames_rendered=F)
        assert same(f, p["rgba"]) and np.array_equal(b, p["rgba8"])


@pytest.mark.gpu
def test_gpu_chain_with_degenerate_halves(aov_tb, s3):
    """20 x 12 at 1 spp: frame 0 always lands in the jittered half, so m == n everywhere and no pixel has an estimate; from the second pass on
    most taps fall outside the frame.  Frames 7 and 8 on a begun state: pixels whose two coins both fell above 0.5 have m == 0."""
    tb, dn = aov_tb, denoiser(5)
    W, H = 20, 12
    tb.Render(W, H, 1, s3, 0.0)
    tb.Denoise(dn, read=False)
    want, o, q = device_chain(tb, dn)
    assert np.array_equal(o[..., 3], q[..., 3]) and np.all(want[0][..., 3] == 0.0)
    assert_stages(tb, want, "1 spp")
    tb.BeginAccumulation(W, H, s3, 0.0, first_frame=7)
    tb.Render(W, H, 2, s3, 0.0)
    assert tb.GetNumberOfSamplesSinceLastInvalidate() == 9
    tb.Denoise(dn, read=False)
    want, o, q = device_chain(tb, dn)
    print("m == 0: %d pixels, m == n: %d, of %d" % (int((q[..., 3] == 0).sum()), int((q[..., 3] == o[..., 3]).sum()), W * H))
    assert (q[..., 3] == 0).any() and ((q[..., 3] > 0) & (q[..., 3] < o[..., 3])).any()
    assert_stages(tb, want, "frames [7, 9)")


def edge_surfaces():
    """(output, jittered), 37 x 23: what a render never holds.  Rows 0-3 all zero; 4-7 m = 0; 8-11 m = n; 12-13 n = 0 with colour sums; 14-15
    m > n (r < 0); 16-17 sums near FLT_MAX whose halves differ by 1e38 (d * d overflows); 18 o - q itself overflows (k infinite); 19 denormal
    sums; the rest ordinary halves."""
    rng = np.random.default_rng(77)
    h, w = 23, 37
    o = np.empty((h, w, 4), F32); q = np.empty_like(o)
    o[..., :3] = rng.uniform(0.0, 20.0, (h, w, 3)); o[..., 3] = 8
    q[..., 3] = rng.integers(1, 8, (h, w)); q[..., :3] = o[..., :3] * (q[..., 3:4] / F32(8)) * rng.uniform(0.7, 1.3, (h, w, 3)).astype(F32)
    o[0:4] = 0; q[0:4] = 0
    q[4:8] = 0
    q[8:12] = o[8:12]
    o[12:14, :, 3] = 0; q[12:14, :, 3] = 0
    q[14:16, :, 3] = 11
    o[16:18, :, :3] = F32(3e38) * rng.uniform(0.9, 1.0, (2, w, 3)).astype(F32); o[16:18, :, 3] = 2
    q[16:18, :, :3] = F32(1e37); q[16:18, :, 3] = 1
    o[18, :, :3] = F32(3e38); q[18, :, :3] = F32(-3e38); o[18, :, 3] = 2; q[18, :, 3] = 1
    o[19, :, :3] = F32(3e-41); q[19, :, :3] = F32(1e-41); o[19, :, 3] = 4; q[19, :, 3] = 2
    return o, q


@pytest.mark.gpu
def test_gpu_edge_surfaces_without_aovs(built, settings, tmp_path):
    """Synthetic surfaces through a state file, WaveletIterations = 0: no AOV is needed, stage 2 does not exist."""
    from tracerboy_amd import api
    from test_render_state_host import default_info
    o, q = edge_surfaces()
    with np.errstate(all="ignore"):                              # the surfaces are what they claim: the unguarded estimate is not finite somewhere
        d = ref.luma(q[..., :3] / q[..., 3:4]) - ref.luma((o[..., :3] - q[..., :3]) / (o[..., 3:4] - q[..., 3:4]))
        assert np.isinf(d * d)[16:19].all()
    want = ref.chain(o, q, None, None, 4, denoiser(0))
    assert np.all(np.isfinite(want[0][..., 3])) and np.all(want[0][16:19, :, 3] == 0.0) and want[0][20:, :, 3].max() > 0
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        path = str(tmp_path / "edge.tbs")
        api.WriteStateFile(path, default_info(first=0, next_frame=4, scene_digest=tb.SceneDigest(), settings=settings, camera=tb.GetCamera()), o, q)
        tb.LoadState(path)
        with pytest.raises(api.TracerBoyError) as e:             # filter passes: the state's frames came without AOVs
            tb.Denoise(denoiser(5))
        assert e.value.code == TB_E_INVALID
        final = tb.Denoise(denoiser(0))
        assert_stages(tb, want, "edge surfaces")
        assert same(final, want[3])
        with pytest.raises(api.TracerBoyError) as e:
            tb.ReadDenoiseStage(2)
        assert e.value.code == TB_E_INVALID
        off = denoiser(5); off.Enabled = 0                       # Enabled == 0: the same as no iterations
        assert same(tb.Denoise(off), want[3])


@pytest.mark.gpu
def test_gpu_denoise_leaves_the_render_alone(aov_tb, s3):
    """The digests of the accumulation surfaces do not move; 8 frames, a denoise, 8 more frames have the digests of 16 straight frames; the
    denoised surface of the first 8 is stale after the second 8."""
    from tracerboy_amd import api
    tb = aov_tb
    W, H = 64, 48
    tb.InvalidateHistory()
    tb.Render(W, H, 8, s3, 0.0)
    before = tb.AccumDigest()
    aovs = [tb.ReadAOV(k) for k in (2, 3, 4)]
    tb.Denoise()
    assert tb.AccumDigest() == before and tb.GetNumberOfSamplesSinceLastInvalidate() == 8
    assert all(same(a, tb.ReadAOV(k)) for a, k in zip(aovs, (2, 3, 4)))
    tb.ReadDenoiseStage(3)
    tb.Render(W, H, 8, s3, 0.0)
    interrupted = tb.AccumDigest()
    tb.SetOption("post_denoised", 1)
    try:
        for stale in (lambda: tb.PostProcess(), lambda: tb.ReadDenoiseStage(3)):
            with pytest.raises(api.TracerBoyError) as e:
                stale()
            assert e.value.code == TB_E_INVALID
    finally:
        tb.SetOption("post_denoised", 0)
    tb.InvalidateHistory()
    tb.Render(W, H, 16, s3, 0.0)
    assert tb.AccumDigest() == interrupted
    tb.Denoise(read=False)
    tb.InvalidateHistory()                                       # a history reset invalidates too
    with pytest.raises(api.TracerBoyError) as e:
        tb.ReadDenoiseStage(3)
    assert e.value.code == TB_E_INVALID


@pytest.mark.gpu
def test_gpu_denoise_refusals(aov_tb, s3, tmp_path):
    from tracerboy_amd import api
    W, H = 32, 24

    def refused(call, code, word):
        with pytest.raises(api.TracerBoyError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    with api.TracerBoy(0) as tb:                                 # option "aov" off
        tb.LoadScene(CORNELL)
        tb.width, tb.height = W, H
        refused(lambda: tb.Denoise(), TB_E_INVALID, "nothing rendered")
        tb.SetOption("post_denoised", 1)
        tb.Render(W, H, 2, s3, 0.0)
        refused(lambda: tb.PostProcess(), TB_E_INVALID, "post_denoised")
        tb.SetOption("post_denoised", 0)
        refused(lambda: tb.Denoise(), TB_E_INVALID, "aov")
        refused(lambda: tb.Denoise(denoiser(11)), TB_E_INVALID, "WaveletIterations")
        mean = tb.Denoise(denoiser(0))                           # no filter pass: no AOV needed
        o = tb.ReadAccumulation()
        assert same(mean[..., :3], o[..., :3] / o[..., 3:4])
        tb.RenderRealTime(W, H, s3, None, 0.0)
        refused(lambda: tb.Denoise(denoiser(0)), TB_E_INVALID, "tb_render_realtime")
    tb = aov_tb
    tb.InvalidateHistory()
    tb.Render(W, H, 3, s3, 0.0)
    tb.Denoise(read=False)
    path = str(tmp_path / "three.tbs")
    tb.SaveState(path)
    tb.LoadState(path)                                           # the same frames, without their AOVs
    refused(lambda: tb.ReadDenoiseStage(3), TB_E_INVALID, "tb_denoise")
    refused(lambda: tb.Denoise(), TB_E_INVALID, "tb_state_load")
    tb.BeginAccumulation(W, H, s3, 0.0, first_frame=5)
    refused(lambda: tb.Denoise(denoiser(0)), TB_E_INVALID, "nothing rendered")
    tb.Render(W, H, 1, s3, 0.0)
    tb.Denoise(read=False)                                       # one frame after the begin: its AOVs are there
    with api.TracerBoy(devices=[0, 0]) as g:                     # a two-member group on one device
        g.LoadScene(CORNELL)
        g.Render(64, 64, 1, s3, 0.0)
        refused(lambda: g.Denoise(denoiser(0)), TB_E_UNSUPPORTED, "group")


@pytest.mark.gpu
def test_cli_denoise(aov_tb, s3, tmp_path):
    from test_render_state import read_pfm
    W, H, F = 64, 48, 8
    out = str(tmp_path / "f.pfm")
    common = [CLI, CORNELL, "--width", str(W), "--height", str(H), "--spp", str(F), "--depth", "3", "--blue-noise", "0"]
    r = subprocess.run(common + ["--denoise", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    aov_tb.InvalidateHistory()
    aov_tb.Render(W, H, F, s3, 0.0)
    final = aov_tb.Denoise()
    assert same(read_pfm(out), final[..., :3])
    r = subprocess.run(common + ["--ranks", "2", "--denoise", "--out", str(tmp_path / "r.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--denoise" in r.stderr and not os.path.exists(str(tmp_path / "r.pfm")), r.stdout + r.stderr
