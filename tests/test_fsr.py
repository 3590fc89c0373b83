"""FSR 1 upscaling: EASU + RCAS behind the output stage.

CPU part (-m "not gpu"): tb_fsr_constants against the NumPy restatement (tests/fsr_ref.py); properties that pin the restatement's reading of the
shader; pre-checks that the GPU cases reach the branches they are meant to reach; the ABI mirror; the command-line tool's refusals.
GPU part (-m gpu): fsr_kernels.hip through tb_run_fsr_easu / tb_run_fsr_rcas and the stage tb_upscale against the restatement, bit for bit (or NaN
on both sides), for both surface types; the invariants and refusals of include/tracerboy_hip.h."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fsr_ref as ref
from conftest import CORNELL, ROOT

F32 = np.float32
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
TB_E_INVALID = -1
# (in_w, in_h, out_w, out_h): 1:1, a single texel, ragged against the 16 x 16 output tile in both directions, more than one tile, one-texel-wide frames
SIZES = [(1, 1, 1, 1), (1, 1, 5, 3), (2, 2, 3, 3), (3, 2, 16, 16), (5, 4, 17, 9), (7, 5, 7, 5), (8, 8, 16, 16), (9, 7, 14, 10), (4, 4, 33, 31),
         (13, 11, 26, 22), (1, 9, 1, 18), (9, 1, 18, 1)]
SIZE_IDS = ["%dx%d-%dx%d" % s for s in SIZES]
COMMON = ["random", "constant", "zero", "one", "step", "checker", "bright", "ramp"]
F32_ONLY = ["above1", "negative", "nan", "inf"]
SHARPNESS = 0.2


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    """bit-equal, a NaN for a NaN (a host and a device NaN may differ in sign and payload, as in tests/test_math.py)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.uint8:
        return bool(np.array_equal(a, b))
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def assert_same(got, want, what):
    if same(got, want):
        return
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: shape / type %s %s, restatement %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want if got.dtype == np.uint8 else ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    first = tuple(np.argwhere(bad)[0][:2])
    raise AssertionError("%s: differs in %d pixels, first at (y, x) = %s: %s, restatement %s" % (what, int(bad.any(-1).sum()), first, got[first], want[first]))


@functools.lru_cache(maxsize=None)
def pattern(name, w, h, f32):
    """An (h, w, 4) test frame: float32 for the RGBA32F surface, uint8 for R8G8B8A8_UNORM."""
    rng = np.random.default_rng(1000 * w + h + 7 * len(name))
    ys, xs = np.mgrid[0:h, 0:w]
    rgb = np.zeros((h, w, 3))
    if name in ("random", "nan", "inf"):
        rgb = rng.random((h, w, 3))
    elif name == "constant":
        rgb[:] = 0.37
    elif name == "one":
        rgb[:] = 1.0
    elif name == "step":
        rgb[:] = (xs >= (w + 1) // 2)[..., None]
    elif name == "checker":
        rgb[:] = ((xs + ys) & 1)[..., None]
    elif name == "bright":
        rgb[h // 2, w // 2] = 1.0
    elif name == "ramp":
        rgb[:] = (xs / max(w - 1, 1))[..., None] * np.array([1.0, 0.5, 0.25])
    elif name == "above1":
        rgb = rng.random((h, w, 3)) * 6.0
    elif name == "negative":
        rgb = rng.random((h, w, 3)) * 2.0 - 1.0
    if not f32:
        out = np.full((h, w, 4), 255, np.uint8)
        out[..., :3] = (rgb * 255.0 + 0.5).astype(np.uint8)
    else:
        out = np.ones((h, w, 4), F32)
        out[..., :3] = rgb
        if name == "nan":
            out[h // 2, w // 3, 1] = np.nan
        if name == "inf":
            out[h // 3, w // 2, 0] = np.inf
    out.setflags(write=False)
    return out


def names(f32):
    return COMMON + (F32_ONLY if f32 else [])


def texels(img):
    return ref.load_unorm8(img) if img.dtype == np.uint8 else img[..., :3]


@functools.lru_cache(maxsize=None)
def easu_case(name, size, f32):
    """(input surface, the restatement's EASU output surface, its intermediates) -- computed once, shared by the CPU and the GPU tests"""
    w, h, ow, oh = size
    img = pattern(name, w, h, f32)
    out, mid = ref.easu(texels(img), ow, oh, ref.easu_constants(w, h, ow, oh))
    surface = ref.store_f32(out) if f32 else ref.store_unorm8(out)
    surface.setflags(write=False)
    return img, surface, mid, out


@functools.lru_cache(maxsize=None)
def rcas_bits(sharpness=SHARPNESS):
    from tracerboy_amd import api
    return int(api.FsrConstants(1, 1, 1, 1, sharpness).rcas[0])


@functools.lru_cache(maxsize=None)
def rcas_case(name, size, f32, raw, sharpness=SHARPNESS):
    """RCAS at the size pair's output size: on the EASU result of the pattern, or (raw) on the pattern generated at that size"""
    img = pattern(name, size[2], size[3], f32) if raw else easu_case(name, size, f32)[1]
    out, mid = ref.rcas(texels(img), rcas_bits(sharpness))
    surface = ref.store_f32(out) if f32 else ref.store_unorm8(out)
    return img, surface, mid


# ---- CPU: constants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [(960, 540, 1920, 1080), (1920, 1080, 3840, 2160), (48, 32, 61, 45)])
def test_easu_constants_are_bit_equal(built, size):
    """each word is one fp32 quotient and at most two products and a difference: the library and the restatement must agree in every bit"""
    from tracerboy_amd import api
    k = api.FsrConstants(*size, SHARPNESS)
    assert np.array_equal(np.array(list(k.easu), np.uint32), ref.easu_constants(*size))


@pytest.mark.parametrize("stops", [0.0, 0.2, 1.0, 2.0])
def test_rcas_constant_is_exp2_of_minus_the_stops(built, stops):
    from tracerboy_amd import api
    k = api.FsrConstants(8, 8, 16, 16, stops)
    got = np.array([k.rcas[0]], np.uint32).view(F32)[0]
    want = 2.0 ** -stops
    print("stops %g: %.9g, 2^-s %.9g, ulp %.3g" % (stops, float(got), want, float(np.spacing(F32(want)))))
    assert abs(float(got) - want) <= float(np.spacing(F32(want)))
    assert k.rcas[1] == ref.half_truncated(got) * 0x10001 and k.rcas[2] == 0 and k.rcas[3] == 0


def test_constants_refuse_zero_sizes_and_sharpness_that_is_not_finite(built):
    from tracerboy_amd import api
    for args in ((0, 1, 1, 1, 0.2), (1, 0, 1, 1, 0.2), (1, 1, 0, 1, 0.2), (1, 1, 1, 0, 0.2), (1, 1, 1, 1, float("nan")), (1, 1, 1, 1, float("inf"))):
        with pytest.raises(api.TracerBoyError) as refused:
            api.FsrConstants(*args)
        assert refused.value.code == TB_E_INVALID
    assert api.lib().tb_fsr_constants(1, 1, 1, 1, 0.2, None) == TB_E_INVALID


# ---- CPU: properties of the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_easu_of_a_constant_image_is_that_constant(size):
    """dir = 0, so zro; whatever aC / aW rounds to, min(max4, max(min4, .)) with min4 = max4 = c is c (and c too where the quotient is NaN)"""
    w, h, ow, oh = size
    for c in (0.0, 1.0, 0.37, 1.0 / 255.0, 1e-3, 123.5, -2.25):
        img = np.full((h, w, 3), c, F32)
        out, _ = ref.easu(img, ow, oh, ref.easu_constants(w, h, ow, oh))
        assert out.shape == (oh, ow, 3) and np.all(bits(out) == bits(F32(c))), c


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_easu_stays_within_the_four_nearest_texels(size):
    for f32 in (False, True):
        for name in ("random", "checker", "bright", "ramp", "step") + (("above1", "negative") if f32 else ()):
            _, _, mid, out = easu_case(name, size, f32)
            assert np.all(out >= mid["lo"]) and np.all(out <= mid["hi"]), name


def test_easu_of_a_vertical_step_is_monotone_across_it():
    for (w, h) in ((8, 6), (13, 5), (4, 4)):
        img = np.zeros((h, w, 3), F32); img[:, w // 2:] = 1.0
        out, _ = ref.easu(img, 2 * w, 2 * h, ref.easu_constants(w, h, 2 * w, 2 * h))
        assert np.all(np.diff(out, axis=1) >= 0), (w, h)
        assert np.all(out[:, 0] == 0) and np.all(out[:, -1] == 1)


def test_rcas_lobe_is_limited_for_taps_in_the_unit_range(built):
    for size in SIZES:
        for name in COMMON:
            for raw in (False, True):
                _, _, mid = rcas_case(name, size, False, raw)
                lobe, con = mid["lobe"], float(mid["con"])
                assert not np.isnan(lobe).any()
                assert np.all(lobe <= 0) and np.all(lobe >= F32(-0.1875) * F32(con)), (size, name, raw)


# ---- CPU: the GPU cases reach what they are meant to reach ---------------------------------------------------------------------------------
def test_easu_cases_reach_every_branch():
    zro_true = zro_false = cut = left = right = top = bottom = False
    for size in SIZES:
        w, h = size[:2]
        for f32 in (False, True):
            for name in names(f32):
                mid = easu_case(name, size, f32)[2]
                zro_true |= bool(mid["zro"].any()); zro_false |= bool((~mid["zro"]).any()); cut |= bool(mid["cut"].any())
                left |= bool((mid["fx"] - 1 < 0).any()); right |= bool((mid["fx"] + 2 > w - 1).any())
                top |= bool((mid["fy"] - 1 < 0).any()); bottom |= bool((mid["fy"] + 2 > h - 1).any())
    assert zro_true and zro_false, "zro is %s for every pixel" % zro_true
    assert cut, "d2 never reaches the clipping point"
    assert left and right and top and bottom, (left, right, top, bottom)
    # and in one frame that is larger than the tap window: inner pixels clamp nothing, border pixels do
    mid = easu_case("random", (13, 11, 26, 22), True)[2]
    inner = (mid["fx"] - 1 >= 0) & (mid["fx"] + 2 <= 12) & (mid["fy"] - 1 >= 0) & (mid["fy"] + 2 <= 10)
    assert inner.any() and (~inner).any()


def test_rcas_cases_reach_every_branch(built):
    nan_min = nan_max = low = high = outside = False
    for size in SIZES:
        for f32 in (False, True):
            for name in names(f32):
                for raw in (False, True):
                    mid = rcas_case(name, size, f32, raw)[2]
                    if name == "zero":
                        assert mid["nan_min"].all(), "a black ring must give hitMin = 0 * (1 / 0) = NaN"
                        nan_min = True
                    if name == "one" and raw:
                        inner = ~mid["outside"]
                        assert mid["nan_max"][inner].all(), "a white ring must give hitMax = 0 * (1 / 0) = NaN"
                        nan_max |= bool(inner.any())
                    with np.errstate(invalid="ignore"):
                        low |= bool((mid["widest"] < F32(-0.1875)).any()); high |= bool((mid["widest"] > 0).any())
                    outside |= bool(mid["outside"].any())
    assert nan_min and nan_max and low and high and outside, (nan_min, nan_max, low, high, outside)


# ---- CPU: ABI and command line ------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_symbols(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    assert C.sizeof(abi.TbFsrConstants) == 80
    assert abi.TbFsrConstants.easu.offset == 0 and abi.TbFsrConstants.rcas.offset == 64
    L = api.lib()
    for symbol in ("tb_fsr_constants", "tb_run_fsr_easu", "tb_run_fsr_rcas", "tb_upscale"):
        assert getattr(L, symbol) is not None and symbol in L._tb_exports


def run_cli(*args):
    """with a scene that does not exist: status 2 can only come from the argument checks, which stand before the first device call"""
    return subprocess.run([CLI, os.path.join(ROOT, "tests", "no-such-scene.pbrt")] + list(args), capture_output=True, text=True, timeout=60)


def test_cli_refuses_bad_upscale_arguments_before_any_device_call(built):
    r = run_cli("--upscale", "64x64", "--render-scale", "0.5")
    assert r.returncode == 2 and "--upscale and --render-scale" in r.stderr, r
    for bad in ("64", "64x", "x64", "0x16", "16x0", "64x64x2", "axb", "64 x 64", "-4x4", "8192x8192"):
        r = run_cli("--upscale", bad)
        assert r.returncode == 2 and "--upscale is WxH" in r.stderr, (bad, r)
    for bad in ("0", "-0.5", "1.5", "nan", "half", "0.5x"):
        r = run_cli("--render-scale", bad)
        assert r.returncode == 2 and "--render-scale is above 0 and at most 1" in r.stderr, (bad, r)
    r = run_cli("--fsr-sharpness", "0.5")
    assert r.returncode == 2 and "--fsr-sharpness needs" in r.stderr, r
    r = run_cli("--upscale", "8x8", "--fsr-sharpness", "inf")
    assert r.returncode == 2 and "--fsr-sharpness is" in r.stderr, r
    assert "--upscale WxH" in subprocess.run([CLI], capture_output=True, text=True, timeout=60).stderr   # the usage text


# ---- GPU: the two kernels through the seam ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["unorm8", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_gpu_easu_is_bit_exact(gpu_tb, size, f32):
    from tracerboy_amd import api
    w, h, ow, oh = size
    k = api.FsrConstants(w, h, ow, oh, SHARPNESS)
    for name in names(f32):
        img, want, _, _ = easu_case(name, size, f32)
        assert_same(gpu_tb.RunFsrEasu(k, img, ow, oh), want, "EASU %s %s" % (SIZE_IDS[SIZES.index(size)], name))


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["unorm8", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_gpu_rcas_is_bit_exact(gpu_tb, size, f32):
    from tracerboy_amd import api
    ow, oh = size[2:]
    k = api.FsrConstants(ow, oh, ow, oh, SHARPNESS)
    for name in names(f32):
        for raw in (False, True):
            img, want, _ = rcas_case(name, size, f32, raw)
            assert_same(gpu_tb.RunFsrRcas(k, img), want, "RCAS %dx%d %s%s" % (ow, oh, name, " (raw)" if raw else " (EASU result)"))
    sharpest = api.FsrConstants(ow, oh, ow, oh, 0.0)      # con = 1: the widest lobe
    img, want, _ = rcas_case("random", size, f32, True, 0.0)
    assert_same(gpu_tb.RunFsrRcas(sharpest, img), want, "RCAS %dx%d random at 0 stops" % (ow, oh))


# ---- GPU: the stage ---------------------------------------------------------------------------------------------------------------------
def expect_upscale(post_f, post_b, ow, oh, sharpness=SHARPNESS):
    from tracerboy_amd import api
    h, w = post_f.shape[:2]
    k = api.FsrConstants(w, h, ow, oh, sharpness)
    return ref.upscale(post_f, ow, oh, k), ref.upscale(post_b, ow, oh, k)


@pytest.fixture(scope="module")
def s3(built, settings):
    s = copy.copy(settings); s.MaxBounces = 3; s.EnableBlueNoise = 0
    return s


@pytest.mark.gpu
def test_gpu_upscale_after_a_render_and_nothing_else_changes(gpu_tb, s3):
    from tracerboy_amd import api
    before = gpu_tb.GetOption("debug_live_device_bytes")
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(48, 32, 8, s3, 0.0)
        uninterrupted = tb.AccumDigest()
        tb.InvalidateHistory()
        tb.Render(48, 32, 4, s3, 0.0)
        digest, frames = tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()
        post_f, post_b = tb.PostProcess()
        held = gpu_tb.GetOption("debug_live_device_bytes")
        for (ow, oh) in ((96, 64), (61, 45)):
            got_f, got_b = tb.Upscale(ow, oh)
            want_f, want_b = expect_upscale(post_f, post_b, ow, oh)
            assert_same(got_b, want_b, "tb_upscale %dx%d, R8G8B8A8_UNORM" % (ow, oh))
            assert_same(got_f, want_f, "tb_upscale %dx%d, RGBA32F" % (ow, oh))
            assert np.all(got_b[..., 3] == 255) and np.all(got_f[..., 3] == 1.0)
            assert tb.GetOption("last_easu_us") > 0 and tb.GetOption("last_rcas_us") > 0
            assert tb.GetOption("last_upscale_us") >= max(tb.GetOption("last_easu_us"), tb.GetOption("last_rcas_us"))
            only_f, none = tb.Upscale(ow, oh, rgba8=False)     # the RGBA32F chain alone
            assert none is None
            assert_same(only_f, want_f, "tb_upscale %dx%d, RGBA32F alone" % (ow, oh))
        # its scratch surfaces are the context's and are counted: two surfaces per chain at the last output size
        assert gpu_tb.GetOption("debug_live_device_bytes") == held + 2 * 61 * 45 * (4 + 16)
        sharp_f, sharp_b = tb.Upscale(61, 45, sharpness=0.0)
        want_f, want_b = expect_upscale(post_f, post_b, 61, 45, 0.0)
        assert_same(sharp_b, want_b, "0 stops, R8G8B8A8_UNORM"); assert_same(sharp_f, want_f, "0 stops, RGBA32F")
        assert not same(sharp_f, got_f), "the sharpness has no effect"
        assert tb.AccumDigest() == digest and tb.GetNumberOfSamplesSinceLastInvalidate() == frames
        tb.Render(48, 32, 4, s3, 0.0)
        assert tb.AccumDigest() == uninterrupted, "frames rendered after an upscale are not those of the uninterrupted render"
    assert gpu_tb.GetOption("debug_live_device_bytes") == before


@pytest.mark.gpu
def test_gpu_upscale_after_a_real_time_frame(built, s3):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.RenderRealTime(40, 24, s3, None, 0.0)
        post_f, post_b = tb.PostProcess(outputType=0)
        got_f, got_b = tb.Upscale(80, 48)
        want_f, want_b = expect_upscale(post_f, post_b, 80, 48)
        assert_same(got_b, want_b, "after tb_render_realtime, R8G8B8A8_UNORM")
        assert_same(got_f, want_f, "after tb_render_realtime, RGBA32F")


@pytest.mark.gpu
def test_gpu_upscale_reads_the_denoised_picture(built, s3):
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.SetOption("aov", 1)
        tb.LoadScene(CORNELL)
        tb.Render(48, 32, 4, s3, 0.0)
        plain_f, plain_b = tb.Upscale(96, 64)
        tb.Denoise(read=False)
        tb.SetOption("post_denoised", 1)
        post_f, post_b = tb.PostProcess()
        got_f, got_b = tb.Upscale(96, 64)
        want_f, want_b = expect_upscale(post_f, post_b, 96, 64)
        assert_same(got_b, want_b, "post_denoised, R8G8B8A8_UNORM")
        assert_same(got_f, want_f, "post_denoised, RGBA32F")
        assert not same(got_f, plain_f) and not same(got_b, plain_b), "the upscale did not read the denoised picture"


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_leave_the_context_usable(built, s3):
    from tracerboy_amd import _ctypes_abi as abi, api
    with api.TracerBoy(0) as tb:
        L, ctx = tb._L, tb._ctx
        ps = api.GetDefaultPostProcessSettings()
        f = np.empty((64, 96, 4), F32); b = np.empty((64, 96, 4), np.uint8)
        pf, pb = f.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)

        def refused(rc, word):
            message = L.tb_last_error(ctx).decode()
            assert rc == TB_E_INVALID and word in message, (rc, message)

        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 64, -1.0, pf, pb), "nothing rendered")        # what tb_post_process refuses
        tb.LoadScene(CORNELL)
        tb.Render(48, 32, 2, s3, 0.0)
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 64, -1.0, None, None), "null")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 0, 64, -1.0, pf, pb), "dimension is 0")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 0, -1.0, pf, pb), "dimension is 0")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 47, 64, -1.0, pf, pb), "only upscales")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 31, -1.0, pf, pb), "only upscales")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 4097, 4096, -1.0, pf, pb), "2^24")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 64, float("nan"), pf, pb), "not finite")
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 64, float("inf"), pf, pb), "not finite")
        tb.SetOption("post_denoised", 1)
        refused(L.tb_upscale(ctx, C.byref(ps), 0, 96, 64, -1.0, pf, pb), "post_denoised")          # tb_post_process's own refusal
        tb.SetOption("post_denoised", 0)
        k = api.FsrConstants(4, 4, 8, 8, SHARPNESS)
        i8 = np.zeros((4, 4, 4), np.uint8); o8 = np.zeros((8, 8, 4), np.uint8)
        pi, po = i8.ctypes.data_as(C.c_void_p), o8.ctypes.data_as(C.c_void_p)
        refused(L.tb_run_fsr_easu(ctx, None, 0, 4, 4, 8, 8, pi, po), "null")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 0, 4, 4, 8, 8, None, po), "null")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 0, 4, 4, 8, 8, pi, None), "null")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 2, 4, 4, 8, 8, pi, po), "surface type")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 0, 0, 4, 8, 8, pi, po), "dimension is 0")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 0, 4, 4, 8, 0, pi, po), "dimension is 0")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 0, 4, 4, 3, 8, pi, po), "only upscales")
        refused(L.tb_run_fsr_easu(ctx, C.byref(k), 0, 4, 4, 4097, 4096, pi, po), "2^24")
        refused(L.tb_run_fsr_rcas(ctx, None, 0, 8, 8, po, po), "null")
        refused(L.tb_run_fsr_rcas(ctx, C.byref(k), 0, 8, 8, None, po), "null")
        refused(L.tb_run_fsr_rcas(ctx, C.byref(k), 7, 8, 8, po, po), "surface type")
        refused(L.tb_run_fsr_rcas(ctx, C.byref(k), 1, 0, 8, po, po), "dimension is 0")
        refused(L.tb_run_fsr_rcas(ctx, C.byref(k), 1, 4097, 4096, po, po), "2^24")
        # and the context still works
        post_f, post_b = tb.PostProcess()
        got_f, got_b = tb.Upscale(96, 64)
        want_f, want_b = expect_upscale(post_f, post_b, 96, 64)
        assert_same(got_b, want_b, "after the refusals, R8G8B8A8_UNORM"); assert_same(got_f, want_f, "after the refusals, RGBA32F")
        assert_same(tb.RunFsrEasu(k, pattern("random", 4, 4, False), 8, 8), easu_case("random", (4, 4, 8, 8), False)[1], "after the refusals, the seam")
