"""The short forms of the six-wave copy's shading arithmetic (PT_SHADING_SHORT_FORMS, pt_variant_matte6.hip; include/tb_math.h: tb_sincos, tb_div_pi,
tb_zero_over_sqrt; docs/experiments/r12.md): the same bits in fewer instructions.

CPU: tests/shading/short_forms_driver.cpp, a host program, compares each short form with the form it stands for, as bits -- all 2^32 numerators for
the division by PI (and prints where the three operations alone are right: the header's interval must be that), every denominator class for the zero
component of reorient, every 251st value for tb_sincos; a second build of it under ASan + UBSan runs a strided sweep and the edge values.
CPU, compile-only: the listing of the unit under the build's own flags against the counts of the commit before.
GPU: cornell-box through the six-wave copy against the oracle, bit for bit, and the device's evaluation of the new functions against the host's."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "shading", "_build")

# where tb_div_pi takes the three operations: +0 and this interval of magnitudes (the sweep's longest run that is right for both signs)
FAST_INTERVAL = ("0x0b1ec7a1", "0x7f7fffff")

# the listing of the commit before, per kernel of the unit (the three are alike): 13 rand() and the azimuth's sine and cosine reduce an argument each;
# 54 IEEE divisions, three of them reorient's (the compiler had merged its two branches: one 0 / s per lane, not two)
RNDNE_F64_BEFORE = 15
DIV_FIXUP_BEFORE = 54
SCRATCH_BYTES_BEFORE = 80
VGPRS = 80
RCP_PI_LITERAL = "0x3ea2f983"


# ---- the host program ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "shading"), "OUT=" + BUILD], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(BUILD, "short_forms_driver"), os.path.join(BUILD, "short_forms_driver_san")


def _answers(program, mode, limit):
    p = subprocess.run([program, mode], capture_output=True, text=True, timeout=limit)
    print(p.stdout)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-3000:] + p.stderr)[-4000:]
    return dict((w[0], w[1:]) for w in (line.split() for line in p.stdout.splitlines()))


def _assert_no_difference(a):
    assert a["ok"] == ["1"]
    for name in ("sincos_differ", "div_pi_differ", "fast_path_differs_where_taken", "zero_over_sqrt_differ"):
        assert a[name] == ["0"], (name, a[name])
    assert all(int(n) > 0 for n in a["sqrt_classes_zero_denormal_normal_inf_nan"])     # +0, denormal, normal, +inf, NaN were all denominators
    assert tuple(a["header_interval"]) == FAST_INTERVAL


def test_every_numerator_and_every_denominator_class_on_the_host(drivers):
    a = _answers(drivers[0], "full", 900)
    _assert_no_difference(a)
    assert int(a["div_pi_compared"][0]) >= 2 ** 32 and int(a["zero_over_sqrt_compared"][0]) >= 2 ** 31 and int(a["sincos_compared"][0]) >= 2 ** 24
    # the domain of the three operations as the sweep finds it: the header's interval is its longest run, +0 is right and -0 is not
    assert tuple(a["fast_path_longest_run"][:2]) == FAST_INTERVAL
    assert a["fast_path_plus_zero"] == ["1"] and a["fast_path_minus_zero"] == ["0"]


def test_strided_sweep_and_edge_values_under_sanitizers(drivers):
    a = _answers(drivers[1], "strided", 300)
    _assert_no_difference(a)
    assert int(a["div_pi_compared"][0]) >= 2 ** 20


# ---- the listing --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """the text of each of the unit's three kernels"""
    from tracerboy_amd import build as b
    out = str(tmp_path_factory.mktemp("isa") / "matte6.s")
    src = "kernels/pt_variant_matte6.hip"
    cmd = [b.HIPCC] + b.COMMON + list(b.device_flags(src)) + ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, src)]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    bodies = [text[m.start():text.index(".end_amdhsa_kernel", m.start())] for m in re.finditer(r"^_ZN\S*pt_persistent\S*:.*$", text, re.M)]
    assert len(bodies) == 3
    return text, bodies


def test_one_reduction_and_one_division_fewer_per_kernel(kernels):
    text, bodies = kernels
    for body in bodies:
        rndne, fixup = len(re.findall(r"\bv_rndne_f64", body)), len(re.findall(r"\bv_div_fixup_f32", body))
        by_rcp_pi = len(re.findall(r"\bv_mul_f32\w*\s.*%s" % RCP_PI_LITERAL, body))
        print("v_rndne_f64", rndne, "v_div_fixup_f32", fixup, "products with the reciprocal of PI", by_rcp_pi)
        assert rndne == RNDNE_F64_BEFORE - 1            # the azimuth's second reduction
        assert fixup == DIV_FIXUP_BEFORE - 1            # reorient's 0 / s; the three divisions by PI stay for the numerators outside the interval
        assert by_rcp_pi == 3                           # diffuse_brdf twice, diffusePdf


def test_scratch_and_registers_are_what_they_were(kernels):
    text, _ = kernels
    scratch = [int(x) for x in re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", text, re.M)]
    vgprs = [int(x) for x in re.findall(r"^\s*\.vgpr_count:\s*(\d+)", text, re.M)]
    print("scratch bytes", scratch, "VGPRs", vgprs)
    assert len(scratch) == 3 and max(scratch) <= SCRATCH_BYTES_BEFORE and vgprs == [VGPRS] * 3


def test_only_the_six_wave_unit_compiles_the_short_forms():
    kernels = os.path.join(ROOT, "tracerboy_amd", "csrc", "kernels")
    defining = sorted(f for f in os.listdir(kernels) if re.search(r"^\s*#\s*define\s+PT_SHADING_SHORT_FORMS\b", open(os.path.join(kernels, f)).read(), re.M))
    assert defining == ["pt_variant_matte6.hip"], defining


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}
_LOADED = {}
CASES = [(40, 24, 4), (64, 48, 8)]      # no multiple of 16, lanes without a sample; whole regions, eight frames (docs/experiments/r10.md)
PARK_MINS = [1, 2, 64]
BOUNCES = 8


@pytest.fixture(scope="module")
def tb(built):
    """a context of this module's own: park_min is read when a scene is loaded"""
    from tracerboy_amd import api
    ctx = api.TracerBoy(0)
    yield ctx
    ctx.close()
    _LOADED.clear()


def _settings():
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings()
    s.EnableBlueNoise = 0
    s.MaxBounces = BOUNCES
    return s


def _oracle(tb, W, H, F, s):
    """the CPU oracle's surfaces, once per size"""
    import oracle_lib as ol
    if (W, H, F) not in _ORACLE:
        _ORACLE[(W, H, F)] = ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, s, 0.0), W, H, F, threads=8, jittered=True)
    return _ORACLE[(W, H, F)]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["plain", "shrinking"])
@pytest.mark.parametrize("W,H,F", CASES)
@pytest.mark.parametrize("park_min", PARK_MINS)
def test_six_wave_copy_is_bit_equal_to_the_oracle(tb, park_min, W, H, F, kernel):
    s = _settings()
    if _LOADED.get("now") != park_min:
        tb.SetOption("park_min", park_min)
        tb.LoadScene(CORNELL)
        _LOADED["now"] = park_min
    tb.InvalidateHistory()
    tb.Render(W, H, F, s, 0.0, sync=kernel != "plain")
    tb.Sync()
    assert tb.GetOption("last_copy_waves") == 6 and tb.GetOption("last_pipeline") == 0
    assert tb.GetOption("last_plan_guided_groups") == (1 if kernel == "shrinking" else 0)
    out, jit = tb.ReadAccumulation(jittered=True)
    ref = _oracle(tb, W, H, F, s)
    diff = int((out.view(np.uint32) != ref["output"].view(np.uint32)).any(axis=-1).sum())
    print(park_min, W, H, F, kernel, "pixels that differ from the oracle:", diff)
    assert np.array_equal(out.view(np.uint32), ref["output"].view(np.uint32)), diff
    assert np.array_equal(jit.view(np.uint32), ref["jittered"].view(np.uint32))


# function codes of tb_device_math, appended to those of tests/test_math.py
SIN, COS, DIV = 0, 1, 11
SINCOS_SIN, SINCOS_COS, DIV_PI, ZERO_OVER_SQRT = 19, 20, 21, 22
N = 1 << 20


def _same(dev, host):
    return (dev.view(np.uint32) == host.view(np.uint32)) | (np.isnan(dev) & np.isnan(host))


@pytest.mark.gpu
def test_device_evaluates_the_short_forms_to_the_host_bits(gpu_tb):
    """one call per function on 2^20 values, the edge classes among them.  The host's bits: the oracle library's tb_sin / tb_cos, and numpy's
    binary32 division, which the host program above has shown to be tb_div_pi's and tb_zero_over_sqrt's for every operand"""
    import oracle_lib as ol
    rng = np.random.default_rng(20262)
    pi = np.float32(3.1415926535)
    lo, hi = (np.array([int(b, 16)], np.uint32).view(np.float32)[0] for b in FAST_INTERVAL)
    edge = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, -1e-38, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1e9, 2.5e9,
                     999999936.0, 6.2831855, 3.1415927, lo, -lo, np.nextafter(lo, np.float32(0)), -np.nextafter(lo, np.float32(0)), hi, -hi], np.float32)
    any_bits = rng.integers(0, 1 << 32, N - len(edge) - (N // 4) * 2, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near_lo = (np.uint32(int(FAST_INTERVAL[0], 16)) + rng.integers(-(1 << 22), 1 << 22, N // 4)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        # the division: every bit pattern alike, a quarter around the lower end of the interval, a quarter the cosines the kernel divides
        a = np.concatenate([any_bits, near_lo * rng.choice(np.float32([-1, 1]), N // 4), rng.uniform(-1, 1, N // 4).astype(np.float32), edge])
        assert a.size == N
        dev = gpu_tb.DeviceMath(DIV_PI, a)
        host = a / pi
        same = _same(dev, host)
        assert same.all(), (a[~same][:4], dev[~same][:4], host[~same][:4])
        # both values of one reduction: the azimuths (2 pi rand), the RNG's range, every bit pattern
        x = np.concatenate([any_bits, rng.uniform(0, 6.2831855, N // 4).astype(np.float32), rng.uniform(-5000, 5000, N // 4).astype(np.float32), edge])
        for fn, ref in ((SINCOS_SIN, SIN), (SINCOS_COS, COS)):
            dev, host = gpu_tb.DeviceMath(fn, x), ol.math_fn(ref, x)
            same = _same(dev, host)
            assert same.all(), (fn, x[~same][:4], dev[~same][:4], host[~same][:4])
        # 0 / s for square roots: +0, normal, +inf, NaN, and denormal denominators as they are
        sq = np.abs(a)
        s = np.concatenate([np.sqrt(sq[:N // 2]), np.sqrt(np.abs(edge)), np.abs(near_lo[:N // 4]), rng.integers(0, 1 << 23, N // 4).astype(np.uint32).view(np.float32)])
        s = s[~(np.isnan(s) & ((s.view(np.uint32) & np.uint32(0x00400000)) == 0))]        # no operation returns a signalling NaN
        dev = gpu_tb.DeviceMath(ZERO_OVER_SQRT, s)
        host = np.float32(0) / s
        assert np.array_equal(dev.view(np.uint32)[~np.isnan(host)], host.view(np.uint32)[~np.isnan(host)]) and np.array_equal(np.isnan(dev), np.isnan(host))
        assert (s == 0).any() and np.isinf(s).any() and np.isnan(s).any() and ((s > 0) & (s < 1.17549435e-38)).any()
        # and against the device's own divisions, NaNs included: what the kernel computed before is what it computes now
        assert np.array_equal(dev.view(np.uint32), gpu_tb.DeviceMath(DIV, np.zeros_like(s), s).view(np.uint32))
        assert np.array_equal(gpu_tb.DeviceMath(DIV_PI, a).view(np.uint32), gpu_tb.DeviceMath(DIV, a, np.full_like(a, pi)).view(np.uint32))
