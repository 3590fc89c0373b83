"""Light probes (include/tracerboy_hip.h tb_bake_probes .. tb_run_probe_project): SH9 records baked around the two queries
and sampled, on the device.  The expected values are tests/probe_cases.py's numpy restatement of kernels/probe_launch.h, TraceRadiance and TraceRays
(which their own tests hold to the oracle) and closed forms; every comparison is on bits unless it says otherwise."""
import copy
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, CORNELL

gpu = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24                                                        # half an ulp of 1: the relative error of one rounded binary32 operation
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
DYNAMIC_TRI3 = os.path.join(os.path.dirname(os.path.dirname(CORNELL)), "dynamic", "tri3.pbrt")


def same_bytes(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same(a, b):
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def test_header_exports_bindings_and_methods_agree(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    h, a = _header("tracerboy_hip.h"), _header("tb_abi.h")
    W = r"\s*\w+\s*"
    assert re.search(r"\bint\s+tb_bake_probes\s*\(\s*tb_context\s*\*" + W + r",\s*const\s+tb_output_settings\s*\*" + W + r",\s*float" + W +
                     r",\s*const\s+tb_probe_call\s*\*" + W + r",\s*const\s+float\s*\*" + W + r",\s*TbProbe\s*\*" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_probes_refusal\s*\(\s*const\s+tb_probe_call\s*\*" + W + r",(\s*const\s+void\s*\*" + W + r",){2}\s*char\s*\*" + W + r",\s*uint32_t" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_read_probe_maps\s*\(\s*tb_context\s*\*" + W + r",\s*float\s*\*" + W + r",\s*TbQueryHit\s*\*" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_sample_probes\s*\(\s*tb_context\s*\*" + W + r",\s*uint32_t" + W + r",\s*const\s+tb_probe_grid\s*\*" + W + r",\s*uint32_t" + W +
                     r",\s*float" + W + r",\s*const\s+TbProbe\s*\*" + W + r",\s*uint64_t" + W + r",(\s*const\s+float\s*\*" + W + r",){2}\s*float\s*\*" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_sh9_irradiance\s*\(\s*const\s+TbProbe\s*\*" + W + r",\s*const\s+float\s*\*" + W + r",\s*float\s*\*" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_probe_directions\s*\(\s*uint32_t" + W + r",(\s*float\s*\*" + W + r",)\s*float\s*\*" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_run_probe_rays\s*\(\s*tb_context\s*\*" + W + r",(\s*uint32_t" + W + r",){3}\s*const\s+float\s*\*" + W + r",\s*TbRadianceRay\s*\*" + W +
                     r",\s*TbQueryRay\s*\*" + W + r"\)", h)
    assert re.search(r"\bint\s+tb_run_probe_project\s*\(\s*tb_context\s*\*" + W + r",(\s*uint32_t" + W + r",){2}(\s*const\s+float\s*\*" + W + r",){2}\s*const\s+TbQueryHit\s*\*" + W +
                     r",\s*TbProbe\s*\*" + W + r"\)", h)
    for name, value in (("TB_PROBES_DEVICE", "0x100u"), ("TB_PROBES_ACCUMULATE", "0x200u"), ("TB_PROBES_KEEP_MAPS", "0x400u"), ("TB_RAYS_DEVICE", "0x100u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), h), name
    assert (api.PROBES_DEVICE, api.PROBES_ACCUMULATE, api.PROBES_KEEP_MAPS) == (0x100, 0x200, 0x400)
    call = re.search(r"typedef\s+struct\s+tb_probe_call\s*\{\s*uint32_t\s+([\w\s,]+);\s*\}\s*tb_probe_call\s*;", h).group(1)
    assert [n.strip() for n in call.split(",")] == [n for n, _ in abi.tb_probe_call._fields_] == ["n", "first_probe_number", "resolution", "first_sample", "num_samples", "flags"]
    assert re.search(r"typedef\s+struct\s+TbProbe\s*\{\s*float\s+SH\s*\[\s*27\s*\]\s*;\s*float\s+Weight\s*,\s*Hits\s*,\s*Backfaces\s*,\s*MinDistance\s*,\s*MeanDistance\s*;\s*\}\s*TbProbe\s*;", a)
    assert re.search(r"typedef\s+struct\s+tb_probe_grid\s*\{\s*float\s+origin\s*\[\s*3\s*\]\s*,\s*spacing\s*\[\s*3\s*\]\s*;\s*uint32_t\s+count\s*\[\s*3\s*\]\s*;\s*\}\s*tb_probe_grid\s*;", a)
    assert re.search(r"sizeof\s*\(\s*TbProbe\s*\)\s*==\s*128", a) and re.search(r"sizeof\s*\(\s*tb_probe_grid\s*\)\s*==\s*36", a)
    assert ctypes.sizeof(abi.TbProbe) == 128 == api.PROBE_DTYPE.itemsize and ctypes.sizeof(abi.tb_probe_grid) == 36 and ctypes.sizeof(abi.tb_probe_call) == 24
    assert {n: getattr(abi.TbProbe, n).offset for n, _ in abi.TbProbe._fields_} == {n: api.PROBE_DTYPE.fields[n][1] for n in api.PROBE_DTYPE.names} \
        == {"SH": 0, "Weight": 108, "Hits": 112, "Backfaces": 116, "MinDistance": 120, "MeanDistance": 124}
    assert api.PROBE_DTYPE["SH"].shape == (9, 3)
    raw = ctypes.CDLL(api.LIB_PATH); bound = api.lib()
    vp, u32, P = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER
    for name in ("tb_bake_probes", "tb_probes_refusal", "tb_read_probe_maps", "tb_sample_probes", "tb_sh9_irradiance", "tb_probe_directions", "tb_run_probe_rays",
                 "tb_run_probe_project"):
        assert hasattr(raw, name) and name in bound._tb_exports, name
    assert bound.tb_bake_probes.argtypes == [vp, P(abi.tb_output_settings), ctypes.c_float, P(abi.tb_probe_call), vp, vp]
    assert bound.tb_read_probe_maps.argtypes == [vp, vp, vp]
    assert bound.tb_sample_probes.argtypes == [vp, u32, P(abi.tb_probe_grid), u32, ctypes.c_float, vp, ctypes.c_uint64, vp, vp, vp]
    assert bound.tb_run_probe_rays.argtypes == [vp, u32, u32, u32, vp, vp, vp] and bound.tb_run_probe_project.argtypes == [vp, u32, u32, vp, vp, vp, vp]
    for m in ("BakeProbes", "ReadProbeMaps", "SampleProbes", "RunProbeRays", "RunProbeProject"):
        assert callable(getattr(api.TracerBoy, m)), m
    for f in ("ProbesRefusal", "sh9_irradiance", "probe_grid_positions", "probe_directions", "ProbeGrid"):
        assert callable(getattr(api, f)), f


def test_the_refusal_table(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    call = lambda n=5, first=0, res=8, fs=0, samples=1, flags=0: abi.tb_probe_call(n, first, res, fs, samples, flags)
    A = 0x10000                                                       # any aligned non-null address: the function compares, it does not read
    ALL = api.PROBES_DEVICE | api.PROBES_ACCUMULATE | api.PROBES_KEEP_MAPS
    assert api.ProbesRefusal(call(), A, A) is None
    assert api.ProbesRefusal(call(n=0), 0, 0) is None                 # no probes: no pointers needed
    assert api.ProbesRefusal(call(n=1 << 19, first=(1 << 24) - (1 << 19), res=64, fs=(1 << 32) - (1 << 24), samples=1 << 24, flags=ALL), A, A) is None
    assert api.ProbesRefusal(call(n=1 << 24, res=8), A, A) is None
    assert api.ProbesRefusal(call(res=2), A + 2, A + 4) is None       # host arrays need no alignment
    table = [
        (None, A, A, "null call"), (call(res=1), A, A, "resolution"), (call(res=0), A, A, "resolution"), (call(res=65), A, A, "resolution"),
        (call(n=(1 << 19) + 1, res=64), A, A, "2^31"), (call(n=(1 << 24) + 1, res=2), A, A, "2^24"), (call(n=2, first=(1 << 24) - 1), A, A, "2^24"),
        (call(samples=0), A, A, "num_samples"), (call(samples=(1 << 24) + 1), A, A, "2^24"), (call(fs=0xffffffff, samples=2), A, A, "2^32"),
        (call(flags=1), A, A, "flag"), (call(flags=0x800), A, A, "flag"), (call(flags=0x80000000), A, A, "flag"),
        (call(), 0, A, "null"), (call(), A, 0, "null"),
        (call(flags=api.PROBES_DEVICE), A + 2, A, "aligned"), (call(flags=api.PROBES_DEVICE), A, A + 8, "aligned"),
    ]
    for c, p, o, word in table:
        why = api.ProbesRefusal(c, p, o)
        assert why is not None and word in why, (word, why)


def test_wrong_inputs_are_refused_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    pos = np.zeros((5, 3), F32)
    for kw in (dict(resolution=1), dict(resolution=65), dict(resolution=8.0), dict(resolution=True), dict(samples=0), dict(samples=(1 << 24) + 1), dict(first_sample=-1),
               dict(first_sample=(1 << 32) - 1, samples=2), dict(first_number=-1), dict(first_number=(1 << 24) - 4), dict(keep_maps=1), dict(accumulate="yes"),
               dict(positions=np.zeros((5, 3), np.float64)), dict(positions=np.zeros((5, 4), F32)), dict(positions=np.zeros(15, F32)),
               dict(positions=np.zeros((10, 3), F32)[::2]), dict(positions=[[0.0, 0.0, 0.0]]), dict(positions=torch.zeros((5, 3), dtype=torch.float32)),
               dict(positions=torch.zeros((5, 3), dtype=torch.float64)), dict(positions=np.zeros(((1 << 19) + 1, 3), F32), resolution=64)):
        args = dict(positions=pos, resolution=8, samples=4); args.update(kw)
        with pytest.raises(ValueError):
            tb.BakeProbes(**args)
            pytest.fail(str(kw))
    grid = api.ProbeGrid((0, 0, 0), (1, 1, 1), (3, 2, 2))
    probes = np.zeros(12, api.PROBE_DTYPE); pts = np.zeros((7, 3), F32)
    for kw in (dict(grid=(0, 0, 0)), dict(probes=np.zeros(11, api.PROBE_DTYPE)), dict(probes=np.zeros((12, 31), F32)), dict(probes=np.zeros((12, 32), np.float64)),
               dict(points=np.zeros((7, 2), F32)), dict(normals=np.zeros((6, 3), F32)), dict(normals=torch.zeros((7, 3))), dict(points=np.zeros((14, 3), F32)[::2]),
               dict(resolution=1), dict(resolution=65), dict(backface_limit=float("nan")), dict(backface_limit=None), dict(backface_limit=True)):
        args = dict(grid=grid, probes=probes, points=pts, normals=pts); args.update(kw)
        with pytest.raises(ValueError):
            tb.SampleProbes(**args)
            pytest.fail(str(kw))
    for args in ((np.zeros((0, 3)), 8), (np.zeros((2, 2)), 8), (np.zeros((2, 3)), 1), (np.zeros((2, 3)), 65), (np.zeros(((1 << 12) + 1, 3)), 64)):
        with pytest.raises(ValueError):
            tb.RunProbeRays(*args)
    with pytest.raises(ValueError):
        tb.RunProbeProject(np.zeros((2, 3)), 8, np.zeros((2, 63, 4), F32), np.zeros((2, 64), api.QUERY_HIT_DTYPE))
    with pytest.raises(ValueError):
        tb.RunProbeProject(np.zeros((2, 3)), 8, np.zeros((2, 64, 4), F32), np.zeros((2, 64, 12), F32))
    for bad in (dict(origin=(0, 0), spacing=(1, 1, 1), count=(1, 1, 1)), dict(origin=(0, 0, 0), spacing=(1, 1, np.inf), count=(1, 1, 1)),
                dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(0, 1, 1)), dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(1 << 12, 1 << 12, 2)),
                dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2))):
        with pytest.raises(ValueError):
            api.ProbeGrid(**bad)
    with pytest.raises(AttributeError):                               # good arguments get past the checks, to the library this object lacks
        tb.BakeProbes(pos, 8, 4, first_sample=3, first_number=7, keep_maps=True)
    with pytest.raises(AttributeError):
        tb.SampleProbes(grid, probes, pts, pts, resolution=8, backface_limit=0.5)


@pytest.mark.parametrize("M", [2, 3, 8, 9, 16])
def test_the_directions_are_the_restatement(built, M):
    import probe_cases as pc
    from tracerboy_amd import api
    d, w = api.probe_directions(M)
    wd, ww, _ = pc.directions(M)
    assert same(d, wd) and same(w, ww) and d.shape == (M * M, 3)
    d64 = d.astype(np.float64)
    assert (np.abs((d64 * d64).sum(axis=1) - 1.0) <= 4 * U).all()       # three roundings of the quotients and the sqrt's: well inside 4 half-ulps
    assert (w > 0).all()
    with pytest.raises(ValueError):
        api.probe_directions(1)
    assert api.lib().tb_probe_directions(65, None, None) != 0 and api.lib().tb_probe_directions(8, None, None) == 0


def test_the_weights_converge_to_the_sphere():
    """The same formulas in float64: the solid angles sum to 4 pi with an error that falls strictly along M = 4, 8, 16, 32, 64 (1.5e-2, 5.1e-5,
    1.8e-6, 1.2e-7, 7.5e-9), and the nine basis functions are orthonormal under them to 2.4e-2 at 8, 7e-3 at 16, 4e-4 at 64."""
    import probe_cases as pc
    err = []
    for M in (4, 8, 16, 32, 64):
        _, w, _ = pc.directions(M, np.float64)
        err.append(abs(w.sum() / (4 * np.pi) - 1))
    print("sum w / 4 pi - 1:", err)
    assert all(b < a for a, b in zip(err, err[1:])) and err[0] < 2e-2 and err[-1] < 1e-8
    for M, bound in ((8, 2.5e-2), (16, 7.5e-3), (64, 4.5e-4)):
        d, w, _ = pc.directions(M, np.float64)
        Y = pc.basis(d)
        gram = (Y * w[:, None]).T @ Y
        print("Gram", M, np.abs(gram - np.eye(9)).max())
        assert np.abs(gram - np.eye(9)).max() <= bound


def test_the_irradiance_is_the_restatement_and_constant_light_gives_pi_l(built):
    import probe_cases as pc
    from tracerboy_amd import api
    rng = np.random.default_rng(25)
    sh = rng.normal(size=(40, 9, 3)).astype(F32)
    n = rng.normal(size=(40, 3)); n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    want = pc.irradiance(sh, n)
    for k in range(40):
        rec = np.zeros(1, api.PROBE_DTYPE); rec["SH"][0] = sh[k]
        assert same(api.sh9_irradiance(rec[0], n[k]), want[k]), k
    # Constant radiance L: SH[0] = 2 sqrt(pi) L, the rest 0, and E = pi L exactly (2 sqrt(pi) * Y0 = 1).  In binary32 the result carries the rounding of
    # SH[0] itself (1), of the constants A0 = pi and Y0 (1 each) and of the two products (A0 * s0) * Y0 (2); the sums add exact zeros.  Five relative
    # errors of at most 2^-24 each: 5 * 2^-24 and their second-order terms, below 6 * 2^-24.
    for L in (0.75, 1.0, 3.3, 1e-3, 5e4):
        rec = np.zeros(1, api.PROBE_DTYPE); rec["SH"][0, 0, :] = F32(2 * np.sqrt(np.pi) * L)
        for normal in n[:5]:
            e = api.sh9_irradiance(rec[0], normal).astype(np.float64)
            assert (np.abs(e / (np.pi * L) - 1) <= 6 * U).all(), (L, e)


def test_the_command_line_refuses_before_any_device_call(built, tmp_path):
    """A malformed size, a render flag beside --bake-probes, a bad resolution or file type: exit status 2, on a machine without a GPU too."""
    out = str(tmp_path / "probes.jsonl")
    base = [CLI, CORNELL, "--bake-probes", "3x2x2", "--probe-res", "8", "--probe-samples", "2", "--out", out]
    for extra in (["--spp", "4"], ["--denoise"], ["--width", "32"], ["--bake-lightmap", "8x8"], ["--resume", "x.tbs"], ["--ranks", "2"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "bake-probes" in r.stderr, (extra, r.returncode, r.stderr)
    for size in ("3x2", "3x2x", "3x2x2x2", "0x2x2", "3,2,2", "x2x2", "3x-2x2", "4096x4096x2", ""):
        r = subprocess.run([CLI, CORNELL, "--bake-probes", size, "--out", out], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (size, r.returncode, r.stderr)
    for args in (["--probe-res", "1"], ["--probe-res", "65"], ["--probe-samples", "0"], ["--probe-bounds", "0,0,0,1,1"], ["--probe-bounds", "0,0,0,1,1,nan"],
                 ["--out", str(tmp_path / "probes.json")]):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe_tb(built):
    """A context of this module's own: the cases load scenes under options that the session's context must not keep, and move them."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    tb._probe_scene = None
    yield tb
    tb.close()


def load(tb, name, fresh=False):
    import probe_cases as pc
    if tb._probe_scene != name or fresh:
        tb.SetOption("flatten_instances", 0 if name == "instances" else 1)
        try:
            tb.LoadScene(DYNAMIC_TRI3 if name == "tri3" else pc.SCENES[name])
        finally:
            tb.SetOption("flatten_instances", 1)
        tb._probe_scene = name
    return tb


def positions_in(tb, n, seed):
    """n seeded positions inside the middle 80 % of the scene's box"""
    info = tb.SceneInfo()
    lo, hi = np.array(info.sceneMin[:], float), np.array(info.sceneMax[:], float)
    return np.ascontiguousarray((lo + (0.1 + 0.8 * np.random.default_rng(seed).random((n, 3))) * (hi - lo)).astype(F32))


def by_the_queries(tb, positions, M, samples, first_number, settings, first_sample=0):
    """What a bake must return by its contract: the restatement's rays through the two queries, projected by the restatement."""
    import probe_cases as pc
    rad, qry = pc.rays(positions, M, first_number)
    sums = tb.TraceRadiance(rad.reshape(-1), samples, first_sample, 0.0, settings=settings).reshape(len(positions), M * M, 4)
    hits = tb.TraceRays(qry.reshape(-1)).reshape(len(positions), M * M)
    return sums, hits, pc.project(positions, M, sums, hits)


SEAM_POSITIONS = lambda n: np.ascontiguousarray((np.random.default_rng(n).uniform(-3, 3, (n, 3))).astype(F32))


@gpu
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("M", [2, 8, 9, 16])
def test_the_ray_kernel_is_the_restatement(gpu_tb, M, n):
    """1. M * M = 4 (fewer than a wave), 64 (one wave), 81 (ragged), 256 (four rounds); 1, 63 and 65 probes; one probe without a finite position."""
    import probe_cases as pc
    p = SEAM_POSITIONS(n)
    p[n // 2, 1] = np.nan if n > 1 else p[0, 1]
    rad, qry = gpu_tb.RunProbeRays(p, M, first_number=1000)
    want_rad, want_qry = pc.rays(p, M, 1000)
    assert same_bytes(rad, want_rad) and same_bytes(qry, want_qry)
    if n > 1:
        assert not rad[n // 2].view(np.uint32).any() and not qry[n // 2].view(np.uint32).any() and rad[0]["SeedX"][0] == 1000 and rad[n - 1]["SeedY"][-1] == M * M - 1


@gpu
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("M", [2, 8, 9, 16])
def test_the_projection_kernel_is_the_restatement(gpu_tb, M, n):
    """1. Seeded synthetic answers: rays without an accepted sample, an all-miss probe, sums over 24 orders of magnitude, a probe without a finite position."""
    import probe_cases as pc
    p = SEAM_POSITIONS(n)
    sums, hits = pc.synthetic_maps(n, M, seed=100 * M + n)
    if n > 1:
        p[n - 1, 2] = np.inf
    got = gpu_tb.RunProbeProject(p, M, sums, hits)
    want = pc.project(p, M, sums, hits)
    assert same_bytes(got, want)
    placed = np.isfinite(p).all(axis=1)
    assert np.isfinite(got["SH"]).all()
    assert np.array_equal(got["Weight"] > 0, placed & (sums[..., 3] > 0).any(axis=1))          # counted by hand: who has a ray with an accepted sample
    assert np.array_equal(got["Hits"], np.where(placed, (hits["T"] >= 0).sum(axis=1), 0))      # ... and how many rays hit
    met = got["Hits"] > 0
    assert (got["MinDistance"][met] <= got["MeanDistance"][met]).all() and (got["MinDistance"][~met] == -1).all() and (got["MeanDistance"][~met] == -1).all()
    assert np.array_equal(got["MinDistance"][met], np.where(hits["T"] >= 0, hits["T"], np.inf).min(axis=1)[met])
    if n > 1:
        assert got["Hits"][0] == 0 and (M == 2 or got["Weight"][0] > 0)                          # the all-miss probe still sees light
        last = got[n - 1]
        assert not last["SH"].any() and last["Weight"] == 0 and last["Hits"] == 0 and last["MinDistance"] == -1 and last["MeanDistance"] == -1
    # all rays rejected: no weight, zero coefficients
    dark = sums.copy(); dark[..., 3] = 0
    none = gpu_tb.RunProbeProject(p, M, dark, hits)
    assert same_bytes(none, pc.project(p, M, dark, hits)) and not none["SH"].any() and not none["Weight"].any()


@gpu
@pytest.mark.parametrize("scene", ["cornell-box", "mix-glass", "instances"])
def test_a_bake_is_the_two_queries_and_the_projection(probe_tb, settings, scene):
    """2. The kept maps are TraceRadiance and TraceRays on the restatement's rays, the records the restatement's projection of those maps."""
    tb = load(probe_tb, scene)
    assert (tb.HostSceneView().numInstances > 0) == (scene == "instances")
    pos = positions_in(tb, 5, seed=7)
    M, S = 8, 4
    got = tb.BakeProbes(pos, M, S, first_number=11, keep_maps=True, settings=settings)
    sums, hits = tb.ReadProbeMaps()
    want_sums, want_hits, want = by_the_queries(tb, pos, M, S, 11, settings)
    assert same(sums, want_sums) and same_bytes(hits, want_hits) and same_bytes(got, want)
    assert (got["Weight"] > 0).all() and (got["Hits"] > 0).all() and got["SH"][:, 0].max() > 0
    assert tb.GetOption("probes_held") == 5 and tb.GetOption("probes_resolution") == M and tb.GetOption("last_probes_batches") == 1


def emissive_box(tb, inward, L):
    import mesh_cases as mc
    import probe_cases as pc
    from tracerboy_amd import api
    p, idx, nrm = pc.box((-1, -1.5, -2), (1, 1.5, 2), inward)
    tb.LoadMeshes([api.Mesh(p, idx, normals=nrm, material=0)], [mc.emitter(*L)])
    tb._probe_scene = None


@gpu
@pytest.mark.parametrize("inward", [True, False], ids=["wound inward", "wound outward"])
@pytest.mark.parametrize("M", [8, 16])
def test_closed_forms(probe_tb, settings, M, inward):
    """3. Inside a closed box that emits L towards the probe and reflects nothing every ray brings L: SH[0] = 2 sqrt(pi) L within (M * M + 8) * 2^-24
    relative (M * M roundings at most along the longest chain of the sums, and the handful of the products and the quotient), the coefficients that
    symmetry cancels stay below the same share of SH[0], every ray hits, and none of the hits is a back face.  The same box wound outward, its
    normals with it: every ray hits and every hit is a back face -- what a sampler needs to leave the probe out -- and no light arrives at all,
    since the renderer's emitters shine from their front only (pt_device.hpp get_material: the emission of a back face is zero); the closed form
    of SH[0] has no meaning there."""
    import probe_cases as pc
    L = (0.75, 1.5, 2.0)                                               # few mantissa bits: the samples' sums are exact
    emissive_box(probe_tb, inward, L)
    tb = probe_tb
    pos = F32([[0.1, -0.2, 0.3], [-0.37, 0.61, -0.83]])                 # off the box's planes of symmetry: no ray runs along a triangle's edge
    got = tb.BakeProbes(pos, M, 4, settings=settings, keep_maps=True)
    sums, hits = tb.ReadProbeMaps()
    print("sums of ray 0:", sums[0, 0], "hit 0:", hits[0, 0], "Backfaces:", got["Backfaces"], "Hits:", got["Hits"])
    bound = (M * M + 8) * U
    assert (got["Hits"] == M * M).all() and (got["Weight"] > 0).all()
    assert (got["MinDistance"] > 0).all() and (got["MinDistance"] <= got["MeanDistance"]).all()
    if not inward:
        assert (got["Backfaces"] == M * M).all() and not got["SH"].any()
        return
    assert (got["Backfaces"] == 0).all()
    for c in range(3):
        rel = np.abs(got["SH"][:, 0, c].astype(np.float64) / (2 * np.sqrt(np.pi) * L[c]) - 1)
        print("M", M, "channel", c, "SH[0] relative error", rel, "bound", bound)
        assert (rel <= bound).all()
    # which coefficients vanish: the float64 evaluation of the same projection of a constant
    d, w, _ = pc.directions(M, np.float64)
    exact = 4 * np.pi * (pc.basis(d) * w[:, None]).sum(axis=0) / w.sum()
    small = np.abs(exact) < 1e-12 * exact[0]
    assert small[1:4].all() and small.sum() >= 5                       # the whole of order 1, and the odd products of order 2
    for c in range(3):
        assert (np.abs(got["SH"][:, small, c]) <= bound * got["SH"][:, 0, c][:, None]).all()


@gpu
def test_a_probe_that_sees_nothing(probe_tb, settings):
    """3. An open scene (one black triangle, no environment), a probe far outside whose rays all miss: zero SH, no hits, distances -1 -- and a weight,
    since a path that leaves the scene is an accepted sample of no light."""
    import mesh_cases as mc
    from tracerboy_amd import api
    tb = probe_tb
    tb.LoadMeshes([api.Mesh(F32([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]), np.uint32([[0, 1, 2]]), material=0)], [mc.matte(0, 0, 0)])
    tb._probe_scene = None
    got = tb.BakeProbes(F32([[50, 60, 70]]), 8, 2, settings=settings)[0]
    assert not got["SH"].any() and got["Hits"] == 0 and got["Backfaces"] == 0 and got["MinDistance"] == -1 and got["MeanDistance"] == -1


@gpu
def test_splits_and_order_change_no_byte(probe_tb, settings, monkeypatch):
    """4. Samples split over accumulated bakes, batches, the probes' order and the kind of array: the same records."""
    import torch
    tb = load(probe_tb, "cornell-box")
    pos = positions_in(tb, 5, seed=4)
    M = 8
    whole = tb.BakeProbes(pos, M, 8, first_number=10, keep_maps=True, settings=settings)
    whole_maps = tb.ReadProbeMaps()
    assert tb.GetOption("last_probes_batches") == 1
    # 3 + 5 = 8
    tb.BakeProbes(pos, M, 3, first_number=10, keep_maps=True, settings=settings)
    added = tb.BakeProbes(pos, M, 5, first_sample=3, first_number=10, accumulate=True, settings=settings)
    assert same_bytes(added, whole) and all(same_bytes(a, b) for a, b in zip(tb.ReadProbeMaps(), whole_maps))
    # three batches of 2, 2 and 1 probes
    monkeypatch.setenv("TB_PROBE_MAX_RAYS", str(2 * M * M + 5))
    cut = tb.BakeProbes(pos, M, 8, first_number=10, keep_maps=True, settings=settings)
    assert tb.GetOption("last_probes_batches") == 3
    assert same_bytes(cut, whole) and all(same_bytes(a, b) for a, b in zip(tb.ReadProbeMaps(), whole_maps))
    cut = tb.BakeProbes(pos, M, 8, first_number=10, settings=settings)                       # and without the maps: one batch's buffers, reused
    assert tb.GetOption("last_probes_batches") == 3 and same_bytes(cut, whole) and tb.GetOption("probes_maps_held") == 0
    monkeypatch.setenv("TB_PROBE_MAX_RAYS", "1")                                             # a batch is at least one probe
    assert same_bytes(tb.BakeProbes(pos, M, 8, first_number=10, settings=settings), whole) and tb.GetOption("last_probes_batches") == 5
    monkeypatch.delenv("TB_PROBE_MAX_RAYS")
    # reversed, each probe in a call of its own with its number
    for i in reversed(range(5)):
        assert same_bytes(tb.BakeProbes(pos[i:i + 1], M, 8, first_number=10 + i, settings=settings), whole[i:i + 1]), i
    # device tensors
    dev = tb.BakeProbes(torch.from_numpy(pos).to("cuda:0"), M, 8, first_number=10, settings=settings)
    assert dev.is_cuda and tuple(dev.shape) == (5, 32) and same_bytes(dev.cpu().numpy().view(whole.dtype).reshape(-1), whole)


@pytest.fixture(scope="module")
def cornell_grid(probe_tb, settings):
    from tracerboy_amd import api
    tb = load(probe_tb, "cornell-box")
    # inside the box's [-1, 1] x [0, 2] x [-1, 1]; origin and spacing have few mantissa bits, so a probe's position gives whole grid coordinates exactly
    grid = api.ProbeGrid((-0.5, 0.5, -0.5), (0.5, 1.0, 1.0), (3, 2, 2))
    probes = tb.BakeProbes(api.probe_grid_positions(grid), 8, 4, settings=settings)
    return grid, probes


def sample_points(grid, n, seed):
    """n seeded points: inside the grid, outside it (clamped) and exactly on probes; unit normals"""
    from tracerboy_amd import api
    rng = np.random.default_rng(seed)
    o, sp, cnt = np.array(grid.origin), np.array(grid.spacing), np.array(grid.count)
    pts = o + rng.uniform(-0.7, cnt - 1 + 0.7, (n, 3)) * sp
    on = api.probe_grid_positions(grid)
    pts = pts.astype(F32); pts[: len(on)] = on
    nrm = rng.normal(size=(n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm)


@gpu
def test_sampling_is_the_restatement(probe_tb, cornell_grid):
    """5. 257 points (more than one workgroup, no multiple of a wave) inside, outside and on probes; a probe's own position gives its own irradiance."""
    import torch
    import probe_cases as pc
    from tracerboy_amd import api
    grid, probes = cornell_grid
    pts, nrm = sample_points(grid, 257, seed=5)
    got = probe_tb.SampleProbes(grid, probes, pts, nrm, resolution=8, backface_limit=1.0)
    want = pc.sample(grid, 8, 1.0, probes, pts, nrm)
    assert same(got, want) and (got[:, 3] > 0).all()
    for i in range(grid.n):                                            # on a probe: weight 1 on it alone
        assert got[i, 3] == 1 and same(got[i, :3], api.sh9_irradiance(probes[i], nrm[i])), i
    dev = probe_tb.SampleProbes(grid, torch.from_numpy(probes.view(F32).reshape(-1, 32)).to("cuda:0"), torch.from_numpy(pts).to("cuda:0"),
                                torch.from_numpy(nrm).to("cuda:0"), resolution=8, backface_limit=1.0)
    assert same(dev.cpu().numpy(), want)


@gpu
def test_sampling_leaves_invalid_probes_out(probe_tb, cornell_grid):
    """5. One corner made invalid through its back faces: the other seven renormalise; all eight invalid: zeros; axes of one probe."""
    import probe_cases as pc
    from tracerboy_amd import api
    grid, baked = cornell_grid
    pts, nrm = sample_points(grid, 257, seed=6)
    probes = baked.copy()
    probes["Backfaces"] = 0; probes["Backfaces"][4] = 17               # 17 of 64 rays: above a limit of 0.25 (16), within one of 0.5
    got = probe_tb.SampleProbes(grid, probes, pts, nrm, resolution=8, backface_limit=0.25)
    assert same(got, pc.sample(grid, 8, 0.25, probes, pts, nrm))
    assert same(probe_tb.SampleProbes(grid, probes, pts, nrm, resolution=8, backface_limit=0.5), pc.sample(grid, 8, 0.5, probes, pts, nrm))
    assert not got[4].any()                                            # on the invalid probe itself: nothing else has weight
    near = (got[:, 3] > 0) & (got[:, 3] < 1)
    assert near.any()
    centre = F32([np.array(grid.origin) + np.array(grid.spacing) * [1.25, 0.5, 0.5]])      # inside the cell whose corners include probe 4 = (1, 1, 0)
    e = probe_tb.SampleProbes(grid, probes, centre, nrm[:1], resolution=8, backface_limit=0.25)
    full = probe_tb.SampleProbes(grid, probes, centre, nrm[:1], resolution=8, backface_limit=0.5)
    assert abs(float(full[0, 3]) - 1) <= 16 * U and abs(float(e[0, 3]) - (1 - 0.75 * 0.5 * 0.5)) <= 16 * U
    # the seven that count, renormalised by hand in float64, to the rounding of the device's 27 x 8 sums
    o, sp = np.array(grid.origin), np.array(grid.spacing)
    acc = np.zeros((9, 3)); wsum = 0.0
    for c in range(8):
        d = np.array([c & 1, (c >> 1) & 1, c >> 2]); ijk = np.array([1, 0, 0]) + d
        k = (ijk[2] * 2 + ijk[1]) * 3 + ijk[0]
        w = np.prod(np.where(d == 1, [0.25, 0.5, 0.5], [0.75, 0.5, 0.5]))
        if k != 4:
            acc += w * probes["SH"][k].astype(np.float64); wsum += w
    rec = np.zeros(1, api.PROBE_DTYPE); rec["SH"][0] = (acc / wsum).astype(F32)
    assert np.allclose(e[0, :3], api.sh9_irradiance(rec[0], nrm[0]), rtol=1e-5, atol=1e-6 * float(np.abs(e[0, :3]).max() + 1e-30))
    # all invalid
    probes["Backfaces"] = 64
    none = probe_tb.SampleProbes(grid, probes, pts, nrm, resolution=8, backface_limit=0.25)
    assert not none.any() and same(none, pc.sample(grid, 8, 0.25, probes, pts, nrm))
    probes["Backfaces"] = 0; probes["Weight"] = 0
    assert not probe_tb.SampleProbes(grid, probes, pts, nrm, resolution=8, backface_limit=1.0).any()
    # counts of 1: a line, a plane and a single probe
    for count in ((3, 1, 1), (1, 2, 2), (1, 1, 1), (3, 2, 1)):
        g = api.ProbeGrid(grid.origin, grid.spacing, count)
        sub = np.ascontiguousarray(baked[: g.n])
        p2, n2 = sample_points(g, 65, seed=sum(count))
        got = probe_tb.SampleProbes(g, sub, p2, n2, resolution=8, backface_limit=1.0)
        assert same(got, pc.sample(g, 8, 1.0, sub, p2, n2)) and (np.abs(got[:, 3] - 1) <= 16 * U).all(), count   # 8 weights of 3 roundings each, 7 sums


@gpu
def test_a_bake_follows_a_committed_scene(probe_tb, settings):
    """6. After UpdatePositions + CommitGeometry a bake is the queries on the moved scene, and an accumulation onto the bake before it is refused."""
    from tracerboy_amd import api
    tb = load(probe_tb, "tri3", fresh=True)
    host = api.HostScene(DYNAMIC_TRI3).triangles()["positions"]
    pos = positions_in(tb, 3, seed=9)
    M, S = 9, 2
    before = tb.BakeProbes(pos, M, S, keep_maps=True, settings=settings)
    moved = (host + np.random.default_rng(3).uniform(-0.2, 0.2, host.shape)).astype(F32)
    tb.UpdatePositions(moved); tb.CommitGeometry()
    with pytest.raises(api.TracerBoyError):
        tb.BakeProbes(pos, M, S, first_sample=S, accumulate=True, settings=settings)
    after = tb.BakeProbes(pos, M, S, keep_maps=True, settings=settings)
    sums, hits = tb.ReadProbeMaps()
    want_sums, want_hits, want = by_the_queries(tb, pos, M, S, 0, settings)
    assert same(sums, want_sums) and same_bytes(hits, want_hits) and same_bytes(after, want)
    assert not same_bytes(after, before)
    tb._probe_scene = None                                             # moved: the next test loads it again


@gpu
def test_every_refusal_on_a_live_context(built, settings):
    """7. Each refusal is followed by a correct bake, and the maps held after a refusal are the previous bake's."""
    import torch
    from tracerboy_amd import _ctypes_abi as abi, api
    INVALID, NO_SCENE, UNSUPPORTED = -1, -7, -6
    with api.TracerBoy(0) as tb:
        pos = np.ascontiguousarray(F32([[0.1, 0.5, 0.2], [-0.3, 1.0, 0.1], [0.2, 1.5, -0.4]]))
        with pytest.raises(api.TracerBoyError) as e:
            tb.BakeProbes(pos, 8, 1)
        assert e.value.code == NO_SCENE
        with pytest.raises(api.TracerBoyError):
            tb.ReadProbeMaps()
        tb.LoadScene(CORNELL)
        with pytest.raises(api.TracerBoyError):
            tb.ReadProbeMaps()                                        # nothing baked yet
        with pytest.raises(api.TracerBoyError):
            tb.BakeProbes(pos, 8, 1, accumulate=True, settings=settings)    # nothing to add to
        pos = positions_in(tb, 3, seed=2)
        good = tb.BakeProbes(pos, 8, 2, keep_maps=True, settings=settings); held = tb.ReadProbeMaps()

        def still_held():
            assert all(same_bytes(a, b) for a, b in zip(tb.ReadProbeMaps(), held))
            assert same_bytes(tb.BakeProbes(pos, 8, 2, keep_maps=True, settings=settings), good)

        def refused(code, **kw):
            args = dict(positions=pos, resolution=8, samples=2, settings=settings); args.update(kw)
            with pytest.raises(api.TracerBoyError) as e:
                tb.BakeProbes(**args)
            assert e.value.code == code, (kw, str(e.value))
            still_held()

        realtime = copy.copy(settings); realtime.RenderModeRealTime = 1
        refused(UNSUPPORTED, settings=realtime)
        refused(INVALID, resolution=9, accumulate=True)               # another resolution than the bake held
        refused(INVALID, positions=pos[:2], accumulate=True)          # another number of probes
        # what Python's own checks keep from the library, through the library: the table's rows on a live context
        out = np.zeros(3, api.PROBE_DTYPE)
        raw = lambda call, p_, o: tb._L.tb_bake_probes(tb._ctx, None, 0.0, ctypes.byref(call) if call is not None else None, p_, o)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        C = abi.tb_probe_call
        for call, p_, o in ((None, p(pos), p(out)), (C(3, 0, 1, 0, 2, 0), p(pos), p(out)), (C(3, 0, 65, 0, 2, 0), p(pos), p(out)),
                            (C((1 << 19) + 1, 0, 64, 0, 2, 0), p(pos), p(out)), (C((1 << 24) + 1, 0, 2, 0, 2, 0), p(pos), p(out)), (C(3, (1 << 24) - 2, 8, 0, 2, 0), p(pos), p(out)),
                            (C(3, 0, 8, 0, 0, 0), p(pos), p(out)), (C(3, 0, 8, 0, (1 << 24) + 1, 0), p(pos), p(out)), (C(3, 0, 8, 0xffffffff, 2, 0), p(pos), p(out)),
                            (C(3, 0, 8, 0, 2, 0x800), p(pos), p(out)), (C(3, 0, 8, 0, 2, 0), None, p(out)), (C(3, 0, 8, 0, 2, 0), p(pos), None),
                            (C(3, 0, 8, 0, 2, api.PROBES_DEVICE), p(pos), p(out))):          # host memory passed as device memory
            assert raw(call, p_, o) == INVALID
            still_held()
        dev = torch.zeros((3 * 32 + 4,), dtype=torch.float32, device="cuda:0"); dpos = torch.from_numpy(pos).to("cuda:0")
        call = C(3, 0, 8, 0, 2, api.PROBES_DEVICE)
        assert raw(call, ctypes.c_void_p(dpos.data_ptr()), ctypes.c_void_p(dev.data_ptr() + 4)) == INVALID            # misaligned records
        assert raw(call, ctypes.c_void_p(dpos.data_ptr() + 2), ctypes.c_void_p(dev.data_ptr())) == INVALID            # misaligned positions
        # runs past its allocation (torch's allocator hands out parts of larger blocks: 2 GiB is past any block that holds a 400 B tensor)
        assert raw(C(1 << 24, 0, 8, 0, 2, api.PROBES_DEVICE), ctypes.c_void_p(dpos.data_ptr()), ctypes.c_void_p(dev.data_ptr())) == INVALID
        still_held()
        assert raw(C(0, 0, 8, 0, 2, 0), None, None) == 0              # no probes: TB_OK, nothing launched, the bake held stays
        still_held()
        # the sampler's refusals
        grid = api.ProbeGrid((0, 0, 0), (1, 1, 1), (3, 1, 1)); g = grid.c_struct()
        pts = np.zeros((2, 3), F32); rgba = np.zeros((2, 4), F32)
        smp = lambda flags, g_, res, limit, pr, n, a, b, o: tb._L.tb_sample_probes(tb._ctx, flags, g_, res, limit, pr, n, a, b, o)
        assert smp(0, ctypes.byref(g), 8, 0.25, p(good), 2, p(pts), p(pts), p(rgba)) == 0
        zero = abi.tb_probe_grid((ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_uint32 * 3)(3, 0, 1))
        for args in ((1, ctypes.byref(g), 8, 0.25, p(good), 2, p(pts), p(pts), p(rgba)), (0, None, 8, 0.25, p(good), 2, p(pts), p(pts), p(rgba)),
                     (0, ctypes.byref(g), 1, 0.25, p(good), 2, p(pts), p(pts), p(rgba)), (0, ctypes.byref(zero), 8, 0.25, p(good), 2, p(pts), p(pts), p(rgba)),
                     (0, ctypes.byref(g), 8, float("nan"), p(good), 2, p(pts), p(pts), p(rgba)), (0, ctypes.byref(g), 8, 0.25, None, 2, p(pts), p(pts), p(rgba)),
                     (0, ctypes.byref(g), 8, 0.25, p(good), 2, p(pts), None, p(rgba)), (0, ctypes.byref(g), 8, 0.25, p(good), 2, p(pts), p(pts), None),
                     (api.PROBES_DEVICE, ctypes.byref(g), 8, 0.25, p(good), 2, p(pts), p(pts), p(rgba))):
            assert smp(*args) == INVALID, args
        assert smp(0, ctypes.byref(g), 8, 0.25, p(good), 0, None, None, None) == 0
        still_held()
    if torch.cuda.device_count() > 1:
        with api.TracerBoy(devices=[0, 1]) as group:
            group.LoadScene(CORNELL)
            with pytest.raises(api.TracerBoyError) as e:
                group.BakeProbes(pos, 8, 2, settings=settings)
            assert e.value.code == UNSUPPORTED


@gpu
def test_probes_hold_memory_from_the_first_bake_to_the_scenes_release(built, settings):
    """debug_live_device_bytes rises at the first bake by at least the records and one batch's four per-ray buffers (128 B a ray), stays at a second of the
    same size, and a new scene or close() gives everything back."""
    from tracerboy_amd import api
    with api.TracerBoy(0) as other:                                   # the count is the process's: read through a context that stays
        before = other.GetOption("debug_live_device_bytes")
        tb = api.TracerBoy(0)
        tb.LoadScene(CORNELL)
        pos = positions_in(tb, 4, seed=1)
        tb.TraceRadiance(api.make_radiance_rays(np.zeros((1, 3)), [[0, 1, 0]]), settings=settings)        # the queries' own buffers
        tb.TraceRays(api.make_query_rays(np.zeros((1, 3)), [[0, 1, 0]]))
        loaded = other.GetOption("debug_live_device_bytes")
        assert tb.GetOption("probes_held") == 0
        tb.BakeProbes(pos, 8, 1, settings=settings)
        first = other.GetOption("debug_live_device_bytes")
        assert first >= loaded + 4 * 64 * 128 + 4 * 128 + 4 * 12 and tb.GetOption("probes_held") == 4
        tb.BakeProbes(pos, 8, 2, settings=settings)
        assert other.GetOption("debug_live_device_bytes") == first
        tb.BakeProbes(pos, 8, 2, keep_maps=True, settings=settings)   # the same 4 x 64 rays: one batch is the whole bake
        tb.BakeProbes(pos, 8, 1, first_sample=2, accumulate=True, settings=settings)
        assert other.GetOption("debug_live_device_bytes") == first
        tb.close()
        assert other.GetOption("debug_live_device_bytes") == before


@gpu
def test_the_command_line_bakes(probe_tb, tmp_path):
    from tracerboy_amd import api
    out = str(tmp_path / "probes.jsonl")
    r = subprocess.run([CLI, CORNELL, "--bake-probes", "3x2x2", "--probe-res", "8", "--probe-samples", "2", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tb = load(probe_tb, "cornell-box")
    info = tb.SceneInfo()
    grid = api.ProbeGrid.in_bounds(info.sceneMin[:], info.sceneMax[:], (3, 2, 2))
    pos = api.probe_grid_positions(grid)
    lines = [json.loads(l) for l in open(out)]
    assert [l["probe"] for l in lines] == list(range(12))
    assert np.abs(np.array([l["position"] for l in lines]) - pos).max() <= 1e-5 * np.abs(pos).max()
    want = tb.BakeProbes(np.ascontiguousarray(F32([l["position"] for l in lines])), 8, 2)
    assert same(np.array([l["sh"] for l in lines]).reshape(12, 9, 3), want["SH"])
    for key, field in (("weight", "Weight"), ("hits", "Hits"), ("backfaces", "Backfaces"), ("min_distance", "MinDistance"), ("mean_distance", "MeanDistance")):
        assert same([l[key] for l in lines], want[field]), key
