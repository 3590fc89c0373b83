"""Radiance queries (include/tracerboy_hip.h tb_trace_radiance / tb_make_camera_rays): the path tracer on a caller's rays.
Every expected value comes from the CPU oracle, from tb_render or from a closed form (tests/radiance_cases.py); every comparison is on bits."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

gpu = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _struct_offsets(struct):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), _header("tb_abi.h"), re.S).group(1)
    offsets, at = {}, 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "uint32_t"), decl
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            offsets[m.group(1)] = at
            at += 4 * int(m.group(2) or 1)
    return offsets, at


def test_header_exports_bindings_and_methods_agree(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    h = _header("tracerboy_hip.h")
    assert re.search(r"\bint\s+tb_trace_radiance\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*const\s+tb_output_settings\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*const\s+TbRadianceCall\s*\*"
                     r"\s*\w+\s*,\s*uint64_t\s+\w+\s*,\s*const\s+TbRadianceRay\s*\*\s*\w+\s*,\s*TbFloat4\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_make_camera_rays\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*const\s+tb_output_settings\s*\*\s*\w+\s*,\s*float\s+\w+\s*,(\s*uint32_t\s+\w+\s*,){8}"
                     r"\s*TbRadianceRay\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", h)
    for name, value in (("TB_RADIANCE_RAY", "0u"), ("TB_RADIANCE_HEMISPHERE", "1u"), ("TB_RADIANCE_DEVICE", "0x100u"), ("TB_RADIANCE_ACCUMULATE", "0x200u"),
                        ("TB_RAYS_DEVICE", "0x100u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), h), name
    assert (api.RADIANCE_RAY, api.RADIANCE_HEMISPHERE, api.RADIANCE_DEVICE, api.RADIANCE_ACCUMULATE) == (0, 1, 0x100, 0x200)
    for struct, mirror, size in (("TbRadianceRay", abi.TbRadianceRay, 32), ("TbRadianceCall", abi.TbRadianceCall, 16)):
        offsets, total = _struct_offsets(struct)
        assert ctypes.sizeof(mirror) == total == size
        assert {n: getattr(mirror, n).offset for n, _ in mirror._fields_} == offsets
    offsets, _ = _struct_offsets("TbRadianceRay")
    assert api.RADIANCE_RAY_DTYPE.itemsize == 32 and {n: api.RADIANCE_RAY_DTYPE.fields[n][1] for n in api.RADIANCE_RAY_DTYPE.names} == offsets
    raw = ctypes.CDLL(api.LIB_PATH); bound = api.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in ("tb_trace_radiance", "tb_make_camera_rays", "tb_radiance_refusal"):
        assert hasattr(raw, name) and name in bound._tb_exports, name
    assert bound.tb_trace_radiance.argtypes == [vp, ctypes.POINTER(abi.tb_output_settings), ctypes.c_float, ctypes.POINTER(abi.TbRadianceCall), ctypes.c_uint64, vp, vp]
    assert bound.tb_make_camera_rays.argtypes == [vp, ctypes.POINTER(abi.tb_output_settings), ctypes.c_float] + [u32] * 8 + [vp, ctypes.POINTER(ctypes.c_float)]
    assert callable(api.TracerBoy.TraceRadiance) and callable(api.TracerBoy.MakeCameraRays) and callable(api.make_radiance_rays)


def test_make_radiance_rays_packs_what_it_is_given():
    from tracerboy_amd import api
    o = np.arange(15, dtype=np.float64).reshape(5, 3); d = -o
    r = api.make_radiance_rays(o, d)
    assert r.dtype == api.RADIANCE_RAY_DTYPE and r.shape == (5,) and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r["Origin"], o.astype(F32)) and np.array_equal(r["Direction"], d.astype(F32))
    assert r["SeedX"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and r["SeedY"].tolist() == [0.0] * 5
    big = api.make_radiance_rays(np.zeros((4098, 3)), np.ones((4098, 3)))
    assert (big["SeedX"][4095], big["SeedY"][4095], big["SeedX"][4096], big["SeedY"][4096], big["SeedX"][4097]) == (4095.0, 0.0, 0.0, 1.0, 1.0)
    r = api.make_radiance_rays(o, d, seed_xy=[[7, 9]] * 5)
    flat = r.view(F32).reshape(5, 8)                                  # the (n, 8) float32 form of the same bytes
    assert np.array_equal(flat[:, 0:3], r["Origin"]) and np.array_equal(flat[:, 4:7], r["Direction"])
    assert flat[:, 3].tolist() == [7.0] * 5 and flat[:, 7].tolist() == [9.0] * 5
    for bad in ((o, d[:4], None), (o[:, :2], d[:, :2], None), (o, d, np.zeros((4, 2))), (o, d, np.zeros(5))):
        with pytest.raises(ValueError):
            api.make_radiance_rays(*bad)


def test_wrong_inputs_are_refused_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    good = api.make_radiance_rays(np.zeros((6, 3)), np.ones((6, 3)))
    wrong = {
        "dtype float64": np.zeros((6, 8), np.float64), "shape (n, 7)": np.zeros((6, 7), F32), "shape (n,)": np.zeros(48, F32),
        "the query-ray dtype": np.zeros(6, api.QUERY_RAY_DTYPE), "two dimensions of the structured dtype": np.zeros((2, 3), api.RADIANCE_RAY_DTYPE),
        "a non-contiguous float array": np.zeros((12, 8), F32)[::2], "a non-contiguous structured array": np.zeros(12, api.RADIANCE_RAY_DTYPE)[::2],
        "a list": [[0.0] * 8], "a tensor on the CPU": torch.zeros((6, 8), dtype=torch.float32), "a float64 tensor": torch.zeros((6, 8), dtype=torch.float64),
    }
    for what, rays in wrong.items():
        with pytest.raises(ValueError):
            tb.TraceRadiance(rays)
            pytest.fail(what)
    for kw in (dict(samples=0), dict(samples=(1 << 24) + 1), dict(samples=1.5), dict(first_sample=-1), dict(first_sample=(1 << 32) - 1, samples=2),
               dict(seed_advance=float("nan")), dict(seed_advance="16"), dict(mode=2), dict(mode=api.RADIANCE_DEVICE), dict(mode=None),
               dict(out=np.zeros((6, 4), np.float64)), dict(out=np.zeros((5, 4), F32)), dict(out=np.zeros((12, 4), F32)[::2]),
               dict(out=torch.zeros((6, 4), dtype=torch.float32))):
        with pytest.raises(ValueError):
            tb.TraceRadiance(good, **kw)
            pytest.fail(str(kw))
    for args in ((0, 24, 0), (32, 24, -1), (32, 24, 0, (0, 0, 33, 24)), (32, 24, 0, (5, 5, 5, 6)), (32, 24, 0, (0, 0, 8, 25)), (1 << 15, 24, 0)):
        with pytest.raises(ValueError):
            tb.MakeCameraRays(*args)
            pytest.fail(str(args))
    with pytest.raises(AttributeError):                               # the good array gets past the checks, to the library this object lacks
        tb.TraceRadiance(good, samples=3, first_sample=5, seed_advance=16.0, mode=api.RADIANCE_HEMISPHERE, out=np.zeros((6, 4), F32))


def test_the_refusal_table(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    call = lambda first=0, samples=1, advance=0.0, flags=0: abi.TbRadianceCall(first, samples, advance, flags)
    A = 0x10000                                                       # any aligned non-null address: the function compares, it does not read
    assert api.RadianceRefusal(call(), 5, A, A) is None
    assert api.RadianceRefusal(call(flags=api.RADIANCE_HEMISPHERE | api.RADIANCE_DEVICE | api.RADIANCE_ACCUMULATE), 1 << 31, A, A) is None
    assert api.RadianceRefusal(call(first=(1 << 32) - (1 << 24), samples=1 << 24), 5, A, A) is None
    assert api.RadianceRefusal(call(), 0, 0, 0) is None               # n = 0 asks for no pointers
    assert api.RadianceRefusal(call(), 5, A + 4, A + 8) is None       # host arrays need no alignment
    table = [
        (None, 5, A, A, "null call"),
        (call(flags=0x400), 5, A, A, "flag"), (call(flags=0x80000000), 5, A, A, "flag"), (call(flags=2), 5, A, A, "mode"), (call(flags=0xff), 5, A, A, "mode"),
        (call(samples=0), 5, A, A, "num_samples"), (call(samples=(1 << 24) + 1), 5, A, A, "2^24"),
        (call(first=0xffffffff, samples=2), 5, A, A, "2^32"), (call(advance=float("nan")), 5, A, A, "seed_advance"), (call(advance=float("inf")), 5, A, A, "seed_advance"),
        (call(), (1 << 31) + 1, A, A, "2^31"), (call(), 5, 0, A, "null"), (call(), 5, A, 0, "null"),
        (call(flags=api.RADIANCE_DEVICE), 5, A + 4, A, "aligned"), (call(flags=api.RADIANCE_DEVICE), 5, A, A + 8, "aligned"),
    ]
    for c, n, r, o, word in table:
        why = api.RadianceRefusal(c, n, r, o)
        assert why is not None and word in why, (word, why)


def test_the_generators_yield_what_the_cases_assume(built, settings):
    """On the CPU: the seeds of the camera cases and of the hemisphere case compose exactly (radiance_cases.compose_exactly), the hemisphere points
    lie on surfaces, the light ray meets the light first and the leaving ray meets nothing."""
    import oracle_lib as ol
    import radiance_cases as rc
    from tracerboy_amd import api
    ys, xs = np.mgrid[0:rc.H, 0:rc.W]
    differ = 0
    for f in range(rc.FRAMES):
        h = rc.hash13(xs.ravel(), ys.ravel(), F32(f))
        assert same(rc.start_seed(xs.ravel(), ys.ravel(), f, 16.0), rc.stepped(h, 16)) and same(rc.start_seed(xs.ravel(), ys.ravel(), f, 0.0), h)
        assert same(rc.stepped(rc.start_seed(xs.ravel(), ys.ravel(), f, 16.0), 2), rc.start_seed(xs.ravel(), ys.ravel(), f, 18.0))
        differ += int(rc.one_addition_differs(xs.ravel(), ys.ravel(), f, 16.0).sum())
    assert differ > 0                                                 # (10, 0) of frame 0 among them: one addition would not be the renderer's seed
    assert same(rc.start_seed([3], [4], 5, 2.5), (rc.stepped(rc.hash13([3], [4], F32(5)), 2) + F32(0.5)).astype(F32))
    assert same(rc.start_seed([3], [4], 5, -2.0), (rc.hash13([3], [4], F32(5)) + F32(-2.0)).astype(F32))
    hs = api.HostScene(rc.SCENES["cornell-box"])
    case = hemisphere_case(hs.view(), hs.info())
    assert len(case.rays) == 257 and np.allclose(np.linalg.norm(case.rays["Direction"], axis=1), 1.0, atol=1e-5)
    probe = ol.trace_closest(hs.view(), case.rays["Origin"] - F32(0.01) * case.rays["Direction"], case.rays["Direction"])
    assert (np.abs(probe["t"] - 0.01) < 1e-3).mean() > 0.95          # a step back along the normal and forward again meets the surface at once
    known = known_rays(hs.view(), hs.info(), hs.camera())
    assert known.hit["t"][0] > 0 and known.emissive.max() > 0 and known.hit["t"][1] < 0


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------------

class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


HEMI_ADVANCE, HEMI_SAMPLES = 16.0, (0, 1, 5)


def hemisphere_case(view, info):
    """257 points with normals on cornell-box surfaces, the default seeds."""
    import radiance_cases as rc
    from tracerboy_amd import api
    p, nrm = rc.surface_points(view, info.sceneMin[:], info.sceneMax[:], 257, seed=31)
    return Bag(rays=api.make_radiance_rays(p, nrm))


def known_rays(view, info, camera):
    """Ray 0 looks straight at the cornell light from below it, ray 1 leaves the box through its open side (towards the camera)."""
    import oracle_lib as ol
    import radiance_cases as rc
    from tracerboy_amd import api
    lo, hi = np.float32(info.sceneMin[:]), np.float32(info.sceneMax[:])
    light = rc.light_of(view)
    centre = ((lo + hi) / 2).astype(F32)
    below = light.copy(); below[1] = centre[1]
    out_dir = rc.unit((np.float32(camera.Position[:]) - centre)[None])[0]
    o = np.stack([below, centre]).astype(F32); d = np.stack([rc.unit((light - below)[None])[0], out_dir]).astype(F32)
    hit = ol.trace_closest(view, o, d)
    e = view.materials[int(hit["material"][0])].emissive if hit["t"][0] > 0 else None
    emissive = np.float32([e.x, e.y, e.z]) if e is not None else np.zeros(3, F32)
    return Bag(rays=api.make_radiance_rays(o, d, [[11, 13], [17, 19]]), hit=hit, emissive=emissive)


@pytest.fixture(scope="module")
def rad_tb(built):
    """A context of this module's own: the cases load scenes under options that the session's context must not keep."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    tb._rad_scene = None
    yield tb
    tb.close()


def load(tb, name):
    import radiance_cases as rc
    if tb._rad_scene != name:
        tb.SetOption("flatten_instances", 0 if name == "instances" else 1)
        try:
            tb.LoadProcedural(0, rc.PROC_TRIANGLES, rc.PROC_SEED) if name == "proc40k" else tb.LoadScene(rc.SCENES[name])
        finally:
            tb.SetOption("flatten_instances", 1)
        tb._rad_scene = name
    return tb


def with_blue_noise(settings, on):
    s = copy.copy(settings); s.EnableBlueNoise = on
    return s


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("blue_noise", [0, 1])
@pytest.mark.parametrize("scene", ["cornell-box", "mix-glass", "Teapot", "instances"])
def test_the_path_is_the_renders_path(rad_tb, settings, scene, blue_noise):
    """1. Camera rays of frame f traced with one sample numbered f are the oracle's frame f, all four channels; the four frames accumulated are
    tb_render's accumulation; the same through device tensors; a window is the slice."""
    import oracle_lib as ol
    import radiance_cases as rc
    import torch
    tb = load(rad_tb, scene)
    s = with_blue_noise(settings, blue_noise)
    view = tb.HostSceneView()
    assert (view.numInstances > 0) == (scene == "instances")
    acc = np.zeros((rc.W * rc.H, 4), F32); acc_dev = torch.zeros((rc.W * rc.H, 4), dtype=torch.float32, device="cuda:0")
    for f in range(rc.FRAMES):
        rays, adv = tb.MakeCameraRays(rc.W, rc.H, f, settings=s)
        assert adv == (0.0 if blue_noise else 16.0)
        ys, xs = np.mgrid[0:rc.H, 0:rc.W]
        assert np.array_equal(rays["SeedX"], xs.ravel().astype(F32)) and np.array_equal(rays["SeedY"], ys.ravel().astype(F32))
        want = ol.render(view, tb.FrameConstants(rc.W, rc.H, f, s, 0.0), rc.W, rc.H, 1, first_frame=f)["output"].reshape(-1, 4)
        got = tb.TraceRadiance(rays, 1, f, adv, settings=s)
        assert same(got, want), (scene, f, np.flatnonzero((bits(got) != bits(want)).any(1))[:8])
        assert tb.TraceRadiance(rays, 1, f, adv, settings=s, out=acc) is acc
        dev, adv_dev = tb.MakeCameraRays(rc.W, rc.H, f, settings=s, device=True)
        assert adv_dev == adv and dev.dtype == torch.float32 and tuple(dev.shape) == (rc.W * rc.H, 8)
        assert same(dev.cpu().numpy(), rays.view(F32).reshape(-1, 8))
        assert same(tb.TraceRadiance(dev, 1, f, adv, settings=s).cpu().numpy(), want)
        assert tb.TraceRadiance(dev, 1, f, adv, settings=s, out=acc_dev) is acc_dev
        if f == 1:
            x0, y0, x1, y1 = rc.WINDOW
            part, adv_part = tb.MakeCameraRays(rc.W, rc.H, f, window=rc.WINDOW, settings=s)
            assert adv_part == adv and same(part.view(F32).reshape(-1, 8), rays.view(F32).reshape(rc.H, rc.W, 8)[y0:y1, x0:x1].reshape(-1, 8))
            assert same(tb.TraceRadiance(part, 1, f, adv, settings=s), want.reshape(rc.H, rc.W, 4)[y0:y1, x0:x1].reshape(-1, 4))
    assert (want[:, 3] == 1).all() and want[:, :3].max() > 0
    tb.InvalidateHistory()
    tb.Render(rc.W, rc.H, rc.FRAMES, s, 0.0)
    rendered = tb.ReadAccumulation().reshape(-1, 4)
    assert same(acc, rendered) and same(acc_dev.cpu().numpy(), rendered)
    assert tb.GetOption("last_radiance_us") > 0


@gpu
def test_hemisphere_mode_is_the_references_sampler(rad_tb, settings):
    """2. Hemisphere mode with seed_advance A equals ray mode along the oracle's GenerateCosineWeightedDirection of the two numbers drawn at
    hash13(SeedX, SeedY, s) + A, with seed_advance A + 2."""
    import radiance_cases as rc
    from tracerboy_amd import api
    tb = load(rad_tb, "cornell-box")
    case = hemisphere_case(tb.HostSceneView(), tb.SceneInfo())
    rays, A = case.rays, HEMI_ADVANCE
    lit = 0
    for s in HEMI_SAMPLES:
        seeds = rc.start_seed(rays["SeedX"], rays["SeedY"], s, A)
        along = rays.copy(); along["Direction"] = rc.cosine_directions(seeds, 0.0, rays["Direction"])
        assert ((along["Direction"] * rays["Direction"]).sum(1) > -1e-5).all()
        want = tb.TraceRadiance(along, 1, s, A + 2, settings=settings)
        got = tb.TraceRadiance(rays, 1, s, A, mode=api.RADIANCE_HEMISPHERE, settings=settings)
        assert same(got, want), (s, np.flatnonzero((bits(got) != bits(want)).any(1))[:8])
        lit += int((got[:, :3].sum(1) > 0).sum())
    assert lit > 100


@gpu
@pytest.mark.parametrize("scene", ["cornell-box", "proc40k"])
def test_the_sum_is_sequential(rad_tb, settings, scene, monkeypatch):
    """3. 8 samples in one call = 8 one-sample calls accumulated = 3 + 5, and = the call cut into launches by a lowered split."""
    import radiance_cases as rc
    tb = load(rad_tb, scene)
    info = tb.SceneInfo()
    assert (info.numTriangles >= 32768) == (scene == "proc40k")
    rays = rc.random_rays(info.sceneMin[:], info.sceneMax[:], 1000, seed=41)
    whole = tb.TraceRadiance(rays, 8, 2, 16.0, settings=settings)
    assert tb.GetOption("last_radiance_launches") == 1 and (whole[:, 3] == 8).all()
    if scene == "cornell-box":
        assert (whole[:, :3].sum(1) > 0).mean() > 0.5
    one = np.zeros((1000, 4), F32)
    for k in range(8):
        tb.TraceRadiance(rays, 1, 2 + k, 16.0, settings=settings, out=one)
    assert same(one, whole)
    two = tb.TraceRadiance(rays, 3, 2, 16.0, settings=settings)
    tb.TraceRadiance(rays, 5, 5, 16.0, settings=settings, out=two)
    assert same(two, whole)
    monkeypatch.setenv("TB_RAD_MAX_PATHS", "3000")                    # 3 samples of the 1 000 rays per launch: 3 + 3 + 2
    cut = tb.TraceRadiance(rays, 8, 2, 16.0, settings=settings)
    assert tb.GetOption("last_radiance_launches") == 3 and same(cut, whole)


@gpu
@pytest.mark.parametrize("scene", ["cornell-box", "proc40k"])
def test_scheduling_does_not_show(rad_tb, settings, scene, monkeypatch):
    """4. Reversed and shuffled rays keep their values; both forms and a refilling grid of one workgroup give the same bytes, at every size."""
    import radiance_cases as rc
    tb = load(rad_tb, scene)
    info = tb.SceneInfo()
    all_rays = rc.random_rays(info.sceneMin[:], info.sceneMax[:], max(rc.SIZES), seed=43)
    shuffle = np.random.default_rng(44).permutation(max(rc.SIZES))
    for n in rc.SIZES:
        rays = all_rays[:n].copy()
        monkeypatch.setenv("TB_RAD_FORM", "0")
        plain = tb.TraceRadiance(rays, 2, 0, 16.0, settings=settings)
        assert tb.GetOption("last_radiance_form") == 0 and (plain[:, 3] == 2).all()
        assert same(tb.TraceRadiance(rays[::-1].copy(), 2, 0, 16.0, settings=settings)[::-1], plain)
        order = shuffle[shuffle < n]
        again = np.empty_like(plain); again[order] = tb.TraceRadiance(rays[order], 2, 0, 16.0, settings=settings)
        assert same(again, plain)
        monkeypatch.setenv("TB_RAD_FORM", "1")
        assert same(tb.TraceRadiance(rays, 2, 0, 16.0, settings=settings), plain), n
        assert tb.GetOption("last_radiance_form") == 1
        again[order] = tb.TraceRadiance(rays[order], 2, 0, 16.0, settings=settings)
        assert same(again, plain)
        monkeypatch.setenv("TB_RAD_GRID", "1")                        # one workgroup: every wave refills many times, across several chunks
        assert same(tb.TraceRadiance(rays, 2, 0, 16.0, settings=settings), plain), n
        assert tb.GetOption("last_radiance_form") == 1
        monkeypatch.delenv("TB_RAD_GRID")
    monkeypatch.delenv("TB_RAD_FORM")


@gpu
def test_known_answers(rad_tb, settings):
    """5. The light seen directly, a ray that leaves the box, MaxBounces 0, degenerate rays, the firefly clamp."""
    import radiance_cases as rc
    from tracerboy_amd import api
    tb = load(rad_tb, "cornell-box")
    known = known_rays(tb.HostSceneView(), tb.SceneInfo(), tb.GetCamera())
    S = 4
    got = tb.TraceRadiance(known.rays, S, 0, 16.0, settings=settings)
    assert tb.GetOption("last_radiance_variant") == 0                 # cornell-box under plain settings: the matte set
    assert same(got[0], np.append(rc.sequential_sum(known.emissive, S), F32(S)))
    assert same(got[1], F32([0, 0, 0, S]))
    none = copy.copy(settings); none.MaxBounces = 0
    assert same(tb.TraceRadiance(known.rays, S, 0, 16.0, settings=none), F32([[0, 0, 0, S]] * 2))
    clamp = copy.copy(settings); clamp.FireflyClampValue = 0.5 * float(known.emissive.max())
    capped = tb.TraceRadiance(known.rays, S, 0, 16.0, settings=clamp)
    assert tb.GetOption("last_radiance_variant") == 4                 # the clamp is a FEAT_EXT setting: the full set
    assert same(capped[0], np.append(rc.sequential_sum(np.minimum(known.emissive, F32(clamp.FireflyClampValue)), S), F32(S)))
    o = np.tile(known.rays["Origin"][0], (6, 1)); d = np.tile(known.rays["Direction"][0], (6, 1))
    d[0] = 0.0; d[1, 1] = np.nan; d[2, 0] = np.inf; o[3, 2] = np.nan; o[4, 0] = -np.inf            # ray 5 stays good
    rays = api.make_radiance_rays(o, d)
    for mode in (api.RADIANCE_RAY, api.RADIANCE_HEMISPHERE):
        got = tb.TraceRadiance(rays, S, 0, 16.0, mode=mode, settings=settings)
        assert same(got[:5], np.zeros((5, 4), F32)) and got[5, 3] == S
        kept = np.full((6, 4), 7.0, F32)
        tb.TraceRadiance(rays, S, 0, 16.0, mode=mode, settings=settings, out=kept)
        assert same(kept[:5], np.full((5, 4), 7.0, F32)) and kept[5, 3] == 7 + S


@gpu
def test_it_follows_a_moved_scene(built, settings):
    """6. After UpdatePositions + CommitGeometry (the emissive quad kept), frame 1's camera rays equal the oracle on the context's refreshed view."""
    import dynamic_cases as dc
    import oracle_lib as ol
    import radiance_cases as rc
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        tb.LoadScene(rc.SCENES["cornell-box"])
        view = tb.HostSceneView()
        pos = dc.positions_of(view)
        rays, adv = tb.MakeCameraRays(rc.W, rc.H, 1, settings=settings)
        before = tb.TraceRadiance(rays, 1, 1, adv, settings=settings)
        tb.UpdatePositions(dc.displaced(pos, 0.05, dc.DISPLACE_SEED, keep=dc.emissive_vertices(view))); tb.CommitGeometry()
        moved = tb.HostSceneView()
        want = ol.render(moved, tb.FrameConstants(rc.W, rc.H, 1, settings, 0.0), rc.W, rc.H, 1, first_frame=1)["output"].reshape(-1, 4)
        got = tb.TraceRadiance(rays, 1, 1, adv, settings=settings)
        assert same(got, want) and not same(got, before)


@gpu
def test_refusals_and_the_call_after_them(built, settings):
    """7. Every refusal of the list with its code, each followed by a correct answer from the same context."""
    import radiance_cases as rc
    from tracerboy_amd import _ctypes_abi as abi, api
    rays = api.make_radiance_rays(np.float32([[0, 1, 3]] * 65), np.float32([[0, 0, -1]] * 65))
    out = np.empty((65, 4), F32)
    vp = ctypes.c_void_p

    def raw(tb, call, n, r, o, s=None):
        return tb._L.tb_trace_radiance(tb._ctx, ctypes.byref(s) if s is not None else None, 0.0, ctypes.byref(call) if call is not None else None, n,
                                       r.ctypes.data_as(vp) if r is not None else None, o.ctypes.data_as(vp) if o is not None else None)

    def last_error(tb):
        return (tb._L.tb_last_error(tb._ctx) or b"").decode()

    call = lambda first=0, samples=1, advance=16.0, flags=0: abi.TbRadianceCall(first, samples, advance, flags)
    with api.TracerBoy(0) as tb:
        with pytest.raises(api.TracerBoyError) as e:
            tb.TraceRadiance(rays, settings=settings)
        assert e.value.code == -7                                     # TB_E_NO_SCENE
        with pytest.raises(api.TracerBoyError) as e:
            tb.MakeCameraRays(8, 8, 0, settings=settings)
        assert e.value.code == -7
        tb.LoadScene(rc.SCENES["cornell-box"])
        good = tb.TraceRadiance(rays, 2, 0, 16.0, settings=settings)
        assert (good[:, 3] == 2).all()
        refused = [(call(flags=0x400), 65, rays, out), (call(flags=2), 65, rays, out), (call(samples=0), 65, rays, out), (call(samples=(1 << 24) + 1), 65, rays, out),
                   (call(first=0xffffffff, samples=2), 65, rays, out), (call(), (1 << 31) + 1, rays, out), (call(), 65, None, out), (call(), 65, rays, None),
                   (None, 65, rays, out), (call(flags=api.RADIANCE_DEVICE), 65, rays, out)]     # host memory handed in as device memory
        for c, n, r, o in refused:
            assert raw(tb, c, n, r, o) == -1 and "tb_trace_radiance" in last_error(tb), last_error(tb)
            assert same(tb.TraceRadiance(rays, 2, 0, 16.0, settings=settings), good)
        assert raw(tb, call(), 0, None, None) == 0                   # n = 0: TB_OK, nothing launched
        realtime = copy.copy(settings); realtime.RenderModeRealTime = 1
        assert raw(tb, call(), 65, rays, out, realtime) == -6 and "real-time" in last_error(tb)
        assert same(tb.TraceRadiance(rays, 2, 0, 16.0, settings=settings), good)
        for filter_type in (1, 2):                                    # triangle, Gaussian: the record has no weight
            weighted = copy.copy(settings); weighted.FilterType = filter_type
            with pytest.raises(api.TracerBoyError) as e:
                tb.MakeCameraRays(8, 8, 0, settings=weighted)
            assert e.value.code == -6
        cam, adv = tb.MakeCameraRays(8, 8, 0, settings=settings)
        assert adv == 16.0 and (tb.TraceRadiance(cam, 1, 0, adv, settings=settings)[:, 3] == 1).all()
    with api.TracerBoy(devices=[0, 0]) as group:
        group.LoadScene(rc.SCENES["cornell-box"])
        with pytest.raises(api.TracerBoyError) as e:
            group.TraceRadiance(rays, settings=settings)
        assert e.value.code == -6 and "multi-device group" in str(e.value)
        with pytest.raises(api.TracerBoyError) as e:
            group.MakeCameraRays(8, 8, 0, settings=settings)
        assert e.value.code == -6
        group.Render(64, 48, 1, settings, 0.0)                       # the group itself goes on working
