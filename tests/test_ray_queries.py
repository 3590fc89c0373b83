"""Ray queries (include/tracerboy_hip.h tb_trace_rays): closest hits and any-hit occlusion of a caller's rays, on host arrays
and on device tensors.  The ray sets and the expected answers come from tests/ray_query_cases.py and the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

import ray_query_cases as rq
from conftest import ROOT

gpu = pytest.mark.gpu


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _header_struct_offsets(struct):
    """Field name -> byte offset of a typedef'd struct of tb_abi.h whose members are 4-byte scalars and arrays of them."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), _header("tb_abi.h"), re.S).group(1)
    offsets, at = {}, 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "uint32_t", "int32_t"), decl
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            offsets[m.group(1)] = at
            at += 4 * int(m.group(2) or 1)
    return offsets, at


def test_header_declares_the_call_and_both_structs():
    api_h = _header("tracerboy_hip.h")
    assert re.search(r"\bint\s+tb_trace_rays\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*,\s*const\s+TbQueryRay\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", api_h)
    for name, value in (("TB_RAYS_CLOSEST", "0u"), ("TB_RAYS_OCCLUDED", "1u"), ("TB_RAYS_DEVICE", "0x100u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), api_h), name
    abi_h = _header("tb_abi.h")
    assert re.search(r"#define\s+TB_QUERY_RAY_DISABLED\s+1u\b", abi_h)
    assert _header_struct_offsets("TbQueryRay")[1] == 32 and _header_struct_offsets("TbQueryHit")[1] == 48
    assert re.search(r"TB_STATIC_ASSERT\(sizeof\(TbQueryRay\) == 32", abi_h) and re.search(r"TB_STATIC_ASSERT\(sizeof\(TbQueryHit\) == 48", abi_h)


def test_library_exports_and_binds_the_call(built):
    from tracerboy_amd import api
    raw = ctypes.CDLL(api.LIB_PATH)
    bound = api.lib()
    assert hasattr(raw, "tb_trace_rays") and "tb_trace_rays" in bound._tb_exports
    assert bound.tb_trace_rays.argtypes == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    assert (api.RAYS_CLOSEST, api.RAYS_OCCLUDED, api.RAYS_DEVICE, api.QUERY_RAY_DISABLED) == (0, 1, 0x100, 1)


def test_struct_mirrors_match_the_header():
    from tracerboy_amd import _ctypes_abi as abi, api
    for struct, mirror, dtype in (("TbQueryRay", abi.TbQueryRay, api.QUERY_RAY_DTYPE), ("TbQueryHit", abi.TbQueryHit, api.QUERY_HIT_DTYPE)):
        offsets, size = _header_struct_offsets(struct)
        assert ctypes.sizeof(mirror) == size == dtype.itemsize
        assert {n: getattr(mirror, n).offset for n, _ in mirror._fields_} == offsets
        assert {n: dtype.fields[n][1] for n in dtype.names} == offsets
    assert ctypes.sizeof(abi.TbQueryRay) == 32 and ctypes.sizeof(abi.TbQueryHit) == 48


def test_make_query_rays_packs_what_it_is_given():
    from tracerboy_amd import api
    o = np.arange(12, dtype=np.float64).reshape(4, 3); d = -o
    r = api.make_query_rays(o, d)
    assert r.dtype == api.QUERY_RAY_DTYPE and r.shape == (4,) and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r["Origin"], o.astype(np.float32)) and np.array_equal(r["Direction"], d.astype(np.float32))
    assert np.isposinf(r["TMax"]).all() and not r["Flags"].any()
    r = api.make_query_rays(o, d, tmax=[1.0, 2.5, np.inf, np.nan], disabled=[False, True, False, True])
    assert np.array_equal(r["TMax"][:3], np.float32([1.0, 2.5, np.inf])) and np.isnan(r["TMax"][3])
    assert r["Flags"].tolist() == [0, 1, 0, 1]
    flat = r.view(np.float32).reshape(4, 8)                         # the (n, 8) float32 form of the same bytes
    assert np.array_equal(flat[:, 0:3], r["Origin"]) and np.array_equal(flat[:, 4:7], r["Direction"]) and flat[1, 3] == 2.5
    assert np.array_equal(flat[:, 7].view(np.uint32), r["Flags"])
    assert api.make_query_rays(o, d, tmax=3.0)["TMax"].tolist() == [3.0] * 4
    with pytest.raises(ValueError):
        api.make_query_rays(o, d[:3])
    with pytest.raises(ValueError):
        api.make_query_rays(o[:, :2], d[:, :2])


def test_trace_rays_refuses_wrong_arrays_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    good = api.make_query_rays(np.zeros((6, 3)), np.ones((6, 3)))
    wrong = {
        "dtype float64": np.zeros((6, 8), np.float64),
        "dtype int32": np.zeros((6, 8), np.int32),
        "shape (n, 7)": np.zeros((6, 7), np.float32),
        "shape (n,)": np.zeros(48, np.float32),
        "two dimensions of the structured dtype": np.zeros((2, 3), api.QUERY_RAY_DTYPE),
        "a non-contiguous float array": np.zeros((12, 8), np.float32)[::2],
        "a non-contiguous structured array": np.zeros(12, api.QUERY_RAY_DTYPE)[::2],
        "a list": [[0.0] * 8],
        "a tensor on the CPU": torch.zeros((6, 8), dtype=torch.float32),
        "a float64 tensor": torch.zeros((6, 8), dtype=torch.float64),
    }
    for what, rays in wrong.items():
        for mode in (api.RAYS_CLOSEST, api.RAYS_OCCLUDED):
            with pytest.raises(ValueError):
                tb.TraceRays(rays, mode)
                pytest.fail(what)
    for mode in (2, -1, api.RAYS_DEVICE, api.RAYS_OCCLUDED | api.RAYS_DEVICE, None):
        with pytest.raises(ValueError):
            tb.TraceRays(good, mode)
    with pytest.raises(AttributeError):                             # the good array gets past the checks, to the library this object lacks
        tb.TraceRays(good)


def test_generated_ray_sets_keep_clear_of_their_hit_distances(built, settings):
    """The occluded comparison leaves out rays with |t - TMax| <= 1e-4 t (ray_query_cases.near_tmax).  Counted here with the oracle alone, on
    host scenes: 0 of 4 608 / 4 676 / 4 676 / 4 676 / 4 573 rays (cornell, alpha0, alpha1, instanced, proc40k) -- the factors 0.5, 2 and 0.999 keep
    clear."""
    import oracle_lib as ol
    try:
        for name in rq.CASES:
            rays, oracle = rq.host_case(name, settings)
            assert 4000 < len(rays) < 5200
            assert int(rq.near_tmax(rays, oracle).sum()) == 0, name
            disabled = (rays["Flags"] & 1) != 0
            assert 0.07 < disabled.mean() < 0.13
            assert rq.expected_occluded(rays, oracle).sum() > 500 and (rq.expected_hits(rays, oracle)["T"] < 0).sum() > 500
    finally:
        ol.set_alpha_test(0)


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rq_tb(built):
    """A context of this module's own: the cases load scenes under options that the session's context must not keep."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    tb._rq_case = None
    yield tb
    tb.close()


_CASE_DATA = {}


def load_case(tb, name, settings):
    """The case's scene in the context (loaded under its options, which then go back to the defaults) and its rays and oracle answers, made once."""
    import oracle_lib as ol
    path, alpha, flatten = rq.CASES[name]
    if tb._rq_case != name:
        tb.SetOption("alpha_test", alpha); tb.SetOption("flatten_instances", flatten)
        try:                                                         # finalizeScene takes alpha_test into the device scene, as tb_trace_closest reads it
            tb.LoadScene(path) if path else tb.LoadProcedural(0, rq.PROC_TRIANGLES, rq.PROC_SEED)
        finally:
            tb.SetOption("alpha_test", 0); tb.SetOption("flatten_instances", 1)
        tb._rq_case = name
    if name not in _CASE_DATA:
        ol.set_alpha_test(alpha)
        try:
            info = tb.SceneInfo()
            _CASE_DATA[name] = rq.build_rays(tb.HostSceneView(), tb.FrameConstants(64, 48, 0, settings, 0.0), tb.GetCamera().LensHeight,
                                             info.sceneMin[:], info.sceneMax[:])
        finally:
            ol.set_alpha_test(0)
    return _CASE_DATA[name]


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@gpu
@pytest.mark.parametrize("case", list(rq.CASES))
def test_closest_mode_on_host_arrays_is_trace_closest_bit_for_bit(rq_tb, settings, case):
    """1. Every field of every record: the oracle's hit (and TraceClosest's) where the ray is traced and t < TMax, the miss record elsewhere."""
    from tracerboy_amd import api
    rays, oracle = load_case(rq_tb, case, settings)
    assert rq_tb.SceneInfo().numTriangles > 0 and (rq_tb.HostSceneView().numInstances > 0) == (case == "instanced")
    got = rq_tb.TraceRays(rays, api.RAYS_CLOSEST)
    assert got.dtype == api.QUERY_HIT_DTYPE and got.shape == rays.shape
    hook = rq_tb.TraceClosest(rays["Origin"], rays["Direction"])
    for k in ("t", "bary", "normal", "uv"):
        assert np.array_equal(hook[k].view(np.uint32), oracle[k].view(np.uint32)), k
    for k in ("material", "prim", "geom"):
        assert np.array_equal(hook[k], oracle[k]), k
    want = rq.expected_hits(rays, oracle)
    for field in api.QUERY_HIT_DTYPE.names:
        assert same_bytes(got[field], want[field]), field
    uncut = rq.traced(rays) & ~(rays["TMax"] < rq.MAX_T)             # the renderer's ray: the hook's own record
    assert uncut.sum() > 2000 and np.array_equal(got["T"][uncut].view(np.uint32), hook["t"][uncut].view(np.uint32))
    cut = rq.traced(rays) & (oracle["t"] >= 0) & (oracle["t"] >= rays["TMax"])
    assert cut.sum() >= 50 and (got["T"][cut] == -1).all()          # at least the traced ones of the 96 copies with TMax = 0.5 t
    disabled = (rays["Flags"] & 1) != 0
    assert disabled.sum() > 300 and (got["T"][disabled] == -1).all() and (got["Material"][disabled] == -1).all()
    as_floats = rq_tb.TraceRays(rays.view(np.float32).reshape(-1, 8), api.RAYS_CLOSEST)      # the (n, 8) float32 form of the same rays
    assert same_bytes(as_floats, got)


@gpu
@pytest.mark.parametrize("case", list(rq.CASES))
def test_occluded_mode_agrees_with_the_oracle(rq_tb, settings, case):
    """2. occluded[i] == (t_oracle >= 0 and t_oracle < min(TMax, MAX_T)) outside |t_oracle - TMax| <= 1e-4 t_oracle; those rays are at most 0.1 %
    of a set -- counted with the oracle alone before any GPU run: 0 in every case (test_generated_ray_sets_keep_clear_of_their_hit_distances)."""
    from tracerboy_amd import api
    rays, oracle = load_case(rq_tb, case, settings)
    got = rq_tb.TraceRays(rays, api.RAYS_OCCLUDED)
    assert got.dtype == np.uint8 and got.shape == rays.shape and set(np.unique(got)) <= {0, 1}
    near = rq.near_tmax(rays, oracle)
    assert near.sum() <= 0.001 * len(rays)
    want = rq.expected_occluded(rays, oracle)
    bad = np.flatnonzero((got != want) & ~near)
    assert bad.size == 0, (bad[:10], rays[bad[:10]], oracle["t"][bad[:10]])
    assert want.sum() > 1000 and (want == 0).sum() > 1000
    assert not got[(rays["Flags"] & 1) != 0].any()


@gpu
def test_occluded_mode_passes_through_transparent_texels(rq_tb, settings):
    """2, alpha-card with alpha_test = 1: a ray through a transparent texel of the card is not occluded up to what lies behind it, a ray through an
    opaque texel is.  Which is which: the context's own TraceClosest with the filter off and on."""
    from tracerboy_amd import api
    rays, _ = load_case(rq_tb, "alpha0", settings)
    o, d = rays["Origin"][:3072], rays["Direction"][:3072]          # the camera rays
    off = rq_tb.TraceClosest(o, d)
    load_case(rq_tb, "alpha1", settings)
    on = rq_tb.TraceClosest(o, d)
    through = (off["t"] > 0) & (on["t"] != off["t"])                # the filter rejected the first hit: a transparent texel
    card = np.unique(off["geom"][through])
    opaque = (off["t"] > 0) & np.isin(off["geom"], card) & (on["t"] == off["t"]) & (on["prim"] == off["prim"])
    assert through.sum() > 20 and opaque.sum() > 20
    behind = np.where(through & (on["t"] > 0), on["t"], np.float32(3.0) * off["t"])    # what the ray meets next; an opaque texel: 2 t in all
    tmax = (off["t"] + np.float32(0.5) * (behind - off["t"])).astype(np.float32)     # past the card, short of what lies behind it
    got = rq_tb.TraceRays(api.make_query_rays(o, d, tmax), api.RAYS_OCCLUDED)
    assert not got[through].any() and got[opaque].all()
    assert rq_tb.TraceRays(api.make_query_rays(o[through], d[through], np.float32(0.5) * off["t"][through]), api.RAYS_OCCLUDED).sum() == 0


@gpu
@pytest.mark.parametrize("case", ["cornell", "proc40k"])
def test_answers_do_not_depend_on_scheduling_or_size(rq_tb, settings, case):
    """3. n in {0, 1, 63, 64, 65, 257}, and 2^17 rays whose walks end many steps apart -- 512 pools of 256 rays, so a wave of the refilling form
    (proc40k; cornell runs one ray per lane) that gets any refills four times and more: the same answers per ray in reversed and in shuffled order,
    in both modes; two calls in a row give the same bytes."""
    import oracle_lib as ol
    from tracerboy_amd import api
    rays, oracle = load_case(rq_tb, case, settings)
    assert (rq_tb.SceneInfo().numTriangles >= 32768) == (case == "proc40k")
    full = {m: rq_tb.TraceRays(rays, m) for m in (api.RAYS_CLOSEST, api.RAYS_OCCLUDED)}
    for n in (0, 1, 63, 64, 65, 257):
        for m in full:
            got = rq_tb.TraceRays(rays[:n].copy(), m)
            assert got.shape == (n,) and same_bytes(got, full[m][:n]), (n, m)
    info = rq_tb.SceneInfo()
    big = rq.scheduling_rays(info.sceneMin[:], info.sceneMax[:])
    n = len(big)
    assert n == 1 << 17
    ref = ol.trace_closest(rq_tb.HostSceneView(), big["Origin"], big["Direction"])
    want = {api.RAYS_CLOSEST: rq.expected_hits(big, ref), api.RAYS_OCCLUDED: rq.expected_occluded(big, ref)}
    assert 0.1 < want[api.RAYS_OCCLUDED].mean() < 0.9 and rq.near_tmax(big, ref).sum() <= 0.001 * n
    shuffle = np.random.default_rng(22).permutation(n)
    for m in full:
        first = rq_tb.TraceRays(big, m)
        ok = ~rq.near_tmax(big, ref) if m == api.RAYS_OCCLUDED else np.ones(n, bool)
        assert same_bytes(first[ok], want[m][ok]), m
        assert same_bytes(rq_tb.TraceRays(big, m), first), m
        assert same_bytes(rq_tb.TraceRays(big[::-1].copy(), m)[::-1], first), m
        again = np.empty_like(first); again[shuffle] = rq_tb.TraceRays(big[shuffle], m)
        assert same_bytes(again, first), m


@gpu
@pytest.mark.parametrize("case", ["cornell", "instanced", "proc40k"])
def test_device_tensors_give_the_host_path_bytes_and_hold_nothing(rq_tb, settings, case):
    """4. The same rays as a torch tensor on the device: the same bytes in both modes, zero copy; wrong tensors are refused in Python; the call
    leaves nothing behind but, once, the work counter of the any-hit walk's refilling form (proc40k), neither in torch's allocator nor in the
    context."""
    import torch
    from test_context_lifetime import live
    from tracerboy_amd import api
    rays, _ = load_case(rq_tb, case, settings)
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
    rq_tb.TraceRays(dev, api.RAYS_OCCLUDED)                          # the counter exists from here on
    for mode in (api.RAYS_CLOSEST, api.RAYS_OCCLUDED):
        host = rq_tb.TraceRays(rays, mode)
        torch.cuda.synchronize()
        held, mine = torch.cuda.memory_allocated(0), live(rq_tb)
        out = rq_tb.TraceRays(dev, mode)
        assert live(rq_tb) == mine                                  # no context buffer made, none left
        assert out.device == dev.device and out.is_contiguous()
        if mode == api.RAYS_CLOSEST:
            assert out.dtype == torch.float32 and tuple(out.shape) == (len(rays), 12)
            assert int(out.view(torch.int32)[:, 5].min()) == -1     # Material of the misses, read as the issue says
        else:
            assert out.dtype == torch.uint8 and tuple(out.shape) == (len(rays),)
        assert 0 < torch.cuda.memory_allocated(0) - held <= out.numel() * out.element_size() + 512      # the result alone, rounded up by torch
        got = out.cpu().numpy()
        del out
        assert torch.cuda.memory_allocated(0) == held
        assert np.array_equal(got.view(np.uint8).ravel(), host.view(np.uint8).ravel()), mode
        assert same_bytes(rq_tb.TraceRays(dev[:0], mode).cpu().numpy().ravel(), got[:0].ravel())          # n = 0: nothing launched
    for wrong in (dev.cpu(), dev.double(), dev[::2], dev[:, :7], dev.view(-1)):
        with pytest.raises(ValueError):
            rq_tb.TraceRays(wrong, api.RAYS_CLOSEST)
    assert same_bytes(rq_tb.TraceRays(dev, api.RAYS_OCCLUDED).cpu().numpy(), rq_tb.TraceRays(rays, api.RAYS_OCCLUDED))    # and it still works


@gpu
def test_the_work_counter_goes_with_the_context(gpu_tb, settings):
    """4. A fresh context: closest mode holds nothing, nor does occluded mode on a small scene (one ray per lane); on a scene of the refilling
    form the first any-hit launch makes the counter, later ones reuse it, and tb_destroy gives it back with everything else."""
    import torch
    from test_context_lifetime import live
    from tracerboy_amd import api
    rays = api.make_query_rays(np.float32([[0, 1, 3]] * 300), np.float32([[0, 0, -1]] * 300))
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
    before = live(gpu_tb)
    with api.TracerBoy(0) as tb:
        tb.LoadScene(rq.CASES["cornell"][0])
        loaded = live(gpu_tb)
        tb.TraceRays(dev, api.RAYS_CLOSEST); tb.TraceRays(rays, api.RAYS_CLOSEST); tb.TraceRays(dev, api.RAYS_OCCLUDED)
        assert live(gpu_tb) == loaded
        tb.LoadProcedural(0, rq.PROC_TRIANGLES, rq.PROC_SEED)
        loaded = live(gpu_tb)
        tb.TraceRays(dev, api.RAYS_CLOSEST)
        assert live(gpu_tb) == loaded
        tb.TraceRays(dev, api.RAYS_OCCLUDED)
        counter = live(gpu_tb) - loaded
        assert 4 <= counter <= 256
        tb.TraceRays(dev, api.RAYS_OCCLUDED); tb.TraceRays(rays, api.RAYS_OCCLUDED)
        assert live(gpu_tb) == loaded + counter
    assert live(gpu_tb) == before


@gpu
def test_refusals_and_the_call_after_them(gpu_tb, settings):
    """5. No scene, a group's context, unknown flag bits and modes, too many rays, null pointers: each with its code, and the next valid call
    works.  (A peer handle is never handed out; TB_REFUSE_PEER refuses it here as everywhere.)"""
    from tracerboy_amd import api
    rays = api.make_query_rays(np.float32([[0, 1, 3]] * 65), np.float32([[0, 0, -1]] * 65))
    out = np.empty(65, api.QUERY_HIT_DTYPE)

    def raw(tb, mode, n, r, o):
        return tb._L.tb_trace_rays(tb._ctx, mode, n, r.ctypes.data_as(ctypes.c_void_p) if r is not None else None,
                                   o.ctypes.data_as(ctypes.c_void_p) if o is not None else None)

    def last_error(tb):
        return (tb._L.tb_last_error(tb._ctx) or b"").decode()

    with api.TracerBoy(0) as tb:
        with pytest.raises(api.TracerBoyError) as e:
            tb.TraceRays(rays)
        assert e.value.code == -7                                   # TB_E_NO_SCENE
        tb.LoadScene(rq.CASES["cornell"][0])
        good = tb.TraceRays(rays)
        assert (good["T"] > 0).all()
        for mode in (0x200, 0x400 | api.RAYS_OCCLUDED, 0x80000000, 2, 0xff):
            assert raw(tb, mode, 65, rays, out) == -1 and "tb_trace_rays" in last_error(tb), hex(mode)
        assert raw(tb, api.RAYS_CLOSEST, (1 << 31) + 1, None, None) == -1 and "2^31" in last_error(tb)
        assert raw(tb, api.RAYS_CLOSEST, 65, None, out) == -1 and raw(tb, api.RAYS_OCCLUDED, 65, rays, None) == -1 and "null" in last_error(tb)
        assert raw(tb, api.RAYS_OCCLUDED, 0, None, None) == 0       # n = 0: TB_OK, nothing launched
        assert same_bytes(tb.TraceRays(rays), good)
        assert tb.TraceRays(rays, api.RAYS_OCCLUDED).all()
    with api.TracerBoy(devices=[0, 0]) as group:
        group.LoadScene(rq.CASES["cornell"][0])
        with pytest.raises(api.TracerBoyError) as e:
            group.TraceRays(rays)
        assert e.value.code == -6 and "multi-device group" in str(e.value)     # TB_E_UNSUPPORTED, the other stages' wording
        group.Render(64, 48, 1, settings, 0.0)                      # the group itself goes on working
