"""Lightmap baking (include/tracerboy_hip.h tb_bake_lightmap .. tb_run_bake_dilate): a UV atlas rasterised, traced, resolved
and dilated on the device.  The expected values are tests/bake_cases.py's numpy restatement of kernels/bake_launch.h, hand-counted cases, and
TraceRadiance (which tests/test_radiance_queries.py holds to the oracle); every comparison is on bits."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, CORNELL

gpu = pytest.mark.gpu
F32 = np.float32
NONE = 0xffffffff


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_bytes(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def test_header_exports_bindings_and_methods_agree(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    h = _header("tracerboy_hip.h")
    assert re.search(r"\bint\s+tb_bake_lightmap\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*const\s+tb_output_settings\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*const\s+tb_bake_call\s*\*"
                     r"\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_read_bake\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*TbRadianceRay\s*\*\s*\w+\s*,\s*TbBakeTexel\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_run_bake_raster\s*\(\s*tb_context\s*\*\s*\w+\s*,(\s*uint32_t\s+\w+\s*,){3}(\s*const\s+float\s*\*\s*\w+\s*,){3}\s*uint32_t\s+\w+\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*TbRadianceRay\s*\*\s*\w+\s*,\s*TbBakeTexel\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_run_bake_dilate\s*\(\s*tb_context\s*\*\s*\w+\s*,(\s*uint32_t\s+\w+\s*,){3}\s*const\s+float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_bake_refusal\s*\(\s*const\s+tb_bake_call\s*\*\s*\w+\s*,(\s*const\s+void\s*\*\s*\w+\s*,){2}\s*char\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", h)
    for name, value in (("TB_BAKE_DEVICE", "0x100u"), ("TB_BAKE_ACCUMULATE", "0x200u"), ("TB_RAYS_DEVICE", "0x100u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), h), name
    assert (api.BAKE_DEVICE, api.BAKE_ACCUMULATE) == (0x100, 0x200)
    call = re.search(r"typedef\s+struct\s+tb_bake_call\s*\{\s*uint32_t\s+([\w\s,]+);\s*\}\s*tb_bake_call\s*;", h).group(1)
    assert [n.strip() for n in call.split(",")] == [n for n, _ in abi.tb_bake_call._fields_] == ["width", "height", "first_sample", "num_samples", "dilate_passes", "flags"]
    assert ctypes.sizeof(abi.tb_bake_call) == 24
    texel = re.search(r"typedef\s+struct\s+TbBakeTexel\s*\{\s*uint32_t\s+triangle\s*,\s*cls\s*;\s*float\s+w0\s*,\s*w1\s*;\s*\}\s*TbBakeTexel\s*;", _header("tb_abi.h"))
    assert texel and re.search(r"sizeof\s*\(\s*TbBakeTexel\s*\)\s*==\s*16", _header("tb_abi.h"))
    assert ctypes.sizeof(abi.TbBakeTexel) == 16 and api.BAKE_TEXEL_DTYPE.itemsize == 16
    assert {n: getattr(abi.TbBakeTexel, n).offset for n, _ in abi.TbBakeTexel._fields_} == {n: api.BAKE_TEXEL_DTYPE.fields[n][1] for n in api.BAKE_TEXEL_DTYPE.names} \
        == {"triangle": 0, "cls": 4, "w0": 8, "w1": 12}
    raw = ctypes.CDLL(api.LIB_PATH); bound = api.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in ("tb_bake_lightmap", "tb_bake_refusal", "tb_read_bake", "tb_run_bake_raster", "tb_run_bake_dilate"):
        assert hasattr(raw, name) and name in bound._tb_exports, name
    assert bound.tb_bake_lightmap.argtypes == [vp, ctypes.POINTER(abi.tb_output_settings), ctypes.c_float, ctypes.POINTER(abi.tb_bake_call), vp, vp]
    assert bound.tb_read_bake.argtypes == [vp, vp, vp, vp]
    assert bound.tb_run_bake_raster.argtypes == [vp, u32, u32, u32, vp, vp, vp, u32, vp, vp, vp]
    assert bound.tb_run_bake_dilate.argtypes == [vp, u32, u32, u32, vp, vp]
    for m in ("BakeLightmap", "ReadBake", "RunBakeRaster", "RunBakeDilate"):
        assert callable(getattr(api.TracerBoy, m)), m
    assert callable(api.BakeRefusal)


def test_the_refusal_table(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    call = lambda w=16, h=8, first=0, samples=1, dilate=2, flags=0: abi.tb_bake_call(w, h, first, samples, dilate, flags)
    A = 0x10000                                                       # any aligned non-null address: the function compares, it does not read
    assert api.BakeRefusal(call(), A, A) is None
    assert api.BakeRefusal(call(), 0, A) is None                      # no UVs: the scene's own
    assert api.BakeRefusal(call(w=8192, h=8192, samples=1 << 24, first=(1 << 32) - (1 << 24), dilate=16, flags=api.BAKE_DEVICE | api.BAKE_ACCUMULATE), A, A) is None
    assert api.BakeRefusal(call(dilate=0), A + 2, A + 4) is None      # host arrays need no alignment
    table = [
        (None, A, A, "null call"), (call(w=0), A, A, "is 0"), (call(h=0), A, A, "is 0"), (call(w=8193), A, A, "8192"), (call(h=1 << 20), A, A, "8192"),
        (call(flags=1), A, A, "flag"), (call(flags=0x400), A, A, "flag"), (call(flags=0x80000000), A, A, "flag"),
        (call(samples=0), A, A, "num_samples"), (call(samples=(1 << 24) + 1), A, A, "2^24"), (call(first=0xffffffff, samples=2), A, A, "2^32"),
        (call(dilate=17), A, A, "16"), (call(), A, 0, "null"), (call(flags=api.BAKE_DEVICE), A, A + 8, "aligned"), (call(flags=api.BAKE_DEVICE), A + 2, A, "aligned"),
    ]
    for c, u, o, word in table:
        why = api.BakeRefusal(c, u, o)
        assert why is not None and word in why, (word, why)


def test_wrong_inputs_are_refused_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    uv = np.zeros((6, 2), F32)
    for kw in (dict(width=0), dict(width=8193), dict(height=0), dict(height=2.0), dict(samples=0), dict(samples=(1 << 24) + 1), dict(first_sample=-1),
               dict(first_sample=(1 << 32) - 1, samples=2), dict(dilate=-1), dict(dilate=17), dict(dilate=True), dict(accumulate=1),
               dict(uv=np.zeros((6, 2), np.float64)), dict(uv=np.zeros((6, 3), F32)), dict(uv=np.zeros(12, F32)), dict(uv=np.zeros((12, 2), F32)[::2]),
               dict(uv=[[0.0, 0.0]]), dict(uv=torch.zeros((6, 2), dtype=torch.float32)), dict(uv=torch.zeros((6, 2), dtype=torch.float64)),
               dict(out=np.zeros((8, 16, 4), np.float64)), dict(out=np.zeros((16, 8, 4), F32)), dict(out=np.zeros((8, 32, 4), F32)[:, ::2]),
               dict(out=torch.zeros((8, 16, 4), dtype=torch.float32)), dict(uv=uv, out=torch.zeros((8, 16, 4), dtype=torch.float32))):
        args = dict(width=16, height=8, samples=4); args.update(kw)
        with pytest.raises(ValueError):
            tb.BakeLightmap(**args)
            pytest.fail(str(kw))
    for args in ((0, 8, uv, uv, uv, [[0, 1, 2]]), (8, 8193, uv, uv, uv, [[0, 1, 2]])):
        with pytest.raises(ValueError):
            tb.RunBakeRaster(*args)
    with pytest.raises(ValueError):
        tb.RunBakeRaster(8, 8, np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 2)), [[0, 1, 3]])
    with pytest.raises(ValueError):
        tb.RunBakeRaster(8, 8, np.zeros((3, 3)), np.zeros((2, 3)), np.zeros((3, 2)), [[0, 1, 2]])
    for args in ((np.zeros((4, 4, 3), F32), 1), (np.zeros((4, 4, 4), F32), 17), (np.zeros((4, 4, 4), F32), -1), (np.zeros((0, 4, 4), F32), 1)):
        with pytest.raises(ValueError):
            tb.RunBakeDilate(*args)
    with pytest.raises(AttributeError):                               # good arguments get past the checks, to the library this object lacks
        tb.BakeLightmap(16, 8, 4, first_sample=3, dilate=0, out=np.zeros((8, 16, 4), F32))


def test_the_restatement_gives_the_hand_counted_cases():
    import bake_cases as bc
    covered = lambda case, W=8, H=8: bc.cover(W, H, case[2], case[3])
    # a right triangle (0,0) (4,0) (0,4): its centres are the 10 texels with x + y <= 3; the mirror winding covers the same
    ys, xs = np.mgrid[0:8, 0:8]
    for case in (bc.hand_right_triangle(), bc.mirrored(bc.hand_right_triangle())):
        keys = covered(case)
        centre = keys == 0                                            # class 0, triangle 0
        assert centre.sum() == 10 and np.array_equal(centre, xs + ys <= 3)
        edge_texels = keys == np.uint64(1 << 32)
        assert np.array_equal(edge_texels, (xs + ys == 4) & (xs <= 4) & (ys <= 4)) # the hypotenuse's texels, within the box; nothing else
        assert ((keys == bc.NO_KEY) | centre | edge_texels).all()
    a, b = bc.texels(8, 8, *bc.hand_right_triangle()), bc.texels(8, 8, *bc.mirrored(bc.hand_right_triangle()))
    assert same_bytes(a[0], b[0]) and np.array_equal(a[1]["triangle"], b[1]["triangle"]) and same(a[1]["w0"], b[1]["w0"])
    # two triangles sharing the diagonal of a 6 x 6 quad: every texel of the quad is a centre hit, the diagonal's go to triangle 0
    keys = covered(bc.hand_quad())
    assert (keys[:6, :6] >> np.uint64(32) == 0).all()
    assert all(keys[i, i] == 0 for i in range(6)) and keys[1, 4] == 0 and keys[4, 1] == 1
    assert (keys[6:, :] != 0).all() and (keys[:, 6:] != 0).all()
    # area 0 and a NaN UV cover nothing
    assert (covered(bc.hand_degenerate()) == bc.NO_KEY).all()
    rays, rec = bc.texels(8, 8, *bc.hand_degenerate())
    assert (rec["triangle"] == NONE).all() and not rays.view(F32).any()
    # a 0.2-texel triangle inside texel (2, 3): that texel alone, class 1, weights inside the triangle
    keys = covered(bc.hand_small())
    assert (keys != bc.NO_KEY).sum() == 1 and keys[3, 2] == np.uint64(1 << 32)
    rays, rec = bc.texels(8, 8, *bc.hand_small())
    t = rec[3, 2]
    w2 = F32(1) - t["w0"] - t["w1"]
    assert t["triangle"] == 0 and t["cls"] == 1 and t["w0"] >= 0 and t["w1"] >= 0 and w2 >= -np.spacing(F32(1))
    assert abs(float(t["w0"]) + float(t["w1"]) + float(max(w2, 0)) - 1.0) <= float(np.spacing(F32(1)))
    assert rays[3, 2]["SeedX"] == 2 and rays[3, 2]["SeedY"] == 3 and abs(np.linalg.norm(rays[3, 2]["Direction"]) - 1) < 1e-6
    # tile counts: what bake_cover is launched over
    assert bc.tile_counts(67, 33, *bc.skewed(67, 33)[2:])[-2:].tolist() == [45, 45] and bc.tile_counts(8, 8, *bc.hand_degenerate()[2:]).tolist() == [0, 0]
    # dilation of one lit texel in a 5 x 5 atlas
    img = np.zeros((5, 5, 4), F32); img[2, 2] = [3, 5, 7, 1]
    one, two = bc.dilate(img, 1), bc.dilate(img, 2)
    ring = np.zeros((5, 5), bool); ring[1:4, 1:4] = True; ring[2, 2] = False
    assert (one[ring, 3] == 0.5).all() and (one[ring, :3] == [3, 5, 7]).all() and not one[~ring & ~(img[..., 3] > 0)].any() and same(one[2, 2], img[2, 2])
    outer = ~ring; outer[2, 2] = False
    assert (two[outer, 3] == 0.25).all() and (two[ring] == one[ring]).all() and (two[outer, :3] == [3, 5, 7]).all()
    assert same(bc.dilate(img, 0), img)
    # resolve: pi * sum / count on covered texels with a count
    rec = np.zeros((1, 3), bc.api.BAKE_TEXEL_DTYPE); rec["triangle"] = [[0, NONE, 5]]
    sums = np.array([[[1, 2, 3, 4], [1, 1, 1, 4], [1, 1, 1, 0]]], F32)
    got = bc.resolve(rec, sums)
    assert same(got[0, 0], [bc.PI * F32(1) / F32(4), bc.PI * F32(2) / F32(4), bc.PI * F32(3) / F32(4), 1]) and not got[0, 1:].any()


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def bake_tb(built):
    """A context of this module's own: the cases load scenes and move them."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    tb._bake_scene = None
    yield tb
    tb.close()


_host = {}


def host_arrays(name):
    """The scene's triangles in their own numbering and its positions, from a host-only load."""
    import bake_cases as bc
    from tracerboy_amd import api
    if name not in _host:
        hs = api.HostScene(procedural=(0, bc.PROC_TRIANGLES, bc.PROC_SEED)) if name == "proc40k" else api.HostScene(SCENES[name])
        t = hs.triangles()
        _host[name] = Bag(tri=t["tri_vertex_index"], positions=t["positions"], geometry=t["tri_geometry"])
        hs.close()
    return _host[name]


def _scenes():
    import bake_cases as bc
    return {"cornell-box": CORNELL, "material-maps": bc.MATERIAL_MAPS, "tri1": os.path.join(bc.DYNAMIC, "tri1.pbrt"), "tri3": os.path.join(bc.DYNAMIC, "tri3.pbrt")}


SCENES = _scenes()


def load(tb, name, fresh=False):
    import bake_cases as bc
    if tb._bake_scene != name or fresh:
        tb.LoadProcedural(0, bc.PROC_TRIANGLES, bc.PROC_SEED) if name == "proc40k" else tb.LoadScene(SCENES[name])
        tb._bake_scene = name
    return tb


def atlas_of(tb, name):
    import bake_cases as bc
    view = tb.HostSceneView()
    return bc.planar_atlas(host_arrays(name).positions, bc.geometry_ranges(view))


RASTER_SIZES = [(1, 1), (7, 5), (64, 64), (67, 33)]


def raster_sets(W, H):
    import bake_cases as bc
    rnd = bc.random_triangles()
    return {"hand": [bc.hand_right_triangle(W, H), bc.mirrored(bc.hand_right_triangle(W, H)), bc.hand_quad(W, H), bc.hand_degenerate(W, H), bc.hand_small(W, H)],
            "random": [rnd], "sparse": [bc.random_triangles(60, seed=8, large=0.0)], "mirrored": [bc.mirrored(rnd)], "skewed": [bc.skewed(W, H)], "zero-normals": [bc.zero_normals(rnd)],
            "collapsed": [bc.collapsed_positions(rnd)]}


@gpu
@pytest.mark.parametrize("size", RASTER_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_rasteriser_is_the_restatement(gpu_tb, size):
    """1. RunBakeRaster against bake_cases.texels, all bytes; both windings, the reversed order, the same input twice."""
    import bake_cases as bc
    W, H = size
    sets = raster_sets(W, H)
    for name, cases in sets.items():
        for case in cases:
            rays, rec = gpu_tb.RunBakeRaster(W, H, *case)
            want_rays, want_rec = bc.texels(W, H, *case)
            assert same_bytes(rec, want_rec), (name, size, np.argwhere(rec != want_rec)[:4])
            assert same_bytes(rays, want_rays), (name, size, np.argwhere(rays != want_rays)[:4])
    rnd = sets["random"][0]
    rays, rec = gpu_tb.RunBakeRaster(W, H, *rnd)
    again = gpu_tb.RunBakeRaster(W, H, *rnd)
    assert same_bytes(again[0], rays) and same_bytes(again[1], rec)
    assert (rec["triangle"] != NONE).any()
    if W >= 64:                                                       # (on the small atlases 300 triangles cover every centre)
        assert ((rec["cls"] == 1) & (rec["triangle"] != NONE)).any()
        sparse = gpu_tb.RunBakeRaster(W, H, *sets["sparse"][0])[1]    # gutters, and edge texels by the dozen
        assert (sparse["triangle"] == NONE).any() and ((sparse["cls"] == 1) & (sparse["triangle"] != NONE)).sum() > 20
    m_rays, m_rec = gpu_tb.RunBakeRaster(W, H, *sets["mirrored"][0])  # the other winding: the same owners and the same rays; w1 is now the other vertex's
    assert np.array_equal(m_rec["triangle"], rec["triangle"]) and np.array_equal(m_rec["cls"], rec["cls"]) and same(m_rec["w0"], rec["w0"]) and same_bytes(m_rays, rays)
    r_rec = gpu_tb.RunBakeRaster(W, H, *bc.reversed_order(rnd))[1]    # the reversed order: other winners, the same mask
    assert np.array_equal(r_rec["triangle"] != NONE, rec["triangle"] != NONE)
    zero = gpu_tb.RunBakeRaster(W, H, *sets["zero-normals"][0])       # the geometric normal stands in: the plane's, unit length
    assert np.array_equal(zero[1]["triangle"], rec["triangle"])
    n = zero[0]["Direction"][zero[1]["triangle"] != NONE]
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-5)
    gone = gpu_tb.RunBakeRaster(W, H, *sets["collapsed"][0])[1]       # no direction can be made: those texels have no triangle
    lost = (rec["triangle"] != NONE) & (rec["triangle"] % 2 == 0)
    assert (gone["triangle"][lost] == NONE).all() and np.array_equal(gone["triangle"][~lost], rec["triangle"][~lost])


@gpu
@pytest.mark.parametrize("size", [(1, 1), (7, 5), (67, 33)], ids=lambda s: "%dx%d" % s)
def test_the_fill_passes_are_the_restatement(gpu_tb, size):
    """2. RunBakeDilate against bake_cases.dilate: seeded masks, an empty atlas, a full one; passes 0, 1, 3, 16."""
    import bake_cases as bc
    W, H = size
    rng = np.random.default_rng(9)
    base = rng.uniform(0, 4, (H, W, 4)).astype(F32)
    pictures = []
    for share in (0.0, 0.05, 0.5, 1.0):
        img = base.copy(); img[..., 3] = np.where(rng.random((H, W)) < share, 1, 0)
        if share == 0.0 or share == 1.0:
            img[..., 3] = share
        pictures.append(img)
    for img in pictures:
        for passes in (0, 1, 3, 16):
            got = gpu_tb.RunBakeDilate(img, passes)
            assert same(got, bc.dilate(img, passes)), (size, passes)
    assert same(gpu_tb.RunBakeDilate(pictures[0], 16), pictures[0]) and same(gpu_tb.RunBakeDilate(pictures[3], 16), pictures[3])


@gpu
@pytest.mark.parametrize("scene", ["cornell-box", "proc40k"])
def test_a_whole_bake_is_raster_query_resolve_and_fill(bake_tb, settings, scene):
    """3. rays and texels = the restatement on the host's arrays; sums = TraceRadiance of those rays; picture = restated resolve + fill; the same
    through device tensors; last_bake_covered."""
    import bake_cases as bc
    import torch
    from tracerboy_amd import api
    tb = load(bake_tb, scene)
    host = host_arrays(scene)
    W, H, S = bc.ATLAS_W, bc.ATLAS_H, bc.ATLAS_SAMPLES
    uv = atlas_of(tb, scene)
    records = bc.vertex_records(tb.HostSceneView())
    picture = tb.BakeLightmap(W, H, S, uv=uv, settings=settings)
    rays, rec, sums = tb.ReadBake()
    want_rays, want_rec = bc.texels(W, H, host.positions, records[:, 0:3], uv, host.tri)
    assert same_bytes(rec, want_rec), np.argwhere(rec != want_rec)[:4]
    assert same_bytes(rays, want_rays), np.argwhere(rays != want_rays)[:4]
    mask = rec["triangle"] != NONE
    assert tb.GetOption("last_bake_covered") == mask.sum() > 0 and (rec["cls"][mask] == 1).any()
    traced = tb.TraceRadiance(rays.reshape(-1), S, 0, 0.0, mode=api.RADIANCE_HEMISPHERE, settings=settings)
    assert same(sums.reshape(-1, 4), traced) and not sums[~mask].any() and (sums[mask][:, 3] <= S).all() and sums[mask][:, 3].any()
    assert same(picture, bc.dilate(bc.resolve(rec, sums), 2))
    assert (picture[mask][:, 3] == 1).all() and set(np.unique(picture[~mask][:, 3]).tolist()) <= {0.0, 0.5, 0.25}
    dev_uv = torch.from_numpy(uv).to("cuda:0")
    dev = tb.BakeLightmap(W, H, S, uv=dev_uv, settings=settings)
    assert isinstance(dev, torch.Tensor) and dev.device.type == "cuda" and same(dev.cpu().numpy(), picture)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    assert tb.BakeLightmap(W, H, S, uv=dev_uv, settings=settings, out=out) is out and same(out.cpu().numpy(), picture)
    again = tb.ReadBake()
    assert same_bytes(again[0], rays) and same_bytes(again[1], rec) and same(again[2], sums)


@gpu
def test_accumulated_bakes_are_one_longer_bake(bake_tb, settings):
    """4. 8 samples = 3 then 5 accumulated = 8 x 1 accumulated; another size or a commit in between is refused."""
    import bake_cases as bc
    from tracerboy_amd import api
    tb = load(bake_tb, "cornell-box")
    W, H = bc.ATLAS_W, bc.ATLAS_H
    uv = atlas_of(tb, "cornell-box")
    whole = tb.BakeLightmap(W, H, 8, uv=uv, settings=settings); whole_sums = tb.ReadBake()[2]
    tb.BakeLightmap(W, H, 3, uv=uv, settings=settings)
    two = tb.BakeLightmap(W, H, 5, first_sample=3, accumulate=True, settings=settings)
    assert same(two, whole) and same(tb.ReadBake()[2], whole_sums)
    one = tb.BakeLightmap(W, H, 1, uv=uv, settings=settings)
    for s in range(1, 8):
        one = tb.BakeLightmap(W, H, 1, first_sample=s, accumulate=True, settings=settings)
    assert same(one, whole) and same(tb.ReadBake()[2], whole_sums)
    with pytest.raises(api.TracerBoyError) as e:                      # another size
        tb.BakeLightmap(W + 1, H, 1, first_sample=8, accumulate=True, settings=settings)
    assert e.value.code == -1 and "no bake of this size" in str(e.value)
    assert same(tb.ReadBake()[2], whole_sums)                         # the refusal left the bake as it was
    moved = host_arrays("cornell-box").positions.copy()
    keep = bc_emissive(tb)
    moved[~keep] += F32(0.001)
    tb.UpdatePositions(moved); tb.CommitGeometry()
    with pytest.raises(api.TracerBoyError) as e:                      # the scene has been committed since
        tb.BakeLightmap(W, H, 1, first_sample=8, accumulate=True, settings=settings)
    assert e.value.code == -1 and "committed" in str(e.value)
    load(tb, "cornell-box", fresh=True)
    with pytest.raises(api.TracerBoyError) as e:                      # nothing to add to
        tb.BakeLightmap(W, H, 1, accumulate=True, settings=settings)
    assert e.value.code == -1


def bc_emissive(tb):
    import dynamic_cases as dc
    return dc.emissive_vertices(tb.HostSceneView())


@gpu
def test_closed_forms(bake_tb, settings):
    """5. MaxBounces 0: covered texels are (0, 0, 0, 1); dilate 0: alpha is the coverage mask; the floor under the light is brighter than the
    ceiling beside it."""
    import bake_cases as bc
    import ctypes as C
    tb = load(bake_tb, "cornell-box")
    W, H = bc.ATLAS_W, bc.ATLAS_H
    uv = atlas_of(tb, "cornell-box")
    dark = copy.copy(settings); dark.MaxBounces = 0
    picture = tb.BakeLightmap(W, H, 4, uv=uv, dilate=0, settings=dark)
    rays, rec, sums = tb.ReadBake()
    mask = rec["triangle"] != NONE
    assert mask.any() and same(picture[mask], np.tile(F32([0, 0, 0, 1]), (mask.sum(), 1))) and not picture[~mask].any()
    assert np.array_equal(picture[..., 3] == 1, mask)
    lit = tb.BakeLightmap(W, H, 64, uv=uv, dilate=0, settings=settings)
    assert np.array_equal(lit[..., 3], mask.astype(F32))
    view = tb.HostSceneView()
    corners = np.array([[[p.x, p.y, p.z] for p in (l.P0, l.P1, l.P2)] for l in (view.lights[i] for i in range(view.numLights))], np.float64).reshape(-1, 3)
    light = corners.mean(0)
    pos = host_arrays("cornell-box").positions
    lo, hi = pos.min(0), pos.max(0)
    up = int(np.argmax(np.abs(light - (lo + hi) / 2) / (hi - lo)))    # the axis along which the light sits at the box's end
    sign = 1.0 if light[up] > (lo[up] + hi[up]) / 2 else -1.0
    groups = np.ctypeslib.as_array(C.cast(view.hitGroups, C.POINTER(C.c_uint32)), shape=(view.numHitGroups, 18))
    emissive = np.array([bool(view.materials[int(groups[g, 8])].Flags & 0x10) for g in range(view.numHitGroups)])
    geometry = host_arrays("cornell-box").geometry
    o, d = rays["Origin"].astype(np.float64), rays["Direction"].astype(np.float64)
    side = [a for a in range(3) if a != up]
    dist = np.linalg.norm(o[..., side] - light[side], axis=-1)
    plain = mask & ~emissive[geometry[np.where(mask, rec["triangle"], 0)]]
    floor = plain & (d[..., up] * sign > 0.9) & (np.abs(o[..., up] - (lo[up] if sign > 0 else hi[up])) < 0.05 * (hi - lo)[up])
    reach = 1.5 * np.linalg.norm(corners[:, side] - light[side], axis=1).max()   # beside the light, not above it: the light hangs just under the ceiling
    ceiling = plain & (dist > reach) & (d[..., up] * sign < -0.9) & (np.abs(o[..., up] - (hi[up] if sign > 0 else lo[up])) < 0.05 * (hi - lo)[up])
    assert floor.any() and ceiling.any()
    # "under the light" is in its sight: the boxes stand on the floor and shade part of it
    from tracerboy_amd import api
    to_light = light - o[floor]; length = np.linalg.norm(to_light, axis=1)
    shaded = tb.TraceRays(api.make_query_rays(o[floor], to_light / length[:, None], tmax=0.99 * length), api.RAYS_OCCLUDED).astype(bool)
    floor[floor] = ~shaded
    # A hemisphere sample meets the light only by chance (no feeler starts at the origin): under the light that is 0.18 / (pi 1.98^2) = 1.5 % of the
    # samples, 0.9 of 64 on average, so ONE floor texel's direct light is a Poisson draw and four in ten have none.  The ceiling has no direct light
    # and its first hits send feelers: it is smooth.  So: the floor texels under the light (its footprint widened by half, in its sight) against
    # the ceiling texels in the ring around the light as far out again -- their means (direct 0.77 + indirect against indirect alone, red), and the
    # brightest of those floor texels against the ceiling texel nearest the light.
    under = floor & (dist <= reach); beside = ceiling & (dist <= 2 * reach)
    assert under.sum() >= 8 and beside.sum() >= 8
    brightness = lit[..., :3].sum(-1, dtype=np.float64)
    c = np.unravel_index(np.argmin(np.where(ceiling, dist, np.inf)), dist.shape)
    print("floor under the light: %d texels, mean %.4f, max %.4f; ceiling beside it: %d texels, mean %.4f, nearest %.4f"
          % (under.sum(), brightness[under].mean(), brightness[under].max(), beside.sum(), brightness[beside].mean(), brightness[c]))
    assert brightness[under].max() > brightness[c] > 0
    assert brightness[under].mean() > brightness[beside].mean() > 0


@gpu
@pytest.mark.parametrize("scene", ["tri1", "tri3"])
def test_a_bake_follows_moved_vertices(bake_tb, settings, scene):
    """6. After UpdatePositions + CommitGeometry the ray origins are the restatement's on the moved positions, and the bake is TraceRadiance on them."""
    import bake_cases as bc
    from tracerboy_amd import api
    tb = load(bake_tb, scene, fresh=True)
    host = host_arrays(scene)
    records = bc.vertex_records(tb.HostSceneView())
    W, H, S = 13, 9, 4
    before = tb.BakeLightmap(W, H, S, settings=settings); rays0 = tb.ReadBake()[0]
    moved = (host.positions + np.random.default_rng(3).uniform(-0.2, 0.2, host.positions.shape)).astype(F32)
    tb.UpdatePositions(moved); tb.CommitGeometry()
    after = tb.BakeLightmap(W, H, S, settings=settings)
    rays, rec, sums = tb.ReadBake()
    want_rays, want_rec = bc.texels(W, H, moved, records[:, 0:3], records[:, 3:5], host.tri)
    assert same_bytes(rays, want_rays) and same_bytes(rec, want_rec) and (rec["triangle"] != NONE).any()
    assert not same_bytes(rays["Origin"], rays0["Origin"])
    assert same(sums.reshape(-1, 4), tb.TraceRadiance(rays.reshape(-1), S, 0, 0.0, mode=api.RADIANCE_HEMISPHERE, settings=settings))
    assert same(after, bc.dilate(bc.resolve(rec, sums), 2))
    tb._bake_scene = None                                             # moved: the next test loads it again


@gpu
def test_the_scenes_own_uvs(bake_tb, settings):
    """7. uv=None on material-maps equals the bake with the vertex records' UVs passed explicitly."""
    import bake_cases as bc
    tb = load(bake_tb, "material-maps")
    records = bc.vertex_records(tb.HostSceneView())
    own = tb.BakeLightmap(40, 24, 2, settings=settings); own_read = tb.ReadBake()
    given = tb.BakeLightmap(40, 24, 2, uv=np.ascontiguousarray(records[:, 3:5]), settings=settings); given_read = tb.ReadBake()
    assert same(own, given) and all(same_bytes(a, b) for a, b in zip(own_read, given_read))
    assert (own_read[1]["triangle"] != NONE).any() and own[..., :3].any()


@gpu
def test_every_refusal_on_a_live_context(built, settings):
    """8. Each refusal is followed by a correct bake, and ReadBake after a refusal returns the previous bake."""
    import bake_cases as bc
    import torch
    from tracerboy_amd import _ctypes_abi as abi, api
    INVALID, NO_SCENE, UNSUPPORTED = -1, -7, -6
    with api.TracerBoy(0) as tb:
        with pytest.raises(api.TracerBoyError) as e:
            tb.BakeLightmap(8, 8, 1)
        codes = {"no scene": e.value.code}
        with pytest.raises(api.TracerBoyError):
            tb.ReadBake()
        tb.LoadScene(CORNELL)
        with pytest.raises(api.TracerBoyError):
            tb.ReadBake()                                             # nothing baked yet
        uv = atlas_of(tb, "cornell-box")
        good = tb.BakeLightmap(16, 12, 2, uv=uv, settings=settings); held = tb.ReadBake()

        def refused(code, **kw):
            args = dict(width=16, height=12, samples=2, uv=uv, settings=settings); args.update(kw)
            with pytest.raises(api.TracerBoyError) as e:
                tb.BakeLightmap(**args)
            assert e.value.code == code, (kw, str(e.value))
            now = tb.ReadBake()
            assert all(same_bytes(a, b) for a, b in zip(now, held)), kw
            assert same(tb.BakeLightmap(16, 12, 2, uv=uv, settings=settings), good)

        realtime = copy.copy(settings); realtime.RenderModeRealTime = 1
        refused(UNSUPPORTED, settings=realtime)
        refused(INVALID, width=17, accumulate=True)
        # what Python's own checks keep from the library, through the library: the table's rows on a live context
        out = np.zeros((12, 16, 4), F32)
        raw = lambda call, u, o: tb._L.tb_bake_lightmap(tb._ctx, None, 0.0, ctypes.byref(call) if call is not None else None, u, o)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for call, u, o in ((None, p(uv), p(out)), (abi.tb_bake_call(0, 12, 0, 2, 2, 0), p(uv), p(out)), (abi.tb_bake_call(16, 8193, 0, 2, 2, 0), p(uv), p(out)),
                           (abi.tb_bake_call(16, 12, 0, 2, 2, 4), p(uv), p(out)), (abi.tb_bake_call(16, 12, 0, 0, 2, 0), p(uv), p(out)),
                           (abi.tb_bake_call(16, 12, 0, (1 << 24) + 1, 2, 0), p(uv), p(out)), (abi.tb_bake_call(16, 12, 0xffffffff, 2, 2, 0), p(uv), p(out)),
                           (abi.tb_bake_call(16, 12, 0, 2, 17, 0), p(uv), p(out)), (abi.tb_bake_call(16, 12, 0, 2, 2, 0), p(uv), None),
                           (abi.tb_bake_call(16, 12, 0, 2, 2, api.BAKE_DEVICE), p(uv), p(out))):   # host memory passed as device memory
            assert raw(call, u, o) == INVALID
            assert all(same_bytes(a, b) for a, b in zip(tb.ReadBake(), held))
            assert same(tb.BakeLightmap(16, 12, 2, uv=uv, settings=settings), good)
        dev =torch.zeros((12 * 16 * 4 + 1,), dtype=torch.float32, device="cuda:0")
        call = abi.tb_bake_call(16, 12, 0, 2, 2, api.BAKE_DEVICE)
        assert raw(call, None, ctypes.c_void_p(dev.data_ptr() + 4)) == INVALID            # misaligned
        # runs past its allocation (torch's allocator hands out parts of larger blocks: 1 GiB is past any block that holds a 3 KiB tensor)
        assert raw(abi.tb_bake_call(8192, 8192, 0, 2, 2, api.BAKE_DEVICE), None, ctypes.c_void_p(dev.data_ptr())) == INVALID
        assert all(same_bytes(a, b) for a, b in zip(tb.ReadBake(), held))
        assert same(tb.BakeLightmap(16, 12, 2, uv=uv, settings=settings), good)
        assert codes["no scene"] == NO_SCENE
        # a two-level scene
        tb.SetOption("flatten_instances", 0)
        tb.LoadScene(os.path.join(os.path.dirname(os.path.dirname(CORNELL)), "instances", "scene.pbrt"))
        tb.SetOption("flatten_instances", 1)
        assert tb.HostSceneView().numInstances > 0
        with pytest.raises(api.TracerBoyError) as e:
            tb.BakeLightmap(16, 12, 2, settings=settings)
        assert e.value.code == UNSUPPORTED
        tb.LoadScene(CORNELL)
        assert same(tb.BakeLightmap(16, 12, 2, uv=uv, settings=settings), good)
    if torch.cuda.device_count() > 1:
        with api.TracerBoy(devices=[0, 1]) as group:
            group.LoadScene(CORNELL)
            with pytest.raises(api.TracerBoyError) as e:
                group.BakeLightmap(16, 12, 2, settings=settings)
            assert e.value.code == UNSUPPORTED


@gpu
def test_a_bake_holds_memory_from_the_first_bake_to_close(built, settings):
    """9. debug_live_device_bytes rises at the first bake, stays at a second of the same size and returns to its former value after close()."""
    from tracerboy_amd import api
    with api.TracerBoy(0) as other:                                   # the count is the process's: read through a context that stays
        before = other.GetOption("debug_live_device_bytes")
        tb = api.TracerBoy(0)
        tb.LoadScene(CORNELL)
        tb.TraceRadiance(api.make_radiance_rays(np.zeros((1, 3)), [[0, 1, 0]]), mode=api.RADIANCE_HEMISPHERE, settings=settings)  # the query's own counter
        loaded = other.GetOption("debug_live_device_bytes")
        tb.Render(16, 16, 1, settings)
        assert tb.GetOption("bake_width") == 0
        rendered = other.GetOption("debug_live_device_bytes")
        tb.BakeLightmap(32, 16, 1, settings=settings)
        first = other.GetOption("debug_live_device_bytes")
        assert first >= rendered + 32 * 16 * (32 + 16 + 16 + 16 + 16 + 8) and loaded > before
        tb.BakeLightmap(32, 16, 2, dilate=5, settings=settings)
        tb.BakeLightmap(32, 16, 1, first_sample=2, accumulate=True, settings=settings)
        assert other.GetOption("debug_live_device_bytes") == first
        tb.close()
        assert other.GetOption("debug_live_device_bytes") == before


@gpu
def test_the_command_line_bakes(bake_tb, tmp_path):
    """10. A 32 x 32, 2-sample bake written as .pfm equals the Python bake; a render flag beside it exits with status 2."""
    from tracerboy_amd import api
    cli = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
    out = str(tmp_path / "lm.pfm")
    r = subprocess.run([cli, CORNELL, "--bake-lightmap", "32x32", "--bake-samples", "2", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tb = load(bake_tb, "cornell-box")
    want = tb.BakeLightmap(32, 32, 2)
    got = api.DecodeImage(out)[0]
    assert got.shape == (32, 32, 4) and same(got[..., :3], want[..., :3])
    r = subprocess.run([cli, CORNELL, "--bake-lightmap", "32x32", "--bake-samples", "2", "--bake-dilate", "0", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and same(api.DecodeImage(out)[0][..., :3], tb.BakeLightmap(32, 32, 2, dilate=0)[..., :3])


def test_the_command_line_refuses_before_any_device_call(built, tmp_path):
    """A render, denoise, upscale, resume or --ranks flag beside --bake-lightmap, a malformed size and a .png: exit status 2, on a machine without a GPU too."""
    cli = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
    out = str(tmp_path / "lm.pfm")
    base = [cli, CORNELL, "--bake-lightmap", "32x32", "--bake-samples", "2", "--out", out]
    for extra in (["--spp", "4"], ["--denoise"], ["--upscale", "64x64"], ["--resume", "x.tbs"], ["--ranks", "2"], ["--width", "32"], ["--denoise-neural", "w.tza"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "bake" in r.stderr, (extra, r.returncode, r.stderr)
    for args in ([cli, CORNELL, "--bake-lightmap", "32", "--bake-samples", "2", "--out", out], [cli, CORNELL, "--bake-lightmap", "32x0", "--bake-samples", "2", "--out", out],
                 [cli, CORNELL, "--bake-lightmap", "32x32", "--out", out], [cli, CORNELL, "--bake-lightmap", "32x32", "--bake-samples", "2", "--out", str(tmp_path / "lm.png")],
                 [cli, CORNELL, "--bake-lightmap", "32x32", "--bake-samples", "2", "--bake-dilate", "17", "--out", out]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
    assert not os.path.exists(out)
