"""Scenes from caller arrays and smooth normals recomputed on the device (include/tracerboy_hip.h tb_load_meshes,
tb_host_scene_from_meshes, tb_meshes_refusal, tb_host_smooth_normals, tb_recompute_normals).  The yardstick (include/tb_normals.h restated in numpy)
and the meshes come from tests/mesh_cases.py; rays are ray_query_cases', the atlas rule bake_cases', expected pictures and hits the CPU oracle's."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dynamic_cases as dc
import mesh_cases as mc
import ray_query_cases as rq
from conftest import ROOT, CORNELL

gpu = pytest.mark.gpu
F32 = np.float32
W, H, FRAMES = 32, 24, 2
E_INVALID, E_UNSUPPORTED, E_NO_SCENE = -1, -6, -7
FLAT3 = os.path.join(dc.DYNAMIC, "flat3.pbrt")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def test_header_library_bindings_and_methods_agree(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracerboy_hip.h")).read(), flags=re.S)
    a = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tb_abi.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+tb_load_meshes\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*const\s+tb_scene_desc\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_host_scene_from_meshes\s*\(\s*const\s+tb_scene_desc\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*tb_host_scene\s*\*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_meshes_refusal\s*\(\s*const\s+tb_scene_desc\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_host_smooth_normals\s*\(\s*const\s+float\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_recompute_normals\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*\)", h)
    for name, value in (("TB_MESH_NORMALS_FLAT", "0u"), ("TB_MESH_NORMALS_SMOOTH", "1u"), ("TB_MESH_DEVICE", "0x100u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), a), name
    assert (abi.TB_MESH_NORMALS_FLAT, abi.TB_MESH_NORMALS_SMOOTH, abi.TB_MESH_DEVICE) == (0, 1, 0x100) == (api.MESH_NORMALS_FLAT, api.MESH_NORMALS_SMOOTH, api.MESH_DEVICE)
    assert api.MESH_DEVICE == api.RAYS_DEVICE
    # the struct mirrors: the fields of the header in its order, on the C layout
    for struct, mirror in (("tb_mesh_desc", abi.tb_mesh_desc), ("tb_scene_desc", abi.tb_scene_desc)):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), a, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *more = decl.split(",")
                names += [re.search(r"(\w+)\s*(\[\d+\])?$", first.strip()).group(1)] + [m.strip() for m in more]
        assert names == [n for n, _ in mirror._fields_], struct
    assert C.sizeof(abi.tb_mesh_desc) == 56 and abi.tb_mesh_desc.material.offset == 48 and abi.tb_mesh_desc.normals_mode.offset == 52
    assert C.sizeof(abi.tb_scene_desc) == 80 and abi.tb_scene_desc.env_scale.offset == 56 and abi.tb_scene_desc.flags.offset == 76
    raw, bound = C.CDLL(api.LIB_PATH), api.lib()
    vp, u32, P = C.c_void_p, C.c_uint32, C.POINTER
    want = {"tb_load_meshes": [vp, P(abi.tb_scene_desc)], "tb_meshes_refusal": [P(abi.tb_scene_desc), C.c_char_p, u32],
            "tb_host_scene_from_meshes": [P(abi.tb_scene_desc), C.c_int, P(vp), C.c_char_p, u32], "tb_host_smooth_normals": [vp, u32, vp, u32, vp],
            "tb_recompute_normals": [vp, u32, u32]}
    for name, args in want.items():
        assert hasattr(raw, name) and name in bound._tb_exports, name
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == C.c_int, name
    for method in ("LoadMeshes", "RecomputeNormals"):
        assert callable(getattr(api.TracerBoy, method)), method
    assert callable(api.HostScene.from_meshes) and callable(api.MeshesRefusal) and callable(api.Mesh) and callable(api.HostSmoothNormals)


def test_wrong_arrays_are_refused_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    p, i = mc.one_triangle()
    mats = mc.MATERIALS()
    wrong = {
        "float64 positions": api.Mesh(p.astype(np.float64), i),
        "positions of shape (n, 4)": api.Mesh(np.zeros((3, 4), F32), i),
        "flat positions": api.Mesh(p.reshape(-1), i),
        "non-contiguous positions": api.Mesh(np.zeros((6, 3), F32)[::2], i),
        "int32 numpy indices": api.Mesh(p, i.astype(np.int32)),
        "int64 indices": api.Mesh(p, i.astype(np.int64)),
        "indices of shape (m, 4)": api.Mesh(p, np.zeros((1, 4), np.uint32)),
        "flat indices": api.Mesh(p, i.reshape(-1)),
        "normals of the wrong length": api.Mesh(p, i, normals=np.zeros((2, 3), F32)),
        "uvs of shape (n, 3)": api.Mesh(p, i, uvs=np.zeros((3, 3), F32)),
        "float64 uvs": api.Mesh(p, i, uvs=np.zeros((3, 2), np.float64)),
        "a list": api.Mesh(p.tolist(), i),
        "missing indices": api.Mesh(p, None),
        "a tensor on the CPU": api.Mesh(torch.from_numpy(p), torch.from_numpy(i.astype(np.int32))),
        "numpy and torch mixed": api.Mesh(p, torch.from_numpy(i.astype(np.int32))),
        "a negative material": api.Mesh(p, i, material=-1),
        "a material that is no index": api.Mesh(p, i, material=1.5),
    }
    for what, mesh in wrong.items():
        with pytest.raises(ValueError):
            tb.LoadMeshes([mesh], mats)
            pytest.fail(what)
        with pytest.raises(ValueError):
            api.HostScene.from_meshes([mesh], mats)
            pytest.fail(what)
    good = api.Mesh(p, i)
    for what, kw in {"not a Mesh": dict(meshes=[(p, i)]), "a material that is no TbMaterial": dict(materials=[None]),
                     "a float64 environment": dict(environment=np.zeros((2, 2, 4), np.float64)), "an environment of 3 channels": dict(environment=np.zeros((2, 2, 3), F32)),
                     "two env scales": dict(env_scale=(1, 1)), "a film of three": dict(film=(1, 2, 3))}.items():
        args = dict(meshes=[good], materials=mats); args.update(kw)
        with pytest.raises(ValueError):
            tb.LoadMeshes(**args)
            pytest.fail(what)
    with pytest.raises(AttributeError):                               # the good mesh gets past the checks, to the library this object lacks
        tb.LoadMeshes([good], mats)
    for first, n in ((-1, None), (0, -1), (1.5, None), (0, 1 << 32), (True, None)):
        with pytest.raises(ValueError):
            tb.RecomputeNormals(first, n)
    with pytest.raises(AttributeError):
        tb.RecomputeNormals(0, 3)


def _desc(meshes, materials, **kw):
    from tracerboy_amd import api
    args = dict(camera=None, environment=None, env_scale=(1, 1, 1), film=(0, 0)); args.update(kw)
    d, keep, _ = api._scene_desc("test", meshes, materials, args["camera"], args["environment"], args["env_scale"], args["film"], None)
    return d, keep


def test_every_argument_refusal_names_its_cause(built):
    """tb_meshes_refusal, in the header's order; then tb_host_scene_from_meshes's value checks, each naming its mesh and element."""
    from tracerboy_amd import _ctypes_abi as abi, api
    p, i = mc.one_triangle(); fp, fi = mc.fan()
    mats = mc.MATERIALS()
    meshes = lambda: [api.Mesh(fp, fi, smooth=True), api.Mesh(p, i, material=1)]
    assert api.MeshesRefusal(None) == "null desc"
    d, keep = _desc(meshes(), mats)
    assert api.MeshesRefusal(d) is None
    cases = []
    def broken(expect, change):
        d, keep = _desc(meshes(), mats, environment=np.ones((2, 3, 4), F32))
        change(d)
        cases.append((expect, api.MeshesRefusal(d)))
    broken("no meshes", lambda d: setattr(d, "n_meshes", 0))
    broken("no materials", lambda d: setattr(d, "n_materials", 0))
    broken("mesh 1: null positions", lambda d: setattr(d.meshes[1], "positions", None))
    broken("mesh 1: null indices", lambda d: setattr(d.meshes[1], "indices", None))
    broken("mesh 0: 0 vertices", lambda d: setattr(d.meshes[0], "n_vertices", 0))
    broken("mesh 1: 0 triangles", lambda d: setattr(d.meshes[1], "n_triangles", 0))
    broken("mesh 1: material 3 is at or past the 3 materials", lambda d: setattr(d.meshes[1], "material", 3))
    broken("mesh 0: unknown normals mode 2", lambda d: setattr(d.meshes[0], "normals_mode", 2))
    broken("unknown flag bits", lambda d: setattr(d, "flags", 0x101))
    broken("a side of the environment is 0", lambda d: setattr(d, "env_width", 0))
    broken("a side of the environment is above 16384", lambda d: setattr(d, "env_height", 16385))
    broken("more than 2^24 - 1 triangles in total", lambda d: setattr(d.meshes[0], "n_triangles", (1 << 24) - 1))
    broken("more than 2^27 - 1 vertices in total", lambda d: setattr(d.meshes[0], "n_vertices", (1 << 27) - 3))
    for expect, got in cases:
        assert got == expect
    # index bytes past 2^32 cannot be reached below the triangle limit (2^24 x 12 B): the test stands, the limits above come first
    # the value checks
    def refused(expect_code, expect_text, ms, materials=mats, **kw):
        with pytest.raises(api.TracerBoyError) as e:
            api.HostScene.from_meshes(ms, materials, **kw)
        assert e.value.code == expect_code and expect_text in str(e.value), str(e.value)
    bad = fi.copy(); bad[5, 1] = len(fp)
    refused(E_INVALID, "mesh 1: index %d (triangle 5, corner 1) is at or past its %d vertices" % (len(fp), len(fp)), [api.Mesh(p, i), api.Mesh(fp, bad)])
    nan = fp.copy(); nan[7, 2] = np.nan
    refused(E_INVALID, "mesh 0: the position of vertex 7 is not finite", [api.Mesh(nan, fi), api.Mesh(p, i)])
    inf = np.zeros_like(p); inf[2, 0] = np.inf
    refused(E_INVALID, "mesh 1: the normal of vertex 2 is not finite", [api.Mesh(fp, fi), api.Mesh(p, i, normals=inf)])
    uv = np.zeros((3, 2), F32); uv[1, 1] = -np.inf
    refused(E_INVALID, "mesh 1: the UV of vertex 1 is not finite", [api.Mesh(fp, fi), api.Mesh(p, i, uvs=uv)])
    env = np.ones((2, 3, 4), F32); env[1, 2, 0] = np.nan
    refused(E_INVALID, "environment texel 5 is not finite", meshes(), environment=env)
    textured = mc.MATERIALS(); textured[1].normalMapIndex = 0
    refused(E_UNSUPPORTED, "material 1 names a texture", meshes(), materials=textured)
    d, keep = _desc(meshes(), mats); d.flags = api.MESH_DEVICE
    out, err = C.c_void_p(), C.create_string_buffer(256)
    assert api.lib().tb_host_scene_from_meshes(C.byref(d), 0, C.byref(out), err, 256) == E_INVALID and b"host arrays only" in err.value and not out.value


def _round_trip(hs, builder, **kw):
    from tracerboy_amd import api
    meshes, materials = mc.cut_meshes(hs)
    return meshes, api.HostScene.from_meshes(meshes, materials, camera=hs.camera(), bvh_builder=builder, **kw)


@pytest.mark.parametrize("name,builder", [("cornell", 0), ("cornell", 1), ("proc10k", 0)])
def test_a_scene_cut_into_arrays_and_handed_back_is_the_same_scene(built, name, builder):
    from tracerboy_amd import api
    hs = api.HostScene(CORNELL, bvh_builder=builder) if name == "cornell" else api.HostScene(procedural=(0, dc.PROC_TRIANGLES, dc.PROC_SEED), bvh_builder=builder)
    env = dict(environment=np.ones((1, 1, 4), F32)) if name == "proc10k" else {}
    meshes, back = _round_trip(hs, builder, film=(hs.info().filmWidth, hs.info().filmHeight), **env)
    a, b = hs.view(), back.view()
    assert same_bytes(dc.bvh_bytes(a), dc.bvh_bytes(b))
    assert same_bytes(mc.index_buffer(a), mc.index_buffer(b)) and same_bytes(mc.vertex_buffer(a), mc.vertex_buffer(b))
    assert same_bytes(mc.hit_groups(a), mc.hit_groups(b)) and same_bytes(mc.material_bytes(a), mc.material_bytes(b))
    la, lb = mc.lights_of(a), mc.lights_of(b)
    assert la.shape == lb.shape and np.array_equal(la[:, 0:14], lb[:, 0:14])          # LightType, LightColor, SurfaceArea, P0..P2
    ta, tb_ = hs.triangles(), back.triangles()
    for k in ta:
        assert same_bytes(ta[k], tb_[k]), k
    if name == "cornell":
        assert len(lb) == 2
        light = [g for g, m in enumerate(meshes) if mc.materials_of(b)[m.material].Flags & mc.MAT_LIGHT]
        assert len(light) == 1
        m = meshes[light[0]]
        assert np.array_equal(lb[:, 14:23].view(F32).reshape(-1, 3, 3), m.normals[m.indices.astype(np.int64)])   # N0..N2: the vertex records' normals
    else:
        assert back.digest() == hs.digest()                           # no file UVs to flip, the same environment: every array of the seam
    assert bytes(back.camera()) == bytes(hs.camera()) and (back.info().filmWidth, back.info().filmHeight) == (hs.info().filmWidth, hs.info().filmHeight)
    ranges = mc.vertex_ranges(meshes)
    groups = mc.hit_groups(b)
    assert [int(o) // 32 for o in groups[:, 10]] == [f for f, _ in ranges] and sum(n for _, n in ranges) == b.numVertexFloats // 8


def test_fma32_is_the_correctly_rounded_one():
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal(400).astype(F32), rng.standard_normal(400).astype(F32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.uniform(-1, 1, 400) * 2.0 ** rng.integers(-30, -1, 400))).astype(F32)   # cancellation: where double rounding bites
    got = mc.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        near = F32(float(exact))
        cands = [near, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf))]
        want = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert g.view(np.uint32) == want.view(np.uint32)


@pytest.mark.parametrize("case", list(mc.RULE_CASES))
def test_host_smooth_normals_are_the_rule_bit_for_bit(built, case):
    from tracerboy_amd import api
    p, i = mc.RULE_CASES[case]()
    want = mc.smooth_normals(p, i)
    got = api.HostSmoothNormals(p, i)
    assert same_bytes(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    moved = mc.displaced(p)
    assert same_bytes(api.HostSmoothNormals(moved, i), mc.smooth_normals(moved, i))
    named = np.zeros(len(p), bool); named[i.reshape(-1)] = True
    lengths = np.linalg.norm(got.astype(np.float64), axis=1)
    assert np.allclose(lengths, 1.0, atol=1e-6)
    if case == "blob of 257":
        assert len(p) == 257 and len(i) == 510 and named.all()
        assert (np.einsum("ij,ij->i", got, p) > 0).all()             # a closed surface around the origin, wound outward
    if case == "fan of 70":
        assert (i == 0).sum() == 70 and got[0, 1] > 0.9
    if case == "unnamed vertex":
        assert not named[3] and np.array_equal(got[3], F32([0, 1, 0]))
        kept = api.HostSmoothNormals(p, i, out=np.full((4, 3), 7, F32))
        assert np.array_equal(kept[3], F32([7, 7, 7])) and same_bytes(kept[:3], want[:3])
    if case == "zero area":
        assert np.array_equal(got[3:], np.tile(F32([0, 1, 0]), (3, 1))) and not np.array_equal(got[0], F32([0, 1, 0]))
    if case == "twice named":
        assert same_bytes(got[:3], mc.smooth_normals(p[:3], i[:1])) and np.array_equal(got[3], F32([0, 1, 0]))
    with pytest.raises(api.TracerBoyError):
        api.HostSmoothNormals(p, np.uint32([[0, 1, len(p)]]))


def test_smooth_mode_of_a_load_is_the_rule_and_the_lights_carry_it(built):
    from tracerboy_amd import api
    meshes, materials = mc.blob_fan_quad()
    meshes.append(api.Mesh(*mc.one_triangle()[:2], material=2, smooth=True))     # an emissive mesh without normals, smooth
    meshes.append(api.Mesh(*mc.one_triangle()[:2], material=2))                  # and a flat one: the loader's face normal
    hs = api.HostScene.from_meshes(meshes, materials)
    vb = mc.vertex_buffer(hs.view())
    for m, (first, n) in zip(meshes, mc.vertex_ranges(meshes)):
        rec = vb[first:first + n]
        if m.normals is None and m.smooth:
            assert same_bytes(np.ascontiguousarray(rec[:, 0:3]), mc.smooth_normals(m.positions, m.indices))
        elif m.normals is not None:
            assert same_bytes(np.ascontiguousarray(rec[:, 0:3]), m.normals)
        assert same_bytes(np.ascontiguousarray(rec[:, 3:5]), m.uvs if m.uvs is not None else np.zeros((n, 2), F32))
        assert np.array_equal(rec[:, 5:8], np.tile(F32([0, 0, 1]), (n, 1)))
    lights = mc.lights_of(hs.view())
    assert len(lights) == 4 and (lights[:, 0] == 0).all() and np.array_equal(lights[:, 1:4].view(F32), np.tile(F32([17, 12, 4]), (4, 1)))
    p, i = mc.one_triangle()
    assert same_bytes(np.ascontiguousarray(lights[2, 5:14].view(F32).reshape(3, 3)), p[i[0]])
    assert same_bytes(np.ascontiguousarray(lights[2, 14:23].view(F32).reshape(3, 3)), mc.smooth_normals(p, i)[i[0]])
    e1, e2 = (p[1] - p[0]).astype(F32), (p[2] - p[0]).astype(F32)
    face = np.cross(e1.astype(np.float64), e2.astype(np.float64)); face /= np.linalg.norm(face)
    flat = lights[3, 14:23].view(F32).reshape(3, 3)
    assert np.array_equal(flat[0], flat[1]) and np.array_equal(flat[0], flat[2]) and np.allclose(flat[0], face, atol=1e-6)


@pytest.mark.parametrize("path", [FLAT3, dc.SCENES["tri3"]])
def test_flat_mode_is_the_loaders_rule(built, path):
    """A mesh without normals from a file and the same mesh from arrays in flat mode: the same vertex records."""
    from tracerboy_amd import api
    hs = api.HostScene(path)
    meshes, materials = mc.cut_meshes(hs)
    without = [g for g, m in enumerate(meshes) if path == FLAT3 or g > 0]             # tri3's first mesh brings normals
    assert without
    for g in without:
        meshes[g].normals = None
    back = api.HostScene.from_meshes(meshes, materials, camera=hs.camera())
    assert same_bytes(mc.vertex_buffer(back.view()), mc.vertex_buffer(hs.view()))
    if path == FLAT3:
        n = mc.vertex_buffer(hs.view())[:, 0:3]
        assert np.array_equal(n[3], F32([0, 1, 0])) and np.array_equal(n[4], F32([0, 1, 0]))     # the triangle of no area was the last to touch them
        assert np.array_equal(n[1], n[2]) and not np.array_equal(n[0], n[1])                     # triangle 1 overwrote what triangle 0 gave 1 and 2


def test_an_array_scene_has_a_valid_tree_and_its_default_camera_sees_it(built, settings):
    import oracle_lib as ol
    from tracerboy_amd import api
    meshes, materials = mc.fan_and_quad()
    colour = F32([0.25, 0.5, 0.75, 1.0])
    for builder in (0, 1):
        hs = api.HostScene.from_meshes(meshes, materials, environment=colour.reshape(1, 1, 4).copy(), bvh_builder=builder)
        view = hs.view(); image = dc.bvh_bytes(view)
        rc, depth = ol.validate_bvh(image, dc.tri_dict(view, image, hs.triangles()["positions"]))
        assert rc == 0 and depth == hs.info().bvhMaxDepth
    assert (hs.info().filmWidth, hs.info().filmHeight) == (1920, 1080) and hs.info().numGeometries == 2 and hs.info().numLights == 2
    out = ol.render(view, hs.frame_constants(settings), W, H, FRAMES, threads=8)["output"]
    assert np.isfinite(out).all()
    sky = out[0, 0]
    assert (out[:, :, :3] != sky[:3]).any(axis=2).sum() > 20 and (out[:, :, :3] == sky[:3]).all(axis=2).sum() > 20    # the mesh, and the environment around it


def test_the_default_camera_is_the_documented_formula(built):
    from tracerboy_amd import api
    meshes, materials = mc.blob_fan_quad()
    for ms in (meshes, [api.Mesh(np.tile(F32([[1, 2, 3]]), (3, 1)), np.uint32([[0, 1, 2]]))]):          # the second: bounds of no extent, d = 1
        cam = api.HostScene.from_meshes(ms, materials).camera()
        want = mc.default_camera([m.positions for m in ms])
        for field in ("Position", "LookAt", "Right", "Up"):
            assert same_bytes(np.array(getattr(cam, field)[:], F32), want[field]), field
        assert F32(cam.LensHeight) == want["LensHeight"] and F32(cam.FocalDistance) == want["FocalDistance"]
        assert hs_lens(api.HostScene.from_meshes(ms, materials)) == 2.0
    given = api.HostScene(CORNELL).camera()
    assert bytes(api.HostScene.from_meshes(meshes, materials, camera=given).camera()) == bytes(given)


def hs_lens(hs):
    return hs.view().config.CameraLensHeight


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

def render(tb, settings):
    tb.InvalidateHistory()
    tb.Render(W, H, FRAMES, settings, 0.0)
    return tb.ReadAccumulation().copy()


def oracle_render(tb, settings):
    import oracle_lib as ol
    return ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, settings, 0.0), W, H, FRAMES, threads=8)["output"]


def normals_of(tb):
    return np.ascontiguousarray(mc.vertex_buffer(tb.HostSceneView())[:, 0:3])


@gpu
def test_an_array_scene_from_numpy_and_from_torch_is_one_scene(gpu_tb, settings):
    import bake_cases as bc
    from tracerboy_amd import api
    tb = gpu_tb
    meshes, materials = mc.fan_and_quad()
    try:
        for builder in (0, 2):
            tb.SetOption("bvh_builder", builder)
            host = api.HostScene.from_meshes(meshes, materials, bvh_builder=builder)
            tb.LoadMeshes(meshes, materials)
            digest = tb.SceneDigest()
            assert same_bytes(dc.bvh_bytes(tb.HostSceneView()), dc.bvh_bytes(host.view()))
            if builder == 0:
                assert digest == host.digest()
            for int32 in (True, False):
                tb.LoadMeshes(mc.to_torch(meshes, int32=int32), materials)
                assert tb.SceneDigest() == digest
    finally:
        tb.SetOption("bvh_builder", 0)
    tb.LoadMeshes(meshes, materials)
    assert [tb.GeometryVertexRange(g) for g in range(2)] == mc.vertex_ranges(meshes)
    assert same_bytes(render(tb, settings), oracle_render(tb, settings))
    view = tb.HostSceneView()
    lo, hi = dc.bounds_of(view, dc.bvh_bytes(view))
    rays, oracle = rq.build_rays(view, tb.FrameConstants(64, 48, 0, settings, 0.0), tb.GetCamera().LensHeight, lo, hi)
    got = tb.TraceRays(rays, api.RAYS_CLOSEST); want = rq.expected_hits(rays, oracle)
    for field in api.QUERY_HIT_DTYPE.names:
        assert same_bytes(got[field], want[field]), field
    assert (got["T"] > 0).sum() > 100
    compare = ~rq.near_tmax(rays, oracle)
    assert np.array_equal(tb.TraceRays(rays, api.RAYS_OCCLUDED)[compare], rq.expected_occluded(rays, oracle)[compare])
    tb.BakeLightmap(16, 16, 2, settings=settings)                   # the meshes' own UVs
    records = mc.vertex_buffer(view)
    tri = np.concatenate([m.indices + first for m, (first, _) in zip(meshes, mc.vertex_ranges(meshes))]).astype(np.uint32)
    positions = np.concatenate([m.positions for m in meshes])
    _, rec = bc.texels(16, 16, positions, records[:, 0:3], records[:, 3:5], tri)
    assert tb.GetOption("last_bake_covered") == (rec["triangle"] != bc.NONE).sum() > 50


@gpu
def test_cornell_box_from_arrays_renders_as_the_loaded_one(gpu_tb, settings):
    from tracerboy_amd import api
    tb = gpu_tb
    tb.LoadScene(CORNELL)
    loaded = render(tb, settings); variant = (tb.GetOption("last_variant"), tb.GetOption("last_copy_waves"), tb.GetOption("scene_in_lds_active"))
    hs = api.HostScene(CORNELL)
    meshes, materials = mc.cut_meshes(hs)
    tb.LoadMeshes(meshes, materials, camera=hs.camera())
    assert same_bytes(dc.bvh_bytes(tb.HostSceneView()), dc.bvh_bytes(hs.view()))
    assert same_bytes(render(tb, settings), loaded)
    assert (tb.GetOption("last_variant"), tb.GetOption("last_copy_waves"), tb.GetOption("scene_in_lds_active")) == variant and variant[2] == 1


def load_three(tb):
    meshes, materials = mc.blob_fan_quad()
    tb.LoadMeshes(meshes, materials)
    return meshes, materials, mc.vertex_ranges(meshes)


def moved_meshes(meshes):
    """every mesh but the emissive quad displaced (section 21 does not let a light move)"""
    return [mc.displaced(m.positions, mc.DISPLACE_SEED + k) if k < 2 else m.positions for k, m in enumerate(meshes)]


@gpu
def test_normals_recomputed_on_the_device_are_the_hosts(gpu_tb, settings):
    from tracerboy_amd import api
    tb = gpu_tb
    meshes, materials, ranges = load_three(tb)
    assert tb.GetOption("dynamic_state") == 0
    before = mc.vertex_buffer(tb.HostSceneView()); digest = tb.SceneDigest()
    moved = moved_meshes(meshes)
    tb.Render(W, H, 1, settings, 0.0)
    tb.UpdatePositions(np.concatenate(moved)); tb.RecomputeNormals()
    assert same_bytes(mc.vertex_buffer(tb.HostSceneView()), before) and tb.SceneDigest() == digest        # nothing changes before the commit
    assert tb.GetNumberOfSamplesSinceLastInvalidate() == 1
    tb.CommitGeometry()
    assert tb.GetNumberOfSamplesSinceLastInvalidate() == 0 and tb.SceneDigest() != digest
    after = mc.vertex_buffer(tb.HostSceneView())
    for k, (first, n) in enumerate(ranges):
        got = np.ascontiguousarray(after[first:first + n, 0:3])
        if k < 2:
            want = api.HostSmoothNormals(moved[k], meshes[k].indices)
            assert same_bytes(got, want), (k, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
            assert same_bytes(want, mc.smooth_normals(moved[k], meshes[k].indices)) and not same_bytes(got, np.ascontiguousarray(before[first:first + n, 0:3]))
        else:
            assert same_bytes(got, meshes[k].normals)                # the quad's stay
    assert same_bytes(np.ascontiguousarray(after[:, 3:8]), np.ascontiguousarray(before[:, 3:8]))             # UVs and tangents stay
    assert same_bytes(render(tb, settings), oracle_render(tb, settings))                                      # a render after the commit
    # load and commit agree: the moved positions loaded with smooth normals
    vb = mc.vertex_buffer(tb.HostSceneView()); image = dc.bvh_bytes(tb.HostSceneView())
    fresh = [api.Mesh(p, m.indices, m.normals, m.uvs, m.material, m.smooth) for p, m in zip(moved, meshes)]
    tb.LoadMeshes(fresh, materials)
    assert same_bytes(mc.vertex_buffer(tb.HostSceneView()), vb)


@gpu
def test_partial_marks_device_updates_and_explicit_normals(gpu_tb):
    import torch
    from tracerboy_amd import api
    tb = gpu_tb
    meshes, materials, ranges = load_three(tb)
    before = normals_of(tb)
    moved = moved_meshes(meshes)
    # a partial mark: mesh 1 alone; mesh 0 moves too, and keeps its normals' bytes
    tb.UpdatePositions(np.concatenate(moved)); tb.RecomputeNormals(*ranges[1]); tb.CommitGeometry()
    got = normals_of(tb)
    (f0, n0), (f1, n1), (f2, n2) = ranges
    assert same_bytes(got[f0:f0 + n0], before[f0:f0 + n0]) and same_bytes(got[f2:], before[f2:])
    assert same_bytes(got[f1:f1 + n1], api.HostSmoothNormals(moved[1], meshes[1].indices))
    # a mark inside a mesh: the face vectors are taken over all of their vertices, marked or not
    tb.RecomputeNormals(f0 + 100, 57); tb.CommitGeometry()
    part = normals_of(tb)
    whole = api.HostSmoothNormals(moved[0], meshes[0].indices)
    assert same_bytes(part[f0 + 100:f0 + 157], whole[100:157]) and same_bytes(part[f0:f0 + 100], before[f0:f0 + 100]) and same_bytes(part[f0 + 157:f0 + n0], before[f0 + 157:f0 + n0])
    # the same update from numpy and from a device tensor
    meshes, materials, ranges = load_three(tb)
    tb.UpdatePositions(torch.from_numpy(np.concatenate(moved)).to("cuda:0")); tb.RecomputeNormals(); tb.CommitGeometry()
    from_device = mc.vertex_buffer(tb.HostSceneView())
    meshes, materials, ranges = load_three(tb)
    tb.UpdatePositions(np.concatenate(moved)); tb.RecomputeNormals(); tb.CommitGeometry()
    from_host = mc.vertex_buffer(tb.HostSceneView())
    assert same_bytes(from_device, from_host)
    # an explicit normal and a recomputation of the same vertex in one commit: the recomputed value; an explicit normal beside the mark: as given
    digest = tb.SceneDigest()
    explicit = np.tile(F32([[1, 0, 0]]), (4, 1))
    tb.UpdateNormals(explicit, f1); tb.RecomputeNormals(f1, 2); tb.CommitGeometry()
    got = normals_of(tb)
    assert same_bytes(got[f1:f1 + 2], np.ascontiguousarray(from_host[f1:f1 + 2, 0:3])) and same_bytes(got[f1 + 2:f1 + 4], explicit[2:])
    assert tb.SceneDigest() != digest
    # a commit of marks alone counts as a change
    tb.Render(W, H, 1); digest = tb.SceneDigest()
    tb.RecomputeNormals(f1, 4); tb.CommitGeometry()
    assert tb.GetNumberOfSamplesSinceLastInvalidate() == 0 and tb.SceneDigest() != digest
    assert same_bytes(normals_of(tb), np.ascontiguousarray(from_host[:, 0:3]))
    tb.RecomputeNormals(0, 0); tb.Render(W, H, 1); tb.CommitGeometry()                                       # n = 0: nothing staged
    assert tb.GetNumberOfSamplesSinceLastInvalidate() == 1


@gpu
def test_refusals_leave_the_scene_as_it_was(gpu_tb, settings, built):
    import torch
    from tracerboy_amd import _ctypes_abi as abi, api
    tb = gpu_tb
    meshes, materials, ranges = load_three(tb)
    digest, picture = tb.SceneDigest(), render(tb, settings)
    nv = sum(n for _, n in ranges)
    p, i = mc.one_triangle()

    def unchanged():
        assert tb.SceneDigest() == digest and same_bytes(render(tb, settings), picture)

    def refused(code, text, call):
        with pytest.raises(api.TracerBoyError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)
        unchanged()

    bad = i.copy(); bad[0, 2] = 3
    nan = p.copy(); nan[1, 0] = np.nan
    textured = mc.MATERIALS(); textured[0].albedoIndex = 0
    env = np.ones((1, 2, 4), F32); env[0, 1, 3] = np.inf
    refused(E_INVALID, "mesh 0: material 3 is at or past the 3 materials", lambda: tb.LoadMeshes([api.Mesh(p, i, material=3)], materials))
    refused(E_UNSUPPORTED, "material 0 names a texture", lambda: tb.LoadMeshes([api.Mesh(p, i)], textured))
    refused(E_INVALID, "mesh 1: index 3 (triangle 0, corner 2) is at or past its 3 vertices", lambda: tb.LoadMeshes([api.Mesh(p, i), api.Mesh(p, bad)], materials))
    refused(E_INVALID, "mesh 0: the position of vertex 1 is not finite", lambda: tb.LoadMeshes([api.Mesh(nan, i)], materials))
    refused(E_INVALID, "environment texel 1 is not finite", lambda: tb.LoadMeshes([api.Mesh(p, i)], materials, environment=env))
    # device arrays: the same value checks after the one read; a pointer that is no device memory
    refused(E_INVALID, "mesh 0: index 3 (triangle 0, corner 2)", lambda: tb.LoadMeshes(mc.to_torch([api.Mesh(p, bad)]), materials))
    refused(E_INVALID, "mesh 0: the position of vertex 1 is not finite", lambda: tb.LoadMeshes(mc.to_torch([api.Mesh(nan, i)]), materials))
    d, keep = _desc([api.Mesh(p, i)], materials); d.flags = api.MESH_DEVICE                  # host pointers under TB_MESH_DEVICE
    refused(E_INVALID, "mesh 0: positions: ", lambda: tb._check(tb._L.tb_load_meshes(tb._ctx, C.byref(d))))
    short = api.Mesh(torch.zeros((3, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((1, 3), dtype=torch.int32, device="cuda:0"))
    d, keep, _ = api._scene_desc("test", [short], materials, None, None, (1, 1, 1), (0, 0), 0); d.meshes[0].n_vertices = 1 << 20
    refused(E_INVALID, "mesh 0: positions: the array runs past its allocation", lambda: tb._check(tb._L.tb_load_meshes(tb._ctx, C.byref(d))))
    # tb_recompute_normals
    refused(E_INVALID, "the vertex range runs past the scene's vertices", lambda: tb.RecomputeNormals(nv - 1, 2))
    refused(E_INVALID, "the vertex range runs past the scene's vertices", lambda: tb.RecomputeNormals(nv + 1, 0))
    tb.RecomputeNormals(nv, 0)
    assert tb.GetOption("dynamic_state") == 0                                                # n = 0 makes nothing
    with api.TracerBoy(0) as fresh:
        with pytest.raises(api.TracerBoyError) as e:
            fresh.RecomputeNormals(0, 1)
        assert e.value.code == E_NO_SCENE
        fresh.SetOption("flatten_instances", 0); fresh.LoadScene(dc.INSTANCED); fresh.SetOption("flatten_instances", 1)
        two_level = fresh.SceneDigest()
        with pytest.raises(api.TracerBoyError) as e:
            fresh.RecomputeNormals(0, 1)
        assert e.value.code == E_UNSUPPORTED and "two-level" in str(e.value) and fresh.SceneDigest() == two_level
        fresh.SetOption("bvh_builder", 1); fresh.SetOption("presplit", 50)
        slanted = api.Mesh(F32([[-8, -1, -8], [8, 3, 8], [8, -1.2, -8]]), np.uint32([[0, 1, 2]]))       # a large, empty box: the builder cuts it
        fresh.LoadMeshes(meshes + [slanted], materials)
        assert (fresh.HostSceneView().bvhBytes - 16 + 32) // 116 > fresh.SceneInfo().numTriangles
        presplit = fresh.SceneDigest()
        with pytest.raises(api.TracerBoyError) as e:
            fresh.RecomputeNormals(0, 1)
        assert e.value.code == E_UNSUPPORTED and "pre-split" in str(e.value) and fresh.SceneDigest() == presplit
    with api.TracerBoy(devices=[0, 0]) as group:
        group.LoadScene(CORNELL)
        both = group.SceneDigest()
        for call in (lambda: group.LoadMeshes(meshes, materials), lambda: group.RecomputeNormals(0, 1)):
            with pytest.raises(api.TracerBoyError) as e:
                call()
            assert e.value.code == E_UNSUPPORTED and "multi-device group" in str(e.value) and group.SceneDigest() == both
    unchanged()
