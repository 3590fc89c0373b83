"""Dynamic scenes (include/tracerboy_hip.h tb_update_positions .. tb_commit_geometry): vertices and instance transforms staged
and committed, the refit of the tree on the device.  The yardstick (refit_layout_a), the scenes and the seeds come from tests/dynamic_cases.py; the ray
sets are ray_query_cases' and the expected answers the CPU oracle's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dynamic_cases as dc
import ray_query_cases as rq
from conftest import ROOT

gpu = pytest.mark.gpu
W, H, FRAMES = 32, 24, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracerboy_hip.h")).read(), flags=re.S)


VERTEX_CALL = r"\bint\s+%s\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*\)"


def test_header_declares_the_calls_and_the_flags():
    h = _header()
    assert re.search(VERTEX_CALL % "tb_update_positions", h) and re.search(VERTEX_CALL % "tb_update_normals", h)
    assert re.search(r"\bint\s+tb_set_instance_transforms\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_commit_geometry\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", h)
    assert re.search(r"\bint\s+tb_geometry_vertex_range\s*\(\s*tb_context\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", h)
    assert re.search(r"#define\s+TB_UPDATE_DEVICE\s+0x100u\b", h) and re.search(r"#define\s+TB_RAYS_DEVICE\s+0x100u\b", h)
    assert re.search(r"#define\s+TB_GEOMETRY_REBUILD\s+1u\b", h)


def test_library_exports_and_binds_the_calls(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    raw = C.CDLL(api.LIB_PATH)
    bound = api.lib()
    vp, u32 = C.c_void_p, C.c_uint32
    want = {"tb_update_positions": [vp, u32, u32, u32, vp], "tb_update_normals": [vp, u32, u32, u32, vp], "tb_set_instance_transforms": [vp, u32, u32, vp],
            "tb_commit_geometry": [vp, u32], "tb_geometry_vertex_range": [vp, u32, C.POINTER(u32), C.POINTER(u32)]}
    for name, args in want.items():
        assert hasattr(raw, name) and name in bound._tb_exports, name
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == C.c_int, name
    assert (api.UPDATE_DEVICE, api.GEOMETRY_REBUILD) == (0x100, 1) == (abi.TB_UPDATE_DEVICE, abi.TB_GEOMETRY_REBUILD) and api.UPDATE_DEVICE == api.RAYS_DEVICE
    for method in ("UpdatePositions", "UpdateNormals", "SetInstanceTransforms", "CommitGeometry", "GeometryVertexRange"):
        assert callable(getattr(api.TracerBoy, method)), method


def test_updates_refuse_wrong_arrays_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    good = np.zeros((6, 3), np.float32)
    wrong = {
        "dtype float64": np.zeros((6, 3), np.float64),
        "dtype int32": np.zeros((6, 3), np.int32),
        "shape (n, 4)": np.zeros((6, 4), np.float32),
        "shape (n,)": np.zeros(18, np.float32),
        "three dimensions": np.zeros((2, 3, 3), np.float32),
        "a non-contiguous array": np.zeros((12, 3), np.float32)[::2],
        "a transposed array": np.zeros((3, 6), np.float32).T,
        "a list": [[0.0] * 3],
        "a tensor on the CPU": torch.zeros((6, 3), dtype=torch.float32),
        "a float64 tensor": torch.zeros((6, 3), dtype=torch.float64),
    }
    for update in (tb.UpdatePositions, tb.UpdateNormals):
        for what, a in wrong.items():
            with pytest.raises(ValueError):
                update(a)
                pytest.fail(what)
        for first in (-1, 1 << 32, (1 << 32) - 3, 1.5, None, True):
            with pytest.raises(ValueError):
                update(good, first)
                pytest.fail(repr(first))
        with pytest.raises(AttributeError):                         # the good array gets past the checks, to the library this object lacks
            update(good)
    for m in (np.zeros((2, 12), np.float64), np.zeros((2, 4, 3), np.float32), np.zeros(12, np.float32), np.zeros((4, 12), np.float32)[::2], [[0.0] * 12]):
        with pytest.raises(ValueError):
            tb.SetInstanceTransforms(m)
    with pytest.raises(ValueError):
        tb.SetInstanceTransforms(np.zeros((1, 12), np.float32), -1)
    with pytest.raises(AttributeError):
        tb.SetInstanceTransforms(np.zeros((1, 3, 4), np.float32))


def _host_scene(name):
    from tracerboy_amd import api
    path = dc.SCENES[name]
    return api.HostScene(path) if path else api.HostScene(procedural=(0, dc.PROC_TRIANGLES, dc.PROC_SEED))


@pytest.mark.parametrize("name", ["cornell", "proc10k"])
def test_yardstick_reproduces_the_loaded_tree_and_traces_like_a_rebuilt_one(built, settings, name):
    """refit_layout_a pinned without a GPU.  Unchanged positions: the image, byte for byte.  Displaced positions (DISPLACE_SEED, 5 % of the extent,
    the light's vertices kept): tbo_validate_bvh accepts the refit image, and tbo_trace_closest gives every ray of the set the GPU tests use the T
    it gives on tbo_build_lbvh2 of the displaced positions -- the condition on the inputs: 0 differing rays of the more than 4 000 of either set."""
    import oracle_lib as ol
    hs = _host_scene(name)
    view = hs.view(); image = dc.bvh_bytes(view)
    pos = dc.positions_of(view, image)
    tri = hs.triangles()
    named = np.zeros(len(pos), bool); named[tri["tri_vertex_index"].reshape(-1)] = True
    assert np.array_equal(pos[named].view(np.uint32), tri["positions"][named].view(np.uint32))   # the view gives the scene's own vertex numbering
    assert same_bytes(dc.refit_layout_a(view, pos), image)
    moved = dc.displaced(pos, 0.05, dc.DISPLACE_SEED, keep=dc.emissive_vertices(view))
    assert not np.array_equal(moved, pos)
    refit = dc.refit_layout_a(view, moved)
    assert not same_bytes(refit, image)
    sorted_tris = dc.tri_dict(view, refit, moved)
    rc, depth = ol.validate_bvh(refit, sorted_tris)
    assert rc == 0 and depth == hs.info().bvhMaxDepth
    rebuilt = ol.build_lbvh(dict(tri, positions=moved))
    assert ol.validate_bvh(rebuilt, dict(tri, positions=moved))[0] == 0
    a_view, b_view = dc.with_bvh(view, refit), dc.with_bvh(view, rebuilt)
    lo, hi = dc.bounds_of(view, refit)
    rays, on_refit = rq.build_rays(a_view, hs.frame_constants(settings), hs.camera().LensHeight, lo, hi)
    on_rebuilt = ol.trace_closest(b_view, rays["Origin"], rays["Direction"])
    assert len(rays) > 4000 and (on_refit["t"] > 0).sum() > 500
    assert int((on_refit["t"].view(np.uint32) != on_rebuilt["t"].view(np.uint32)).sum()) == 0


def test_yardstick_on_the_smallest_trees(built):
    """One, two and three triangles: root a leaf, one inner node, a leaf beside an inner node."""
    import oracle_lib as ol
    for name, depth in (("tri1", 1), ("tri2", 2), ("tri3", 3)):
        hs = _host_scene(name)
        view = hs.view(); image = dc.bvh_bytes(view); pos = dc.positions_of(view, image)
        assert hs.info().bvhMaxDepth == depth and same_bytes(dc.refit_layout_a(view, pos), image)
        for fraction, seed in ((0.05, dc.DISPLACE_SEED), (1.0, dc.DISPLACE_SEED_FAR)):
            moved = dc.displaced(pos, fraction, seed)
            refit = dc.refit_layout_a(view, moved)
            assert ol.validate_bvh(refit, dc.tri_dict(view, refit, moved)) == (0, depth)


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dyn_tb(built):
    """A context of this module's own: the tests move its scenes and load under options the session's context must not keep."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    yield tb
    tb.close()


def load(tb, name, **options):
    """A fresh load of the scene (no dynamic state, no staged data), under `options`, which then go back to their defaults."""
    for k, v in options.items():
        tb.SetOption(k, v)
    try:
        if name == "instanced":
            tb.SetOption("flatten_instances", 0)
            tb.LoadScene(dc.INSTANCED)
        else:
            tb.LoadScene(dc.SCENES[name]) if dc.SCENES[name] else tb.LoadProcedural(0, dc.PROC_TRIANGLES, dc.PROC_SEED)
    finally:
        tb.SetOption("flatten_instances", 1)
    view = tb.HostSceneView()
    image = dc.bvh_bytes(view)                                       # (a two-level scene's: the bottom-level images back to back)
    return view, image, None if name == "instanced" else dc.positions_of(view, image)


def moved_positions(view, pos, fraction=0.05, seed=dc.DISPLACE_SEED):
    return dc.displaced(pos, fraction, seed, keep=dc.emissive_vertices(view))


def rays_of(tb, settings):
    """ray_query_cases' ray set for the scene as the context holds it now, and the oracle's closest hits on the context's own view."""
    view = tb.HostSceneView()
    lo, hi = dc.bounds_of(view, dc.bvh_bytes(view))
    return rq.build_rays(view, tb.FrameConstants(64, 48, 0, settings, 0.0), tb.GetCamera().LensHeight, lo, hi)


def render(tb, settings):
    tb.InvalidateHistory()
    tb.Render(W, H, FRAMES, settings, 0.0)
    return tb.ReadAccumulation().copy()


def oracle_render(tb, settings):
    import oracle_lib as ol
    return ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, settings, 0.0), W, H, FRAMES, threads=8)["output"]


@gpu
@pytest.mark.parametrize("name", list(dc.SCENES))
def test_refit_boxes_are_the_fit_rule_bit_for_bit(dyn_tb, name):
    """Every vertex (the light's kept) displaced by 5 % of the extent, then by 100 %: the context's layout-A image after the commit is the yardstick's
    refit of the image before it, byte for byte, and tbo_validate_bvh accepts it."""
    import oracle_lib as ol
    view, image, pos = load(dyn_tb, name)
    assert dyn_tb.GetOption("dynamic_state") == 0
    depth = dyn_tb.SceneInfo().bvhMaxDepth
    for fraction, seed in ((0.05, dc.DISPLACE_SEED), (1.0, dc.DISPLACE_SEED_FAR)):
        new = moved_positions(view, pos, fraction, seed)
        dyn_tb.UpdatePositions(new); dyn_tb.CommitGeometry()
        assert dyn_tb.GetOption("host_geometry_stale") == (1 if name == "proc10k" else 0)   # an LDS-resident scene's image needs the host tree at once
        view = dyn_tb.HostSceneView(); got = dc.bvh_bytes(view)
        assert dyn_tb.GetOption("host_geometry_stale") == 0
        want = dc.refit_layout_a(view, new, image=image)
        assert same_bytes(got, want) and not same_bytes(got, image)
        assert ol.validate_bvh(got, dc.tri_dict(view, got, new)) == (0, depth)
        info = dyn_tb.SceneInfo()
        named = np.zeros(len(new), bool); named[dc.sorted_tri_vertices(view, got).reshape(-1)] = True
        lo, hi = dc.bounds_of(view, got)                             # the bounds follow (a vertex no triangle names keeps its place in them)
        assert (np.float32(info.sceneMin[:]) <= lo).all() and (np.float32(info.sceneMax[:]) >= hi).all()
        assert not named.all() or (np.array_equal(np.float32(info.sceneMin[:]), lo) and np.array_equal(np.float32(info.sceneMax[:]), hi))
        image, pos = got, new


@gpu
@pytest.mark.parametrize("form", ["0", "1"])
def test_both_forms_of_the_bottom_up_pass_give_the_same_bytes(dyn_tb, monkeypatch, form):
    """TB_REFIT_FORM = 0, one launch per level, and 1, the top levels fused into one workgroup (what ships): on the 10 k-triangle tree, 25 levels deep, whose
    upper levels the fused launch takes, and on the three-triangle tree, whose two levels are too few to fuse."""
    monkeypatch.setenv("TB_REFIT_FORM", form)
    for name in ("proc10k", "tri3"):
        view, image, pos = load(dyn_tb, name)
        new = moved_positions(view, pos, 1.0, dc.DISPLACE_SEED_FAR)
        dyn_tb.UpdatePositions(new); dyn_tb.CommitGeometry()
        assert same_bytes(dc.bvh_bytes(dyn_tb.HostSceneView()), dc.refit_layout_a(view, new, image=image))


@gpu
@pytest.mark.parametrize("name", ["cornell", "proc10k"])
def test_moving_back_restores_the_loaded_scene(dyn_tb, settings, name):
    view, image, pos = load(dyn_tb, name)
    digest = dyn_tb.SceneDigest(); before = render(dyn_tb, settings)
    dyn_tb.UpdatePositions(moved_positions(view, pos)); dyn_tb.CommitGeometry()
    assert dyn_tb.SceneDigest() != digest
    dyn_tb.UpdatePositions(pos); dyn_tb.CommitGeometry()
    assert same_bytes(dc.bvh_bytes(dyn_tb.HostSceneView()), image) and dyn_tb.SceneDigest() == digest
    assert same_bytes(render(dyn_tb, settings), before)


@gpu
@pytest.mark.parametrize("name", ["tri3", "cornell", "proc10k"])
def test_hits_on_the_moved_scene_are_the_oracles_and_a_rebuilt_trees(dyn_tb, settings, name):
    import torch
    from tracerboy_amd import api
    view, image, pos = load(dyn_tb, name)
    dyn_tb.UpdatePositions(moved_positions(view, pos)); dyn_tb.CommitGeometry()
    rays, oracle = rays_of(dyn_tb, settings)
    want = rq.expected_hits(rays, oracle)
    got = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST)
    for field in api.QUERY_HIT_DTYPE.names:
        assert same_bytes(got[field], want[field]), field
    assert (got["T"] > 0).sum() > (20 if name == "tri3" else 500)
    on_device = dyn_tb.TraceRays(torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0"), api.RAYS_CLOSEST)
    assert same_bytes(on_device.cpu().numpy().view(api.QUERY_HIT_DTYPE).reshape(-1), got)
    occluded = dyn_tb.TraceRays(rays, api.RAYS_OCCLUDED)
    compare = ~rq.near_tmax(rays, oracle)
    assert np.array_equal(occluded[compare], rq.expected_occluded(rays, oracle)[compare])
    dyn_tb.CommitGeometry(rebuild=True)                               # nothing staged: the refit tree is built again
    assert dyn_tb.GetOption("dynamic_state") == 0
    rebuilt = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST)
    assert np.array_equal(rebuilt["T"].view(np.uint32), got["T"].view(np.uint32))


@gpu
@pytest.mark.parametrize("name,node_layout", [("cornell", 0), ("proc10k", 0), ("proc10k", 1)])
def test_render_of_the_moved_scene_is_the_oracles(dyn_tb, settings, name, node_layout):
    """cornell-box renders from the rebuilt LDS image, the procedural scene from memory, and with node_layout = 1 from the rebuilt layout C."""
    view, image, pos = load(dyn_tb, name)
    dyn_tb.SetOption("node_layout", node_layout)
    try:
        before = render(dyn_tb, settings)
        assert dyn_tb.GetOption("last_node_layout") == node_layout
        dyn_tb.UpdatePositions(moved_positions(view, pos)); dyn_tb.CommitGeometry()
        after = render(dyn_tb, settings)
        assert dyn_tb.GetOption("last_node_layout") == node_layout
    finally:
        dyn_tb.SetOption("node_layout", 0)
    assert not same_bytes(after, before)
    assert same_bytes(after, oracle_render(dyn_tb, settings))


@gpu
def test_partial_host_and_device_updates_are_one_whole_update(dyn_tb, settings):
    import torch
    from tracerboy_amd import api
    view, image, pos = load(dyn_tb, "proc10k")
    new = moved_positions(view, pos)
    rays, oracle = rays_of(dyn_tb, settings)
    old = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST)
    dyn_tb.UpdatePositions(new); dyn_tb.CommitGeometry()
    whole = dc.bvh_bytes(dyn_tb.HostSceneView())
    view, image, pos = load(dyn_tb, "proc10k")
    half = len(new) // 2 + 1
    dyn_tb.UpdatePositions(np.ascontiguousarray(new[:half]), 0)
    dyn_tb.UpdatePositions(torch.from_numpy(new[half:].copy()).to("cuda:0"), half)
    assert dyn_tb.GetOption("dynamic_state") == 1
    assert same_bytes(dyn_tb.TraceRays(rays, api.RAYS_CLOSEST), old)  # staged data has no effect before the commit
    assert same_bytes(dc.bvh_bytes(dyn_tb.HostSceneView()), image)
    dyn_tb.CommitGeometry()
    assert same_bytes(dc.bvh_bytes(dyn_tb.HostSceneView()), whole)
    assert not same_bytes(dyn_tb.TraceRays(rays, api.RAYS_CLOSEST), old)


@gpu
def test_device_updates_in_a_context_that_has_rendered_nothing(built):
    """Two device updates in a row, a commit and a trace in a fresh context: between them Python waits with tb_sync, which leaves the runtime's
    error of a never-recorded event behind; the launchers must not take it for their own."""
    import torch
    from tracerboy_amd import api
    with api.TracerBoy(0) as tb:
        view, image, pos = load(tb, "tri3")
        new = moved_positions(view, pos)
        tb.UpdatePositions(torch.from_numpy(new[:1].copy()).to("cuda:0"))
        tb.UpdatePositions(torch.from_numpy(new.copy()).to("cuda:0"))
        tb.UpdateNormals(torch.from_numpy(np.float32([[0.0, 0.0, 1.0]])).to("cuda:0"), 2)
        tb.CommitGeometry()
        assert same_bytes(dc.bvh_bytes(tb.HostSceneView()), dc.refit_layout_a(view, new, image=image))


@gpu
@pytest.mark.parametrize("name", ["cornell", "proc10k"])
def test_new_normals_change_the_shading_and_no_distance(dyn_tb, settings, name):
    from tracerboy_amd import api
    view, image, pos = load(dyn_tb, name)
    rays, oracle = rays_of(dyn_tb, settings)
    old = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST)
    rng = np.random.default_rng(dc.NORMAL_SEED)
    normals = rng.normal(size=pos.shape); normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    light = dc.emissive_vertices(view)
    vb = np.ctypeslib.as_array(view.vertexBuffer, shape=(view.numVertexFloats // 8, 8)).copy()
    normals[light] = vb[light, 0:3]
    dyn_tb.UpdateNormals(normals); dyn_tb.CommitGeometry()
    view = dyn_tb.HostSceneView()
    now = np.ctypeslib.as_array(view.vertexBuffer, shape=(view.numVertexFloats // 8, 8))
    assert same_bytes(now[:, 0:3].copy(), normals) and same_bytes(now[:, 3:].copy(), vb[:, 3:].copy())   # UVs and tangents stay
    assert same_bytes(dc.bvh_bytes(view), image)
    new = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST)
    for field in ("T", "U", "V", "Prim", "Geom", "Material", "UV"):
        assert same_bytes(new[field], old[field]), field
    assert not same_bytes(new["Normal"], old["Normal"])
    import oracle_lib as ol
    want = rq.expected_hits(rays, ol.trace_closest(view, rays["Origin"], rays["Direction"]))
    assert same_bytes(new["Normal"], want["Normal"])
    assert same_bytes(render(dyn_tb, settings), oracle_render(dyn_tb, settings))


def _instances(view):
    """The top level's metadata by instance, and every instance's bottom-level root box (min, max)."""
    from tracerboy_amd import _ctypes_abi as abi
    tl = dc.tlas_bytes(view).tobytes(); bvh = dc.bvh_bytes(view)
    off_meta = int(np.frombuffer(tl, np.uint32, 1, 4)[0])
    md = sorted((abi.TbBvhMetadata.from_buffer_copy(tl, off_meta + 116 * k) for k in range(view.numInstances)), key=lambda m: m.InstanceIndex)
    roots = []
    for m in md:
        root = bvh[view.blasOffsets[m.BlasIndex] + 16:view.blasOffsets[m.BlasIndex] + 48].view(np.float32)
        roots.append(np.concatenate([root[0:3] - root[4:7], root[0:3] + root[4:7]]))
    return md, np.array(roots, np.float32)


@gpu
def test_instance_transforms_rebuild_the_top_level(dyn_tb, settings):
    """A translation, a rotation and a non-uniform scale on the instanced fixture: the top-level image is tbo_build_tlas of the new transforms, hits and
    a small render are the oracle's, and the loaded transforms bring back the loaded bytes."""
    import oracle_lib as ol
    from tracerboy_amd import api
    view, image, _ = load(dyn_tb, "instanced")
    assert view.numInstances == 3
    loaded = dc.tlas_bytes(view); digest = dyn_tb.SceneDigest(); before = render(dyn_tb, settings)
    md, roots = _instances(view)
    o2w = np.array([m.ObjectToWorld[:] for m in md], np.float32).reshape(3, 3, 4)
    new = o2w.copy()
    new[0, :, 3] += np.float32([0.0, 0.25, -0.5])                                            # the world-level shapes: a translation
    a = np.float32(np.deg2rad(50.0)); rot = np.float32([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    new[1, :, :3] = (rot @ new[1, :, :3]).astype(np.float32)                                  # a rotation
    new[2, :, :3] = (new[2, :, :3] * np.float32([1.5, 0.6, 2.0])).astype(np.float32)          # a non-uniform scale
    new[2, :, 3] += np.float32([-0.4, 0.3, 0.2])
    dyn_tb.SetInstanceTransforms(np.ascontiguousarray(new[:1]), 0)
    dyn_tb.SetInstanceTransforms(np.ascontiguousarray(new[1:].reshape(2, 12)), 1)
    assert same_bytes(dc.tlas_bytes(dyn_tb.HostSceneView()), loaded)                          # staged only
    dyn_tb.CommitGeometry()
    view = dyn_tb.HostSceneView()
    want = ol.build_tlas(new.reshape(3, 12), roots, [m.BlasIndex for m in md], [m.InstanceContributionToHitGroupIndexAndFlags & 0xFFFFFF for m in md])
    assert same_bytes(dc.tlas_bytes(view), want) and not same_bytes(want, loaded)
    assert same_bytes(dc.bvh_bytes(view), image) and dyn_tb.SceneDigest() != digest           # the bottom levels are untouched
    info = dyn_tb.SceneInfo()
    rays, oracle = rq.build_rays(view, dyn_tb.FrameConstants(64, 48, 0, settings, 0.0), dyn_tb.GetCamera().LensHeight, info.sceneMin[:], info.sceneMax[:])
    got = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST); expect = rq.expected_hits(rays, oracle)
    for field in api.QUERY_HIT_DTYPE.names:
        assert same_bytes(got[field], expect[field]), field
    after = render(dyn_tb, settings)
    assert same_bytes(after, oracle_render(dyn_tb, settings)) and not same_bytes(after, before)
    dyn_tb.SetInstanceTransforms(np.ascontiguousarray(o2w))
    dyn_tb.CommitGeometry()
    assert same_bytes(dc.tlas_bytes(dyn_tb.HostSceneView()), loaded) and dyn_tb.SceneDigest() == digest
    assert same_bytes(render(dyn_tb, settings), before)


def _refused(code, text, call, *args):
    from tracerboy_amd import api
    with pytest.raises(api.TracerBoyError) as e:
        call(*args)
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


@gpu
def test_refusals_leave_the_scene_as_it_was(built, dyn_tb, settings):
    import torch
    from tracerboy_amd import api
    INVALID, UNSUPPORTED, NO_SCENE = -1, -6, -7
    three = np.zeros((3, 3), np.float32)
    fresh = api.TracerBoy(0)
    try:                                                            # no scene
        for call, args in ((fresh.UpdatePositions, (three,)), (fresh.UpdateNormals, (three,)), (fresh.CommitGeometry, ()), (fresh.GeometryVertexRange, (0,)),
                           (fresh.SetInstanceTransforms, (np.zeros((1, 12), np.float32),))):
            _refused(NO_SCENE, "no scene", call, *args)
    finally:
        fresh.close()
    group = api.TracerBoy(devices=[0, 0])
    try:                                                            # a group context
        group.LoadScene(dc.SCENES["tri3"])
        for call, args in ((group.UpdatePositions, (three,)), (group.UpdateNormals, (three,)), (group.CommitGeometry, ()),
                           (group.SetInstanceTransforms, (np.zeros((1, 12), np.float32),))):
            _refused(UNSUPPORTED, "multi-device group", call, *args)
    finally:
        group.close()

    view, image, pos = load(dyn_tb, "cornell")
    rays, oracle = rays_of(dyn_tb, settings)
    answers = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST)

    def unchanged():
        return same_bytes(dyn_tb.TraceRays(rays, api.RAYS_CLOSEST), answers) and same_bytes(dc.bvh_bytes(dyn_tb.HostSceneView()), image)

    n = len(pos)
    for update in (dyn_tb.UpdatePositions, dyn_tb.UpdateNormals):
        _refused(INVALID, "past the scene's vertices", update, pos, 1)
        _refused(INVALID, "past the scene's vertices", update, three, n - 2)
        bad = pos.copy(); bad[5, 1] = np.nan
        _refused(INVALID, "not finite", update, bad)
        bad[5, 1] = np.inf
        _refused(INVALID, "not finite", update, bad)
    for fn in (dyn_tb._L.tb_update_positions, dyn_tb._L.tb_update_normals):
        assert fn(dyn_tb._ctx, 0, 0, 3, None) == INVALID and fn(dyn_tb._ctx, 2, 0, 3, three.ctypes.data) == INVALID      # a null pointer; an unknown flag
        assert fn(dyn_tb._ctx, api.UPDATE_DEVICE, 0, 3, three.ctypes.data) == INVALID                                    # a host pointer passed as a device pointer
    assert dyn_tb._L.tb_commit_geometry(dyn_tb._ctx, 2) == INVALID
    _refused(UNSUPPORTED, "no instances", dyn_tb.SetInstanceTransforms, np.zeros((1, 12), np.float32))
    _refused(INVALID, "out of range", dyn_tb.GeometryVertexRange, view.numHitGroups)
    dyn_tb.CommitGeometry()                                         # nothing was staged by any of them
    assert unchanged() and dyn_tb.GetOption("dynamic_state") == 0

    # a vertex of the light quad: refused at the commit, the geometry named; the staged data stays, so the light's own position makes it good again
    light = np.flatnonzero(dc.emissive_vertices(view))
    geometry = [g for g in range(view.numHitGroups) if dyn_tb.GeometryVertexRange(g) == (int(light[0]), len(light))]
    assert len(light) == 4 and len(geometry) == 1
    moved = pos[light[1]:light[1] + 1] + np.float32([0.0, -0.125, 0.0])
    dyn_tb.UpdatePositions(moved, int(light[1]))
    _refused(UNSUPPORTED, "geometry %d" % geometry[0], dyn_tb.CommitGeometry)
    assert unchanged()
    _refused(UNSUPPORTED, "geometry %d" % geometry[0], dyn_tb.CommitGeometry)
    dyn_tb.UpdatePositions(torch.from_numpy(pos[light[1]:light[1] + 1].copy()).to("cuda:0"), int(light[1]))
    dyn_tb.CommitGeometry()
    assert unchanged()
    dyn_tb.UpdateNormals(np.float32([[0.0, 1.0, 0.0]]), int(light[2]))
    _refused(UNSUPPORTED, "geometry %d" % geometry[0], dyn_tb.CommitGeometry)

    view, image, _ = load(dyn_tb, "instanced")                       # a two-level scene
    info = dyn_tb.SceneInfo()
    rays, oracle = rq.build_rays(view, dyn_tb.FrameConstants(64, 48, 0, settings, 0.0), dyn_tb.GetCamera().LensHeight, info.sceneMin[:], info.sceneMax[:])
    answers = dyn_tb.TraceRays(rays, api.RAYS_CLOSEST); loaded = dc.tlas_bytes(view)
    _refused(UNSUPPORTED, "two-level", dyn_tb.UpdatePositions, three)
    _refused(UNSUPPORTED, "two-level", dyn_tb.UpdateNormals, three)
    identity = np.float32([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]])
    _refused(INVALID, "past the scene's instances", dyn_tb.SetInstanceTransforms, np.repeat(identity, 4, axis=0))
    _refused(INVALID, "past the scene's instances", dyn_tb.SetInstanceTransforms, identity, 3)
    singular = identity.copy(); singular[0, 10] = 0.0
    _refused(INVALID, "singular", dyn_tb.SetInstanceTransforms, singular)
    flat = identity.copy(); flat[0, 4:8] = flat[0, 0:4]
    _refused(INVALID, "singular", dyn_tb.SetInstanceTransforms, flat, 1)
    nan = identity.copy(); nan[0, 3] = np.nan
    _refused(INVALID, "not finite", dyn_tb.SetInstanceTransforms, nan)
    assert dyn_tb._L.tb_set_instance_transforms(dyn_tb._ctx, 0, 1, None) == INVALID
    dyn_tb.CommitGeometry()
    assert same_bytes(dyn_tb.TraceRays(rays, api.RAYS_CLOSEST), answers) and same_bytes(dc.tlas_bytes(dyn_tb.HostSceneView()), loaded)


@gpu
def test_a_commit_resets_the_history_and_an_empty_one_does_not(dyn_tb, settings, tmp_path):
    from tracerboy_amd import api
    view, image, pos = load(dyn_tb, "cornell")
    dyn_tb.InvalidateHistory(); dyn_tb.Render(W, H, FRAMES, settings, 0.0)
    state = str(tmp_path / "before.tbstate"); dyn_tb.SaveState(state)
    digest = dyn_tb.SceneDigest()
    dyn_tb.CommitGeometry()                                         # no dynamic state at all
    assert dyn_tb.GetNumberOfSamplesSinceLastInvalidate() == FRAMES and dyn_tb.SceneDigest() == digest
    dyn_tb.UpdatePositions(pos[:0]); dyn_tb.CommitGeometry()        # an update of no vertex stages nothing
    assert dyn_tb.GetNumberOfSamplesSinceLastInvalidate() == FRAMES and dyn_tb.SceneDigest() == digest
    dyn_tb.LoadState(state)
    assert dyn_tb.GetNumberOfSamplesSinceLastInvalidate() == FRAMES
    dyn_tb.UpdatePositions(moved_positions(view, pos)); dyn_tb.CommitGeometry()
    assert dyn_tb.GetNumberOfSamplesSinceLastInvalidate() == 0 and dyn_tb.SceneDigest() != digest
    _refused(-1, "scene_digest", dyn_tb.LoadState, state)
    assert dyn_tb.GetNumberOfSamplesSinceLastInvalidate() == 0
