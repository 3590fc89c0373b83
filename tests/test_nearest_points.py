"""Point queries (include/tracerboy_hip.h tb_nearest_points, tb_bake_distance_field; the rule: include/tb_nearest.h): the
nearest surface point of a scene to a point, by a distance-ordered walk on the device, against the host's statement of the same rule (bit for bit)
and against geometry (a float64 brute force by another method, tests/nearest_cases.py).  Scenes: the adversarial soups of tests/adversarial_cases.py
under the builders tests/test_adversarial_meshes.py runs, cornell-box, the 40 000-triangle procedural scene."""
import numpy as np
import pytest

import adversarial_cases as ac
import dynamic_cases as dc
import mesh_cases as mc
import nearest_cases as nc
import ray_query_cases as rq
from conftest import CORNELL

gpu = pytest.mark.gpu
HOST_BUILDERS = (0, 1, 3)             # as tests/test_adversarial_meshes.py: LBVH, the SAH builder, LBVH + treelet passes
WALK_BUILDERS = (0, 1, 3, 4)          # and the treelet passes on the device
MOVED = ("rand64", "sliver64", "flat512", "rand512", "expo40")
INVALID, UNSUPPORTED, NO_SCENE = -1, -6, -7
INF = np.float32(np.inf)


def same_bytes(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def meshes_of(tri):
    from tracerboy_amd import api
    p, i = ac.soup(tri)
    return [api.Mesh(p, i)]


_hosts = {}


def host(name, builder, moved=False):
    """The case -- its partner's positions with `moved` -- built on the host, made once"""
    from tracerboy_amd import api
    key = (name, builder, moved)
    if key not in _hosts:
        _hosts[key] = api.HostScene.from_meshes(meshes_of(ac.partner(name) if moved else ac.triangles(name)), mc.MATERIALS(), bvh_builder=builder)
    return _hosts[key]


def query_points(name, moved=False, seed=nc.POINT_SEED):
    from tracerboy_amd import api
    pos, maxd, kinds = nc.case_points(name + ("/moved" if moved else ""), ac.partner(name) if moved else ac.triangles(name), seed)
    return api.make_query_points(pos, maxd), kinds


_brute = {}


def brute(name, moved=False, signed=False):
    """The host brute force's records of the case's points: the expectation of every walk, made once and left unchanged"""
    key = (name, moved, signed)
    if key not in _brute:
        pts, _ = query_points(name, moved)
        _brute[key] = host(name, 0, moved).nearest(pts, signed=signed)
        _brute[key].setflags(write=False)
    return _brute[key]


def is_miss(rec):
    return (rec["Prim"] == 0xffffffff) & (rec["Geom"] == 0xffffffff)


def check_misses(rec):
    m = is_miss(rec)
    assert (rec["Distance"][m] == INF).all() and not rec["Point"][m].any() and not rec["U"][m].any() and not rec["V"][m].any()
    assert np.isfinite(rec["Distance"][~m]).all() and np.isfinite(rec["Point"][~m]).all()


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def test_records_and_packing(built):
    from tracerboy_amd import api
    assert api.QUERY_POINT_DTYPE.itemsize == 16 and api.NEAREST_DTYPE.itemsize == 32
    p = api.make_query_points(np.arange(12).reshape(4, 3), [1.0, np.inf, 0.0, 2.5])
    flat = p.view(np.float32).reshape(4, 4)
    assert np.array_equal(flat[:, :3], np.arange(12, dtype=np.float32).reshape(4, 3)) and flat[:, 3].tolist() == [1.0, np.inf, 0.0, 2.5]
    assert np.isinf(api.make_query_points(np.zeros((3, 3)))["MaxDistance"]).all()
    with pytest.raises(ValueError):
        api.make_query_points(np.zeros((3, 2)))


def test_known_answers_on_one_triangle(built):
    """v0 = (0, 0, 0), v1 = (4, 0, 0), v2 = (0, 4, 0): one point in each of the seven regions, every number exact in binary32."""
    from tracerboy_amd import api
    tri = np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]])
    cases = [  # point, Point, U, V, Distance
        ((-3, -4, 0), (0, 0, 0), 0.0, 0.0, 5.0),        # vertex 0
        ((7, -4, 0), (4, 0, 0), 1.0, 0.0, 5.0),         # vertex 1
        ((-4, 7, 0), (0, 4, 0), 0.0, 1.0, 5.0),         # vertex 2
        ((1, -3, 4), (1, 0, 0), 0.25, 0.0, 5.0),        # edge AB
        ((-3, 1, 4), (0, 1, 0), 0.0, 0.25, 5.0),        # edge AC
        ((5, 3, 1), (3, 1, 0), 0.75, 0.25, 3.0),        # edge BC
        ((1, 1, 3), (1, 1, 0), 0.25, 0.25, 3.0),        # interior, above
        ((1, 1, -3), (1, 1, 0), 0.25, 0.25, 3.0),       # interior, below
    ]
    pts = api.make_query_points(np.float32([c[0] for c in cases]))
    for builder in HOST_BUILDERS:
        hs = api.HostScene.from_meshes(meshes_of(tri), mc.MATERIALS(), bvh_builder=builder)
        for walk in (False, True):
            got = hs.nearest(pts, walk=walk)
            signed = hs.nearest(pts, signed=True, walk=walk)
            for k, (_, point, u, v, d) in enumerate(cases):
                assert got["Point"][k].tolist() == list(point) and (got["U"][k], got["V"][k], got["Distance"][k]) == (u, v, d), (k, got[k])
                assert (got["Prim"][k], got["Geom"][k]) == (0, 0)
            assert signed["Distance"].tolist() == [5.0, 5.0, 5.0, 5.0, 5.0, 3.0, 3.0, -3.0]        # the face vector is +z; on the plane: positive
            for f in ("Point", "U", "V", "Prim", "Geom"):
                assert same_bytes(signed[f], got[f])


def cube():
    """the unit cube, 12 triangles wound so that every face vector points outward"""
    corners = np.float32([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])            # index = 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x, +x, -y, +y, -z, +z
    tri = np.float32([[corners[q[0]], corners[q[a]], corners[q[a + 1]]] for q in quads for a in (1, 2)])
    face = np.cross(tri[:, 2] - tri[:, 0], tri[:, 2] - tri[:, 1])                                # tb_face_vector
    assert ((face * (tri.mean(axis=1) - 0.5)).sum(-1) > 0).all()
    return tri


def test_signed_distance_of_a_unit_cube(built):
    """A convex closed mesh: the side of the nearest triangle is the exact inside test.  Coordinates are multiples of 1 / 8, so every distance to a
    face, an edge or a corner is computed without a rounding that could change a sign; points ON the surface are positive (+0)."""
    from tracerboy_amd import api
    tri = cube()
    g = np.float32([-0.5, -0.125, 0.0, 0.125, 0.5, 0.875, 1.0, 1.125, 1.5])
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    inside = ((pos > 0) & (pos < 1)).all(axis=1)
    outside = ((pos < 0) | (pos > 1)).any(axis=1)
    on = ~inside & ~outside
    assert inside.sum() == 27 and on.sum() == 125 - 27 and outside.sum() == 729 - 125
    lo = np.maximum(np.maximum(-pos, pos - 1), 0).astype(np.float64)                              # exact distance to the cube
    want = np.where(inside, -np.minimum(pos, 1 - pos).min(axis=1), np.sqrt((lo * lo).sum(-1)))
    pts = api.make_query_points(pos)
    for builder in HOST_BUILDERS:
        hs = api.HostScene.from_meshes(meshes_of(tri), mc.MATERIALS(), bvh_builder=builder)
        for walk in (False, True):
            got = hs.nearest(pts, signed=True, walk=walk)
            d = got["Distance"]
            assert (d[inside] < 0).all() and (d[outside] > 0).all()
            assert (d[on] == 0).all() and not np.signbit(d[on]).any()
            assert np.allclose(d, want, rtol=2e-7, atol=0)
            assert same_bytes(np.abs(d), hs.nearest(pts, walk=walk)["Distance"])


@pytest.mark.parametrize("name", ac.NAMES)
def test_host_walk_is_the_brute_force_bit_for_bit(built, name):
    """The test of the pruning slack: the kernel's walk as scalar C++ over every builder's tree gives the 32 bytes of the brute force per point.
    In same70 and split65 every point has 33 to 70 triangles at one D2 and the tie-break decides every record; zero32 has triangles of no area."""
    pts, kinds = query_points(name)
    for signed in (False, True):
        want = brute(name, signed=signed)
        check_misses(want)
        for builder in HOST_BUILDERS:
            got = host(name, builder).nearest(pts, signed=signed, walk=True)
            assert same_bytes(got, want), (builder, signed, np.flatnonzero(got != want)[:8])
            if builder:
                assert same_bytes(host(name, builder).nearest(pts, signed=signed), want)          # the triangle SET decides, not its order
    if name in ("same70", "split65"):
        tri = ac.triangles(name)
        found = ~is_miss(want)
        first = np.array([np.flatnonzero((tri == tri[k]).all(axis=(1, 2)))[0] for k in want["Prim"][found]])
        assert (want["Prim"][found] == first).all()                                                # of equal triangles the lowest number wins


@pytest.mark.parametrize("name", [n for n in ac.NAMES if n != "zero32"])
def test_host_brute_force_is_the_geometrys(built, name):
    """Against the float64 brute force by another method: |Distance - d64| <= DISTANCE_C 2^-23 M aspect(Prim) for EVERY record, the aspect scaling
    being the only allowance; which points miss is what their kind says; Point is (v0 + (v1 - v0) U) + (v2 - v0) V of the case's corners on
    bits; the weights lie in the triangle."""
    tri = ac.triangles(name)
    for seed in (nc.POINT_SEED, nc.POINT_SEED + 1, nc.POINT_SEED + 2):
        pts, kinds = query_points(name, seed=seed)
        got = host(name, 0).nearest(pts)
        check_misses(got)
        miss = is_miss(got)
        expect_miss = np.isin(kinds, ("zero", "nan", "negative", "half", "not_finite"))
        assert np.array_equal(miss, expect_miss), (kinds[miss != expect_miss][:8])
        f = ~miss
        pos = pts["Position"][f]
        d64 = nc.distance64(tri, pos)
        bound = nc.DISTANCE_C * nc.ULP * nc.scale(tri, pos) * nc.aspect(tri)[got["Prim"][f]]
        err = np.abs(got["Distance"][f].astype(np.float64) - d64)
        print(name, seed, "worst |Distance - d64| / (2^-23 M aspect):", float((err / (bound / nc.DISTANCE_C)).max()))
        assert (err <= bound).all(), (np.flatnonzero(err > bound)[:8], err.max())
        assert (got["Geom"][f] == 0).all() and (got["Prim"][f] < len(tri)).all()
        v = tri[got["Prim"][f]]
        u_, v_ = got["U"][f][:, None], got["V"][f][:, None]
        point = (v[:, 0] + (v[:, 1] - v[:, 0]) * u_) + (v[:, 2] - v[:, 0]) * v_
        assert point.dtype == np.float32 and same_bytes(point, got["Point"][f])
        assert (got["U"][f] >= 0).all() and (got["V"][f] >= 0).all()
        assert (got["U"][f].astype(np.float64) + got["V"][f].astype(np.float64) <= 1 + 2.0 ** -22).all()


@pytest.mark.parametrize("name", ac.NAMES)
def test_candidate_rule_at_the_found_distance(built, name):
    """MaxDistance = the Distance found: the same record.  MaxDistance = the next float below it: a MISS -- the header's rule counts a triangle iff
    the Distance of its record is <= MaxDistance, the winner's is now above it, and a triangle whose Distance is smaller would have won before."""
    from tracerboy_amd import api
    pts, kinds = query_points(name)
    want = brute(name)
    f = ~is_miss(want)
    at = api.make_query_points(pts["Position"][f], want["Distance"][f])
    below = api.make_query_points(pts["Position"][f], np.nextafter(want["Distance"][f], -INF))
    for walk in (False, True):
        for builder in HOST_BUILDERS if walk else (0,):
            assert same_bytes(host(name, builder).nearest(at, walk=walk), want[f])
            assert is_miss(host(name, builder).nearest(below, walk=walk)).all()


def test_refusals_of_the_arguments(built):
    from tracerboy_amd import api
    from tracerboy_amd import _ctypes_abi as abi
    assert api.NearestRefusal(0, 4, 64, 128) is None and api.NearestRefusal(api.NEAREST_SIGNED | api.NEAREST_DEVICE, 4, 64, 128) is None
    assert api.NearestRefusal(0, 0, 0, 0) is None                                                  # n = 0 needs no pointers
    assert "flag" in api.NearestRefusal(2, 4, 64, 128) and "flag" in api.NearestRefusal(api.NEAREST_HOST_WALK, 4, 64, 128)
    assert "2^31" in api.NearestRefusal(0, (1 << 31) + 1, 64, 128) and api.NearestRefusal(0, 1 << 31, 64, 128) is None
    assert "null" in api.NearestRefusal(0, 4, 0, 128) and "null" in api.NearestRefusal(0, 4, 64, 0)
    assert "aligned" in api.NearestRefusal(api.NEAREST_DEVICE, 4, 72, 128) and "aligned" in api.NearestRefusal(api.NEAREST_DEVICE, 4, 64, 136)
    assert api.NearestRefusal(0, 4, 72, 136) is None                                               # host arrays need no alignment

    def grid(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 3, 4)):
        return abi.tb_probe_grid((abi.C.c_float * 3)(*origin), (abi.C.c_float * 3)(*spacing), (abi.C.c_uint32 * 3)(*count))
    assert api.NearestRefusal(0, 0, 0, 64, grid()) is None
    assert "flag" in api.NearestRefusal(4, 0, 0, 64, grid())
    assert "count" in api.NearestRefusal(0, 0, 0, 64, grid(count=(2, 0, 4)))
    assert "2^31" in api.NearestRefusal(0, 0, 0, 64, grid(count=(1 << 16, 1 << 15, 2))) and api.NearestRefusal(0, 0, 0, 64, grid(count=(1 << 16, 1 << 15, 1))) is None
    assert "2^31" in api.NearestRefusal(0, 0, 0, 64, grid(count=(1 << 31, 1 << 31, 1 << 31)))
    assert "finite" in api.NearestRefusal(0, 0, 0, 64, grid(origin=(0, np.nan, 0))) and "finite" in api.NearestRefusal(0, 0, 0, 64, grid(spacing=(np.inf, 1, 1)))
    assert "null" in api.NearestRefusal(0, 0, 0, 0, grid())
    assert "aligned" in api.NearestRefusal(api.NEAREST_DEVICE, 0, 0, 66, grid()) and api.NearestRefusal(0, 0, 0, 66, grid()) is None
    hs = host("rand7", 0)
    pts, _ = query_points("rand7")
    out = np.empty(len(pts), api.NEAREST_DTYPE)
    L = api.lib()
    for flags in (0, api.NEAREST_HOST_BRUTE | api.NEAREST_HOST_WALK, api.NEAREST_HOST_BRUTE | api.NEAREST_DEVICE, api.NEAREST_HOST_WALK | 2):
        assert L.tb_host_scene_nearest(hs._h, flags, len(pts), pts.ctypes.data, out.ctypes.data) == INVALID
    assert L.tb_host_scene_nearest(hs._h, api.NEAREST_HOST_BRUTE, 4, None, out.ctypes.data) == INVALID
    assert L.tb_host_scene_nearest(hs._h, api.NEAREST_HOST_BRUTE, 0, None, None) == 0
    two_level = api.HostScene(dc.INSTANCED, flatten_instances=False)
    assert L.tb_host_scene_nearest(two_level._h, api.NEAREST_HOST_BRUTE, len(pts), pts.ctypes.data, out.ctypes.data) == UNSUPPORTED


def test_wrong_arrays_are_refused_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    good = api.make_query_points(np.zeros((6, 3)))
    wrong = {
        "dtype float64": np.zeros((6, 4), np.float64),
        "three columns": np.zeros((6, 3), np.float32),
        "one dimension": np.zeros(24, np.float32),
        "two dimensions of records": np.zeros((3, 2), api.QUERY_POINT_DTYPE),
        "not contiguous": np.zeros((12, 4), np.float32)[::2],
        "records not contiguous": np.zeros(12, api.QUERY_POINT_DTYPE)[::2],
        "a list": [[0.0, 0.0, 0.0, 1.0]],
        "a host tensor": torch.zeros((6, 4), dtype=torch.float32),
        "a double tensor": torch.zeros((6, 4), dtype=torch.float64),
        "a query ray": np.zeros(6, api.QUERY_RAY_DTYPE),
    }
    for what, points in wrong.items():
        with pytest.raises(ValueError):
            tb.NearestPoints(points)
            pytest.fail(what)
    for signed in (1, None, "yes"):
        with pytest.raises(ValueError):
            tb.NearestPoints(good, signed=signed)
    with pytest.raises(AttributeError):                             # the good array gets past the checks, to the library this object lacks
        tb.NearestPoints(good)
    g = api.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    for kw in (dict(grid=(0, 0, 0)), dict(grid=g, signed=1), dict(grid=g, max_distance="far"), dict(grid=g, max_distance=None), dict(grid=g, device=1)):
        with pytest.raises(ValueError):
            tb.BakeDistanceField(**kw)
    with pytest.raises(AttributeError):
        tb.BakeDistanceField(g)
    hs = object.__new__(api.HostScene); hs._h = None
    for points in (wrong["dtype float64"], wrong["a host tensor"], wrong["a list"]):
        with pytest.raises(ValueError):
            hs.nearest(points)
    with pytest.raises(ValueError):
        hs.nearest(good, walk=1)


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pq_tb(built):
    """A context of this module's own: the tests load under builder options and move its scenes, which the session's context must not keep."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    yield tb
    tb.close()


def load(tb, name, builder):
    tb.SetOption("bvh_builder", builder)
    try:
        tb.LoadMeshes(meshes_of(ac.triangles(name)), mc.MATERIALS())
    finally:
        tb.SetOption("bvh_builder", 0)


def _refused(code, text, call, *args, **kw):
    from tracerboy_amd import api
    with pytest.raises(api.TracerBoyError) as e:
        call(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


@gpu
@pytest.mark.parametrize("builder", WALK_BUILDERS)
@pytest.mark.parametrize("name", ac.NAMES)
def test_device_records_are_the_host_brute_forces(pq_tb, name, builder):
    pts, kinds = query_points(name)
    load(pq_tb, name, builder)
    got = pq_tb.NearestPoints(pts)
    want = brute(name)
    assert same_bytes(got, want), np.flatnonzero(got != want)[:8]
    assert pq_tb.GetOption("last_nearest_us") > 0
    assert same_bytes(pq_tb.NearestPoints(pts[:0]), want[:0])                                      # n = 0: nothing launched


@gpu
@pytest.mark.parametrize("name", ["rand257", "same70"])
def test_device_path_signs_and_orders(pq_tb, name):
    """The device path on a torch tensor, signed, and the points reversed and shuffled: the same bytes per point."""
    import torch
    from tracerboy_amd import api
    pts, kinds = query_points(name)
    load(pq_tb, name, 4)
    flat = np.ascontiguousarray(pts.view(np.float32).reshape(-1, 4))
    dev = torch.from_numpy(flat).cuda()
    for signed in (False, True):
        want = brute(name, signed=signed)
        got = pq_tb.NearestPoints(dev, signed=signed)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(pts), 8) and got.device == dev.device
        assert same_bytes(got.cpu().numpy().view(api.NEAREST_DTYPE).ravel(), want)
        assert same_bytes(got.view(torch.int32)[:, 6].cpu().numpy().view(np.uint32), want["Prim"])
        assert same_bytes(pq_tb.NearestPoints(pts, signed=signed), want)
        order = np.random.default_rng(5).permutation(len(pts))
        for o in (np.arange(len(pts))[::-1].copy(), order):
            assert same_bytes(pq_tb.NearestPoints(np.ascontiguousarray(pts[o]), signed=signed), want[o])
            assert same_bytes(pq_tb.NearestPoints(dev[torch.from_numpy(o).cuda()].contiguous(), signed=signed).cpu().numpy().view(api.NEAREST_DTYPE).ravel(), want[o])
    assert (brute(name, signed=True)["Distance"] < 0).any()
    assert tuple(pq_tb.NearestPoints(dev[:0]).shape) == (0, 8)
    for wrong in (dev.cpu(), dev.double(), dev[::2], dev[:, :3], dev.view(-1), dev.view(-1)[1:-3].view(-1, 4)):
        with pytest.raises(ValueError):
            pq_tb.NearestPoints(wrong)
    # a host pointer passed as a device pointer
    out = np.empty(len(pts), api.NEAREST_DTYPE)
    assert pq_tb._L.tb_nearest_points(pq_tb._ctx, api.NEAREST_DEVICE, len(pts), flat.ctypes.data & ~15, out.ctypes.data & ~15) == INVALID


def layout_b_triangles(hs):
    nodes, tris, root = hs.layout_b()
    return np.ascontiguousarray(tris.view(np.float32).reshape(-1, 3, 4)[:, :, :3])


@gpu
@pytest.mark.parametrize("scene", ["cornell", "proc40k"])
def test_cornell_box_and_a_deep_tree(pq_tb, scene):
    """cornell-box (several geometries), and the 40 000-triangle procedural scene for a deep tree and the stack's upper reach."""
    from tracerboy_amd import api
    if scene == "cornell":
        hs = api.HostScene(CORNELL); pq_tb.LoadScene(CORNELL); n = 1500
    else:
        hs = api.HostScene(procedural=(0, rq.PROC_TRIANGLES, rq.PROC_SEED)); pq_tb.LoadProcedural(0, rq.PROC_TRIANGLES, rq.PROC_SEED); n = 4096
    pos, maxd, kinds = nc.points(layout_b_triangles(hs), n=n)
    pts = api.make_query_points(pos, maxd)
    for signed in (False, True):
        want = hs.nearest(pts, signed=signed)
        check_misses(want)
        assert same_bytes(pq_tb.NearestPoints(pts, signed=signed), want)
    assert len(np.unique(want["Geom"][~is_miss(want)])) > (1 if scene == "cornell" else 0)


@gpu
@pytest.mark.parametrize("builder", (0, 3))
@pytest.mark.parametrize("name", MOVED)
def test_moved_geometry(pq_tb, name, builder):
    """UpdatePositions + CommitGeometry (the refit, whose boxes are looser) and CommitGeometry(rebuild=True): the bytes of a host scene made of the
    moved soup, under brute force."""
    pts, kinds = query_points(name, moved=True)
    want = brute(name, moved=True)
    moved_positions, _ = ac.soup(ac.partner(name))
    for rebuild in (False, True):
        load(pq_tb, name, builder)
        before = pq_tb.NearestPoints(pts)
        pq_tb.UpdatePositions(moved_positions)
        assert same_bytes(pq_tb.NearestPoints(pts), before)                                        # staged, not yet committed
        pq_tb.CommitGeometry(rebuild=rebuild)
        assert same_bytes(pq_tb.NearestPoints(pts), want), rebuild
    assert not same_bytes(before, want)


@gpu
@pytest.mark.parametrize("count", [(9, 5, 3), (64, 1, 1)])
def test_distance_field(pq_tb, count):
    import torch
    from tracerboy_amd import api
    name = "rand65"
    load(pq_tb, name, 3)
    lo, hi = nc.bounds(ac.triangles(name))
    grid = api.ProbeGrid.in_bounds(lo - 0.25, hi + 0.25, count)
    centres = api.probe_grid_positions(grid)
    shape = (count[2], count[1], count[0])
    for signed in (False, True):
        want = pq_tb.NearestPoints(api.make_query_points(centres), signed=signed)["Distance"].reshape(shape)
        assert same_bytes(want.ravel(), host(name, 0).nearest(api.make_query_points(centres), signed=signed)["Distance"])
        got = pq_tb.BakeDistanceField(grid, signed=signed)
        assert got.dtype == np.float32 and same_bytes(got, want)
        dev = pq_tb.BakeDistanceField(grid, signed=signed, device=True)
        assert dev.dtype == torch.float32 and tuple(dev.shape) == shape and dev.is_cuda and same_bytes(dev.cpu().numpy(), want)
        cut = float(np.median(np.abs(want)))
        limited = pq_tb.NearestPoints(api.make_query_points(centres, cut), signed=signed)["Distance"].reshape(shape)
        assert np.isinf(limited).any() and np.isfinite(limited).any() and (limited[np.isinf(limited)] > 0).all()
        assert same_bytes(pq_tb.BakeDistanceField(grid, signed=signed, max_distance=cut), limited)
        assert same_bytes(np.where(np.abs(want) <= np.float32(cut), want, INF), limited)
    assert pq_tb.GetOption("last_nearest_us") > 0


@gpu
def test_refusals_on_a_context(pq_tb):
    import torch
    from tracerboy_amd import api
    pts, _ = query_points("rand7")
    grid = api.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    fresh = api.TracerBoy(0)
    try:                                                            # no scene
        _refused(NO_SCENE, "no scene", fresh.NearestPoints, pts)
        _refused(NO_SCENE, "no scene", fresh.BakeDistanceField, grid)
        assert fresh._L.tb_nearest_points(fresh._ctx, 2, len(pts), pts.ctypes.data, pts.ctypes.data) == INVALID     # the arguments come first
    finally:
        fresh.close()
    group = api.TracerBoy(devices=[0, 0])
    try:                                                            # a group context
        group.LoadScene(CORNELL)
        _refused(UNSUPPORTED, "multi-device group", group.NearestPoints, pts)
        _refused(UNSUPPORTED, "multi-device group", group.BakeDistanceField, grid)
    finally:
        group.close()
    pq_tb.SetOption("flatten_instances", 0)
    try:                                                            # a two-level scene
        pq_tb.LoadScene(dc.INSTANCED)
    finally:
        pq_tb.SetOption("flatten_instances", 1)
    assert pq_tb.HostSceneView().numInstances > 0
    _refused(UNSUPPORTED, "two-level", pq_tb.NearestPoints, pts)
    _refused(UNSUPPORTED, "two-level", pq_tb.BakeDistanceField, grid)
    load(pq_tb, "rand7", 0)
    want = brute("rand7")
    out = np.empty(len(pts), api.NEAREST_DTYPE)
    L, ctx = pq_tb._L, pq_tb._ctx
    assert L.tb_nearest_points(ctx, 2, len(pts), pts.ctypes.data, out.ctypes.data) == INVALID                       # an unknown flag
    assert L.tb_nearest_points(ctx, 0, len(pts), None, out.ctypes.data) == INVALID and L.tb_nearest_points(ctx, 0, len(pts), pts.ctypes.data, None) == INVALID
    assert L.tb_nearest_points(ctx, 0, (1 << 31) + 1, pts.ctypes.data, out.ctypes.data) == INVALID
    assert L.tb_nearest_points(ctx, 0, 0, None, None) == 0
    dev = torch.from_numpy(np.ascontiguousarray(pts.view(np.float32).reshape(-1, 4))).cuda()
    res = torch.empty((len(pts), 8), dtype=torch.float32, device=dev.device)
    torch.cuda.synchronize()
    assert L.tb_nearest_points(ctx, api.NEAREST_DEVICE, len(pts), dev.data_ptr() + 4, res.data_ptr()) == INVALID     # misaligned
    # past the allocation -- torch's allocator hands out pieces of larger blocks, so by more than any block of a 24 KB tensor: 2^27 points are 2 GB
    assert L.tb_nearest_points(ctx, api.NEAREST_DEVICE, 1 << 27, dev.data_ptr(), res.data_ptr()) == INVALID
    assert L.tb_nearest_points(ctx, api.NEAREST_DEVICE, len(pts), dev.data_ptr(), out.ctypes.data & ~15) == INVALID  # a host pointer as a device pointer
    g = grid.c_struct()
    field = np.empty(8, np.float32)
    assert L.tb_bake_distance_field(ctx, 0, None, np.inf, field.ctypes.data) == INVALID and L.tb_bake_distance_field(ctx, 0, api.C.byref(g), np.inf, None) == INVALID
    assert L.tb_bake_distance_field(ctx, 4, api.C.byref(g), np.inf, field.ctypes.data) == INVALID
    assert L.tb_bake_distance_field(ctx, api.NEAREST_DEVICE, api.C.byref(g), np.inf, field.ctypes.data & ~3) == INVALID
    g.count[1] = 0
    assert L.tb_bake_distance_field(ctx, 0, api.C.byref(g), np.inf, field.ctypes.data) == INVALID
    assert same_bytes(pq_tb.NearestPoints(pts), want)                                              # and it still works
