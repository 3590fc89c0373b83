"""Winding numbers (include/tracerboy_hip.h tb_winding_numbers .. tb_bake_distance_field_winding; the rule:
include/tb_winding.h): robust inside / outside by the generalized winding number, the host's statement of the rule against a float64 sum by another
route (tests/winding_cases.py), the device against the host on bits.  Scenes: the closed meshes of winding_cases.py, the adversarial soups of
tests/adversarial_cases.py under the builders tests/test_adversarial_meshes.py runs, cornell-box, the 40 000-triangle procedural scene."""
import ctypes as C

import numpy as np
import pytest

import adversarial_cases as ac
import dynamic_cases as dc
import mesh_cases as mc
import nearest_cases as nc
import ray_query_cases as rq
import winding_cases as wc
from conftest import CORNELL

gpu = pytest.mark.gpu
HOST_BUILDERS = (0, 1, 3)
WALK_BUILDERS = (0, 1, 3, 4)
INVALID, UNSUPPORTED, NO_SCENE = -1, -6, -7
INF = np.float32(np.inf)
NAN_BITS = 0x7fc00000


def same_bytes(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def meshes_of(tri):
    from tracerboy_amd import api
    p, i = ac.soup(tri)
    return [api.Mesh(p, i)]


_hosts = {}


def host(name, builder):
    from tracerboy_amd import api
    if (name, builder) not in _hosts:
        _hosts[(name, builder)] = api.HostScene.from_meshes(meshes_of(wc.triangles(name)), mc.MATERIALS(), bvh_builder=builder)
    return _hosts[(name, builder)]


def points_of(positions):
    from tracerboy_amd import api
    return api.make_query_points(positions)


def case_points(name, seed=nc.POINT_SEED):
    """the case's query points WITH the tail's MaxDistance values (the winding number does not read them; the signed point query does)"""
    from tracerboy_amd import api
    pos, maxd, kinds = nc.case_points("winding/" + name, wc.triangles(name), seed)
    return api.make_query_points(pos, maxd), kinds


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def test_header_exports_and_bindings(built):
    from tracerboy_amd import api
    raw = C.CDLL(api.LIB_PATH)
    bound = api.lib()
    for name in ("tb_winding_numbers", "tb_bake_winding_field", "tb_nearest_points_winding", "tb_bake_distance_field_winding", "tb_winding_refusal",
                 "tb_host_scene_winding"):
        assert hasattr(raw, name) and name in bound._tb_exports, name
    assert (api.WINDING_DEVICE, api.WINDING_HOST_BRUTE, api.WINDING_HOST_WALK) == (0x100, 0x1000, 0x2000) and api.WINDING_DEVICE == api.RAYS_DEVICE
    assert api.WINDING_BETA == wc.DEFAULT_BETA
    for method in ("WindingNumbers", "BakeWindingField"):
        assert callable(getattr(api.TracerBoy, method)), method
    assert api.winding_inside(np.float32([0.5, -0.5, 0.49, -2.0, np.nan, 0.0])).tolist() == [True, True, False, True, False, False]


def test_known_answers(built):
    """An octant; the unit cube on the grid of eighths off its boundary, reversed and twice over; the cavity of the shell."""
    from tracerboy_amd import api
    octant = np.float32([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]])
    origin = points_of(np.zeros((1, 3), np.float32))
    g = np.arange(-4, 13, dtype=np.float32) / 8
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    inside = ((pos > 0) & (pos < 1)).all(axis=1)
    off = inside | ((pos < 0) | (pos > 1)).any(axis=1)
    grid = points_of(pos[off]); inside = inside[off]
    cavity = ((pos[off] > 0.25) & (pos[off] < 0.75)).all(axis=1)
    wall = inside & ((pos[off] < 0.25) | (pos[off] > 0.75)).any(axis=1)
    assert inside.sum() == 343 and cavity.sum() == 27 and wall.sum() == 343 - 125
    for builder in HOST_BUILDERS:
        for kw in (dict(), dict(walk=True), dict(walk=True, beta=np.inf), dict(walk=True, beta=1.0)):
            w = api.HostScene.from_meshes(meshes_of(octant), mc.MATERIALS(), bvh_builder=builder).winding(origin, **kw)
            if kw.get("beta") != 1.0:                             # at beta = 1 the one triangle is its own dipole: an estimate
                assert abs(abs(float(w[0])) - 0.125) <= 2.0 ** -23, (builder, kw, w)
        for kw in (dict(), dict(walk=True), dict(walk=True, beta=2.0), dict(walk=True, beta=np.inf)):
            beta = kw.get("beta", wc.DEFAULT_BETA) if kw.get("walk") else np.inf
            tol = wc.W_EXACT_TOL if beta == np.inf else wc.W_BETA_TOL[beta]
            w = host("cube12", builder).winding(grid, **kw)
            assert np.abs(w - inside).max() <= tol, (builder, kw)
            rev = api.HostScene.from_meshes(meshes_of(wc.reverse(wc.triangles("cube12"))), mc.MATERIALS(), bvh_builder=builder).winding(grid, **kw)
            assert np.abs(rev + inside).max() <= tol, (builder, kw)
            assert np.abs(host("twice", builder).winding(grid, **kw) - 2.0 * inside).max() <= 2 * tol, (builder, kw)
            sh = host("shell", builder).winding(grid, **kw)
            assert np.abs(sh[cavity]).max() <= tol and np.abs(sh[wall] - 1).max() <= tol and np.abs(sh[~inside]).max() <= tol, (builder, kw)
            assert np.array_equal(api.winding_inside(w), inside) and np.array_equal(api.winding_inside(rev), inside)
            clear = cavity | wall | ~inside                         # (the grid also has points ON the inner cube)
            assert np.array_equal(api.winding_inside(sh)[clear], wall[clear])


@pytest.mark.parametrize("name", ["tetra4", "star40"])
def test_the_nearest_triangles_side_is_not_the_inside_test(built, name):
    """The motivating measurement, made with the library: the off-surface points of the seeds 70, 71, 72 at which HostScene.nearest(signed=True)
    has another sign than winding64 > 0.5.  Measured: tetra4 209 of 3 843 (5.4 %) -- a CONVEX closed mesh --, star40 239 of 3 849 (6.2 %).  The
    host walk at the default beta: none on either."""
    from tracerboy_amd import api
    wrong = total = 0
    for seed in wc.SEEDS:
        pos, kinds, off, w64 = wc.truth(name, seed)
        pts = points_of(pos[off])
        inside = w64[off] > 0.5
        wrong += int(((host(name, 0).nearest(pts, signed=True)["Distance"] < 0) != inside).sum())
        total += len(inside)
        for builder in HOST_BUILDERS:
            assert np.array_equal(api.winding_inside(host(name, builder).winding(pts, walk=True)), inside), (seed, builder)
    print(name, "the nearest triangle's side is wrong at", wrong, "of", total)
    assert wrong >= 1


@pytest.mark.parametrize("name", wc.ACCURACY_NAMES)
def test_accuracy_of_the_exact_and_the_dipole_form(built, name):
    """|w - winding64| <= W_EXACT_TOL for the brute force and the walk at beta = inf, <= W_BETA_TOL[beta] for the walk at beta 2, 3 and 4: every
    off-surface point (winding_cases.py has the rule) of the seeds 70, 71, 72, builders 0, 1 and 3."""
    worst = {"exact": 0.0, 2.0: 0.0, 3.0: 0.0, 4.0: 0.0}
    for seed in wc.SEEDS:
        pos, kinds, off, w64 = wc.truth(name, seed)
        pts = points_of(pos[off]); want = w64[off]
        err = lambda w: float(np.abs(w.astype(np.float64) - want).max())
        worst["exact"] = max(worst["exact"], err(host(name, 0).winding(pts)))
        for builder in HOST_BUILDERS:
            worst["exact"] = max(worst["exact"], err(host(name, builder).winding(pts, beta=np.inf, walk=True)))
            for beta in wc.W_BETA_TOL:
                worst[beta] = max(worst[beta], err(host(name, builder).winding(pts, beta=beta, walk=True)))
    print(name, "worst |w - winding64|:", worst)
    assert worst["exact"] <= wc.W_EXACT_TOL
    for beta, tol in wc.W_BETA_TOL.items():
        assert worst[beta] <= tol, beta
    for tol, measured in [(wc.W_EXACT_TOL, wc.W_EXACT_MEASURED)] + [(wc.W_BETA_TOL[b], wc.W_BETA_MEASURED[b]) for b in wc.W_BETA_TOL]:
        assert 2 * measured < tol <= 4 * measured and np.log2(tol) == round(np.log2(tol))             # the next power of two above twice the worst


@pytest.mark.parametrize("name", list(wc.CLOSED))
def test_classification_of_closed_meshes(built, name):
    from tracerboy_amd import api
    pos, kinds, off, w64 = wc.truth(name)
    pts = points_of(pos[off])
    inside = np.abs(w64[off]) > 0.5
    assert inside.any() and (~inside).any()
    assert np.array_equal(api.winding_inside(host(name, 0).winding(pts)), inside)
    for builder in HOST_BUILDERS:
        for beta in (2.0, wc.DEFAULT_BETA, np.inf):
            assert np.array_equal(api.winding_inside(host(name, builder).winding(pts, beta=beta, walk=True)), inside), (builder, beta)


def test_triangles_of_no_area_and_positions_that_are_not_finite(built):
    pts, kinds = case_points("zero32")
    finite = np.isfinite(pts["Position"]).all(axis=1)
    assert (~finite).sum() == nc.TAIL_EACH and (kinds[~finite] == "not_finite").all()
    for builder in HOST_BUILDERS:
        for kw in (dict(), dict(walk=True), dict(walk=True, beta=2.0), dict(walk=True, beta=np.inf), dict(walk=True, beta=1.0)):
            w = host("zero32", builder).winding(pts, **kw)
            assert np.isfinite(w[finite]).all(), (builder, kw)
            assert (w[~finite].view(np.uint32) == NAN_BITS).all(), (builder, kw)
    # triangles collapsed to one point, seen from so near that L2 * sqrt(L2) underflows: N = 0 over 0 would be a NaN; the rule says 0
    from tracerboy_amd import api
    tri = np.concatenate([np.zeros((3, 3, 3), np.float32), np.float32([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]])])
    near = points_of(np.float32([[1e-20, 0, 0], [0, -1e-19, 1e-20], [1e-16, 1e-16, 0]]))
    for builder in HOST_BUILDERS:
        hs = api.HostScene.from_meshes(meshes_of(tri), mc.MATERIALS(), bvh_builder=builder)
        for beta in (1.0, 2.0, wc.DEFAULT_BETA):
            assert np.abs(np.abs(hs.winding(near, beta=beta, walk=True)) - 0.125).max() <= wc.W_BETA_TOL[2.0], (builder, beta)


def test_the_walk_at_infinite_beta_visits_every_triangle_and_the_far_field_is_one_dipole(built):
    """beta = inf accepts nothing, so the walk's sum differs from the brute force's by the order of its additions alone; a point 10^6 extents away
    gets the root's dipole, whatever beta."""
    for name in ("rand1", "rand2", "rand257", "same70", "torus256"):
        pts, kinds = case_points(name)
        far = kinds == "far"
        for builder in HOST_BUILDERS:
            h = host(name, builder)
            exact = h.winding(pts, beta=np.inf, walk=True)
            assert np.abs(exact[kinds != "not_finite"] - h.winding(pts)[kinds != "not_finite"]).max() <= wc.W_EXACT_TOL
            assert same_bytes(h.winding(pts[far], beta=1.0, walk=True), h.winding(pts[far], beta=64.0, walk=True))


def test_a_tree_of_presplit_references_is_refused(built):
    """Option presplit leaves a cut triangle in the tree once per reference: a sum over the leaves would count it as often (the `twice` case: w = 2),
    so both host forms refuse such a scene, as the refit does, and answer the same scene built without it."""
    from tracerboy_amd import api
    kw = dict(procedural=(1, 20000, 7), bvh_builder=1, reinsertion_passes=0)
    plain, cut = api.HostScene(**kw), api.HostScene(presplit=30, **kw)
    assert len(cut.layout_b()[1]) > len(plain.layout_b()[1]) == plain.info().numTriangles == cut.info().numTriangles
    pts = points_of(np.float32([[0.1, 0.2, 0.3], [5.0, 5.0, 5.0]]))
    for walk in (False, True):
        with pytest.raises(api.TracerBoyError) as e:
            cut.winding(pts, walk=walk)
        assert e.value.code == UNSUPPORTED
        assert np.isfinite(plain.winding(pts, walk=walk)).all()


def test_refusals_of_the_arguments(built):
    from tracerboy_amd import api
    from tracerboy_amd import _ctypes_abi as abi
    R = api.WindingRefusal
    assert R(0, 4, 64, 128) is None and R(api.WINDING_DEVICE, 4, 64, 128) is None and R(api.WINDING_HOST_WALK, 4, 64, 128) is None
    assert R(0, 0, 0, 0) is None
    assert "flag" in R(1, 4, 64, 128) and "flag" in R(api.WINDING_HOST_BRUTE, 4, 64, 128) and "flag" in R(api.WINDING_DEVICE | api.WINDING_HOST_WALK, 4, 64, 128)
    assert "2^31" in R(0, (1 << 31) + 1, 64, 128) and "null" in R(0, 4, 0, 128) and "null" in R(0, 4, 64, 0)
    assert "aligned" in R(api.WINDING_DEVICE, 4, 72, 128) and "aligned" in R(api.WINDING_DEVICE, 4, 64, 130) and R(api.WINDING_DEVICE, 4, 64, 132) is None
    for beta in (np.nan, 0.5, -1.0, 0.0, -np.inf):
        assert "beta" in R(0, 4, 64, 128, beta=beta), beta
    assert R(0, 4, 64, 128, beta=1.0) is None and R(0, 4, 64, 128, beta=np.inf) is None
    assert "flag" in R(1, 4, 64, 128, beta=np.nan)                                                # the arguments' order: flags before beta

    def grid(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 3, 4)):
        return abi.tb_probe_grid((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*count))
    assert R(0, 0, 0, 64, grid()) is None and "flag" in R(api.WINDING_HOST_WALK, 0, 0, 64, grid()) and "count" in R(0, 0, 0, 64, grid(count=(2, 0, 4)))
    assert "finite" in R(0, 0, 0, 64, grid(origin=(0, np.nan, 0))) and "null" in R(0, 0, 0, 0, grid()) and "beta" in R(0, 0, 0, 64, grid(), beta=0.5)
    assert "aligned" in R(api.WINDING_DEVICE, 0, 0, 66, grid())
    assert "flag" in api.NearestRefusal(2, 4, 64, 128)                                             # flag 2 is still nobody's in tb_nearest_points
    hs = host("rand7", 0)
    pts, _ = case_points("rand7")
    out = np.empty(len(pts), np.float32)
    L = api.lib()
    for flags in (0, api.WINDING_HOST_BRUTE | api.WINDING_HOST_WALK, api.WINDING_HOST_BRUTE | api.WINDING_DEVICE, api.WINDING_HOST_WALK | 1):
        assert L.tb_host_scene_winding(hs._h, flags, len(pts), pts.ctypes.data, 2.0, out.ctypes.data) == INVALID
    for beta in (np.nan, 0.5, -1.0):
        assert L.tb_host_scene_winding(hs._h, api.WINDING_HOST_WALK, len(pts), pts.ctypes.data, beta, out.ctypes.data) == INVALID
    assert L.tb_host_scene_winding(hs._h, api.WINDING_HOST_BRUTE, 4, None, 2.0, out.ctypes.data) == INVALID
    assert L.tb_host_scene_winding(hs._h, api.WINDING_HOST_BRUTE, 0, None, 2.0, None) == 0
    two_level = api.HostScene(dc.INSTANCED, flatten_instances=False)
    assert L.tb_host_scene_winding(two_level._h, api.WINDING_HOST_BRUTE, len(pts), pts.ctypes.data, 2.0, out.ctypes.data) == UNSUPPORTED


def test_wrong_arguments_are_refused_before_any_library_call():
    """On an object that has no context and no library: whatever got past the checks would fail on the missing attribute, not with ValueError."""
    import torch
    from tracerboy_amd import api
    tb = object.__new__(api.TracerBoy)
    good = api.make_query_points(np.zeros((6, 3)))
    g = api.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    for points in (np.zeros((6, 4), np.float64), np.zeros((6, 3), np.float32), [[0.0] * 4], torch.zeros((6, 4), dtype=torch.float32), np.zeros((12, 4), np.float32)[::2]):
        with pytest.raises(ValueError):
            tb.WindingNumbers(points)
    for beta in (np.nan, 0.5, -1, 0, None, "2", True):
        with pytest.raises(ValueError):
            tb.WindingNumbers(good, beta=beta)
        with pytest.raises(ValueError):
            tb.BakeWindingField(g, beta=beta)
        if beta is not None:                                         # None is the keyword's "not asked for"
            with pytest.raises(ValueError):
                tb.NearestPoints(good, winding_beta=beta)
            with pytest.raises(ValueError):
                tb.BakeDistanceField(g, winding_beta=beta)
    with pytest.raises(ValueError):
        tb.WindingNumbers(good, host_walk=1)
    with pytest.raises(ValueError):
        tb.NearestPoints(good, signed=True, winding_beta=2.0)
    with pytest.raises(ValueError):
        tb.BakeDistanceField(g, signed=True, winding_beta=2.0)
    with pytest.raises(ValueError):
        tb.NearestPoints(good, signed=1)                             # signed stays a strict bool
    for kw in (dict(grid=(0, 0, 0)), dict(grid=g, device=1)):
        with pytest.raises(ValueError):
            tb.BakeWindingField(**kw)
    for call in (lambda: tb.WindingNumbers(good), lambda: tb.WindingNumbers(good, beta=np.inf), lambda: tb.BakeWindingField(g),
                 lambda: tb.NearestPoints(good, winding_beta=2), lambda: tb.BakeDistanceField(g, winding_beta=2.0)):
        with pytest.raises(AttributeError):                          # good arguments get past the checks, to the library this object lacks
            call()
    hs = object.__new__(api.HostScene); hs._h = None
    for kw in (dict(points=np.zeros((6, 4), np.float64)), dict(points=good, beta=0.5), dict(points=good, beta=np.nan), dict(points=good, walk=1)):
        with pytest.raises(ValueError):
            hs.winding(**kw)


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wn_tb(built):
    """A context of this module's own: the tests load under builder options and move its scenes, which the session's context must not keep."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    yield tb
    tb.close()


def load(tb, tri, builder):
    tb.SetOption("bvh_builder", builder)
    try:
        tb.LoadMeshes(meshes_of(tri), mc.MATERIALS())
    finally:
        tb.SetOption("bvh_builder", 0)


def _refused(code, text, call, *args, **kw):
    from tracerboy_amd import api
    with pytest.raises(api.TracerBoyError) as e:
        call(*args, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def device_equals_host_walk(tb, pts, betas, shuffled_beta=None):
    """The device's numbers are the context's host walk's on bits, for host arrays; and, at shuffled_beta, for a device tensor reversed and shuffled:
    a point's number does not depend on its lane."""
    import torch
    for beta in betas:
        want = tb.WindingNumbers(pts, beta=beta, host_walk=True)
        got = tb.WindingNumbers(pts, beta=beta)
        assert got.dtype == np.float32 and same_bytes(got, want), (beta, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
        if beta == shuffled_beta:
            dev = torch.from_numpy(np.ascontiguousarray(pts.view(np.float32).reshape(-1, 4))).cuda()
            for o in (np.arange(len(pts))[::-1].copy(), np.random.default_rng(5).permutation(len(pts))):
                out = tb.WindingNumbers(dev[torch.from_numpy(o).cuda()].contiguous(), beta=beta)
                assert out.dtype == torch.float32 and tuple(out.shape) == (len(pts),) and out.is_cuda
                assert same_bytes(out.cpu().numpy(), want[o]), beta
    return want


@gpu
@pytest.mark.parametrize("builder", WALK_BUILDERS)
@pytest.mark.parametrize("name", wc.NAMES)
def test_device_numbers_are_the_host_walks(wn_tb, name, builder):
    pts, kinds = case_points(name)
    load(wn_tb, wc.triangles(name), builder)
    w = device_equals_host_walk(wn_tb, pts, (1.0, 2.0, np.inf), shuffled_beta=2.0)
    assert (w[kinds == "not_finite"].view(np.uint32) == NAN_BITS).all() and np.isfinite(w[kinds != "not_finite"]).all()
    assert wn_tb.GetOption("last_winding_us") > 0 and wn_tb.GetOption("last_winding_fit_us") > 0
    assert wn_tb.WindingNumbers(pts[:0]).shape == (0,)                                             # n = 0: nothing launched


def layout_b_triangles(hs):
    nodes, tris, root = hs.layout_b()
    return np.ascontiguousarray(tris.view(np.float32).reshape(-1, 3, 4)[:, :, :3])


@gpu
@pytest.mark.parametrize("scene", ["cornell", "proc40k"])
def test_cornell_box_and_a_deep_tree(wn_tb, scene):
    from tracerboy_amd import api
    if scene == "cornell":
        hs = api.HostScene(CORNELL); wn_tb.LoadScene(CORNELL); n = 1500; betas = (2.0, wc.DEFAULT_BETA, np.inf)
    else:
        hs = api.HostScene(procedural=(0, rq.PROC_TRIANGLES, rq.PROC_SEED)); wn_tb.LoadProcedural(0, rq.PROC_TRIANGLES, rq.PROC_SEED); n = 4096
        betas = (1.0, 2.0, wc.DEFAULT_BETA)                        # (the exact form of 40 000 triangles x 4 096 points is the host's minute, not a test's)
    pos, maxd, kinds = nc.points(layout_b_triangles(hs), n=n)
    pts = api.make_query_points(pos, maxd)
    w = device_equals_host_walk(wn_tb, pts, betas, shuffled_beta=2.0)
    if scene == "cornell":                                           # the room faces inward: inside it |w| is about 1, and orientation does not matter
        assert api.winding_inside(w).any() and not api.winding_inside(w).all()


def moved_triangles(name):
    if name == "torus256":
        return np.ascontiguousarray(wc.triangles(name) * np.float32([1.0, 0.5, 2.0]))
    return ac.partner(name)


@gpu
@pytest.mark.parametrize("builder", (0, 3))
@pytest.mark.parametrize("name", ["rand64", "sliver64", "flat512", "rand512", "expo40", "torus256"])
def test_moved_geometry(wn_tb, name, builder):
    """UpdatePositions + CommitGeometry (the moments are fitted again over the standing topology) and CommitGeometry(rebuild=True): the device is the
    context's host walk on bits, and within the tolerances of winding64 OF THE MOVED SOUP -- stale moments fail this."""
    moved = moved_triangles(name)
    pos, kinds, off, w64 = wc.truth(name, tri=moved, key=name + "/moved")
    pts = points_of(pos)
    positions, _ = ac.soup(moved)
    for rebuild in (False, True):
        load(wn_tb, wc.triangles(name), builder)
        before = wn_tb.WindingNumbers(pts, beta=2.0)                                               # the moments of the scene as loaded
        before_exact = wn_tb.WindingNumbers(pts, beta=np.inf)
        wn_tb.UpdatePositions(positions)
        assert same_bytes(wn_tb.WindingNumbers(pts, beta=2.0), before)                             # staged, not yet committed
        wn_tb.CommitGeometry(rebuild=rebuild)
        for beta, tol in ((2.0, wc.W_BETA_TOL[2.0]), (np.inf, wc.W_EXACT_TOL)):
            w = device_equals_host_walk(wn_tb, pts, (beta,))
            err = float(np.abs(w[off].astype(np.float64) - w64[off]).max())
            print(name, builder, "rebuild" if rebuild else "refit", "beta", beta, "worst |w - winding64|:", err)
            assert err <= tol, (rebuild, beta)
    assert float(np.abs(before_exact[off].astype(np.float64) - w64[off]).max()) > wc.W_EXACT_TOL   # the case bites: the old geometry is far off


@gpu
@pytest.mark.parametrize("count", [(9, 5, 3), (64, 1, 1)])
def test_winding_field(wn_tb, count):
    import torch
    from tracerboy_amd import api
    load(wn_tb, wc.triangles("torus256"), 3)
    lo, hi = nc.bounds(wc.triangles("torus256"))
    grid = api.ProbeGrid.in_bounds(lo - 0.25, hi + 0.25, count)
    centres = points_of(api.probe_grid_positions(grid))
    shape = (count[2], count[1], count[0])
    for beta in (2.0, np.inf):
        want = wn_tb.WindingNumbers(centres, beta=beta).reshape(shape)
        got = wn_tb.BakeWindingField(grid, beta=beta)
        assert got.dtype == np.float32 and same_bytes(got, want)
        dev = wn_tb.BakeWindingField(grid, beta=beta, device=True)
        assert dev.dtype == torch.float32 and tuple(dev.shape) == shape and dev.is_cuda and same_bytes(dev.cpu().numpy(), want)
    assert same_bytes(wn_tb.BakeWindingField(grid), wn_tb.WindingNumbers(centres).reshape(shape))  # the default beta is one and the same


def check_sign_bits(signed, unsigned, inside):
    """every byte the unsigned answer's but the sign bit of Distance, which is set iff the record is a hit and the point inside"""
    from tracerboy_amd import api
    s = np.ascontiguousarray(signed).view(np.uint32).reshape(-1, 8).copy(); u = np.ascontiguousarray(unsigned).view(np.uint32).reshape(-1, 8)
    hit = unsigned["Distance"] != INF
    assert np.array_equal(s[:, 3] >> 31 == 1, hit & inside)
    s[:, 3] &= 0x7fffffff
    assert np.array_equal(s, u)


@gpu
@pytest.mark.parametrize("name", ["star40", "shell", "rand257"])
def test_signed_distance_by_winding_number(wn_tb, name):
    import torch
    from tracerboy_amd import api
    pts, kinds = case_points(name)
    load(wn_tb, wc.triangles(name), 4)
    unsigned = wn_tb.NearestPoints(pts)
    inside = api.winding_inside(wn_tb.WindingNumbers(pts, beta=2.0))
    signed = wn_tb.NearestPoints(pts, winding_beta=2)
    check_sign_bits(signed, unsigned, inside)
    miss = np.isin(kinds, ("zero", "nan", "negative", "half", "not_finite"))
    assert np.array_equal(unsigned["Distance"] == INF, miss) and (signed["Distance"][miss] == INF).all()
    assert (signed["Distance"] < 0).any() or name == "rand257"
    dev = torch.from_numpy(np.ascontiguousarray(pts.view(np.float32).reshape(-1, 4))).cuda()
    got = wn_tb.NearestPoints(dev, winding_beta=2.0)
    assert same_bytes(got.cpu().numpy().view(api.NEAREST_DTYPE).ravel(), signed)
    assert same_bytes(wn_tb.NearestPoints(pts), unsigned)                                          # and the plain call is what it was
    assert same_bytes(wn_tb.NearestPoints(pts[:0], winding_beta=2.0), unsigned[:0])


@gpu
@pytest.mark.parametrize("count", [(9, 5, 3), (64, 1, 1), (24, 24, 8)])
def test_signed_distance_field_by_winding_number(wn_tb, count):
    import torch
    from tracerboy_amd import api
    tri = wc.triangles("star40")
    load(wn_tb, tri, 3)
    lo, hi = nc.bounds(tri)
    grid = api.ProbeGrid.in_bounds(lo - 0.2, hi + 0.2, count)
    centres = api.probe_grid_positions(grid)
    shape = (count[2], count[1], count[0])
    unsigned = wn_tb.BakeDistanceField(grid)
    inside = api.winding_inside(wn_tb.WindingNumbers(points_of(centres), beta=2.0)).reshape(shape)
    got = wn_tb.BakeDistanceField(grid, winding_beta=2)
    assert got.dtype == np.float32 and same_bytes(np.abs(got), unsigned) and np.array_equal(np.signbit(got), inside)
    dev = wn_tb.BakeDistanceField(grid, winding_beta=2.0, device=True)
    assert dev.dtype == torch.float32 and dev.is_cuda and same_bytes(dev.cpu().numpy(), got)
    off = nc.distance64(tri, centres) >= nc.ULP * nc.scale(tri, centres)                          # winding_cases.py: off the surface
    assert off.sum() >= 0.9 * len(off)
    assert np.array_equal(np.signbit(got).ravel()[off], wc.winding64(tri, centres[off]) > 0.5)
    assert same_bytes(wn_tb.BakeDistanceField(grid), unsigned)
    cut = float(np.median(unsigned))
    limited = wn_tb.BakeDistanceField(grid, max_distance=cut, winding_beta=2.0)                    # a miss stays +inf, whatever the winding number there
    assert same_bytes(limited, np.where(unsigned <= np.float32(cut), got, INF)) and np.isinf(limited).any()
    if count == (24, 24, 8):
        assert np.signbit(got).any() and not np.signbit(got).all()


@gpu
def test_refusals_on_a_context(wn_tb):
    import torch
    from tracerboy_amd import api
    pts, _ = case_points("rand7")
    grid = api.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2))
    calls = lambda tb: ((tb.WindingNumbers, pts), (tb.BakeWindingField, grid), (lambda p: tb.NearestPoints(p, winding_beta=2.0), pts),
                        (lambda g: tb.BakeDistanceField(g, winding_beta=2.0), grid), (lambda p: tb.WindingNumbers(p, host_walk=True), pts))
    fresh = api.TracerBoy(0)
    try:                                                            # no scene
        for call, arg in calls(fresh):
            _refused(NO_SCENE, "no scene", call, arg)
        out = np.empty(len(pts), np.float32)
        assert fresh._L.tb_winding_numbers(fresh._ctx, 1, len(pts), pts.ctypes.data, 2.0, out.ctypes.data) == INVALID    # the arguments come first
        assert fresh._L.tb_winding_numbers(fresh._ctx, 0, len(pts), pts.ctypes.data, 0.5, out.ctypes.data) == INVALID
    finally:
        fresh.close()
    group = api.TracerBoy(devices=[0, 0])
    try:                                                            # a group context
        group.LoadScene(CORNELL)
        for call, arg in calls(group):
            _refused(UNSUPPORTED, "multi-device group", call, arg)
    finally:
        group.close()
    wn_tb.SetOption("flatten_instances", 0)
    try:                                                            # a two-level scene
        wn_tb.LoadScene(dc.INSTANCED)
    finally:
        wn_tb.SetOption("flatten_instances", 1)
    assert wn_tb.HostSceneView().numInstances > 0
    for call, arg in calls(wn_tb):
        _refused(UNSUPPORTED, "two-level", call, arg)
    wn_tb.SetOption("bvh_builder", 1); wn_tb.SetOption("presplit", 30)
    try:                                                            # a tree of pre-split references
        wn_tb.LoadProcedural(1, 20000, 7)
    finally:
        wn_tb.SetOption("bvh_builder", 0); wn_tb.SetOption("presplit", 0)
    for call, arg in calls(wn_tb):
        _refused(UNSUPPORTED, "pre-split", call, arg)
    assert np.isfinite(wn_tb.NearestPoints(pts)["Distance"]).any()                                 # the unsigned query has no such limit
    load(wn_tb, wc.triangles("rand7"), 0)
    want = wn_tb.WindingNumbers(pts, beta=2.0)
    out = np.empty(len(pts), np.float32); rec = np.empty(len(pts), api.NEAREST_DTYPE)
    L, ctx = wn_tb._L, wn_tb._ctx
    assert L.tb_winding_numbers(ctx, 1, len(pts), pts.ctypes.data, 2.0, out.ctypes.data) == INVALID                  # an unknown flag
    assert L.tb_winding_numbers(ctx, 0, len(pts), None, 2.0, out.ctypes.data) == INVALID and L.tb_winding_numbers(ctx, 0, len(pts), pts.ctypes.data, 2.0, None) == INVALID
    assert L.tb_winding_numbers(ctx, 0, (1 << 31) + 1, pts.ctypes.data, 2.0, out.ctypes.data) == INVALID
    for beta in (np.nan, 0.5, -1.0):
        assert L.tb_winding_numbers(ctx, 0, len(pts), pts.ctypes.data, beta, out.ctypes.data) == INVALID
        assert L.tb_nearest_points_winding(ctx, 0, len(pts), pts.ctypes.data, beta, rec.ctypes.data) == INVALID
    assert L.tb_winding_numbers(ctx, 0, 0, None, 2.0, None) == 0
    assert L.tb_nearest_points_winding(ctx, api.NEAREST_SIGNED, len(pts), pts.ctypes.data, 2.0, rec.ctypes.data) == INVALID   # the other rule's flag
    assert L.tb_nearest_points(ctx, 2, len(pts), pts.ctypes.data, rec.ctypes.data) == INVALID                        # flag 2 is still nobody's
    dev = torch.from_numpy(np.ascontiguousarray(pts.view(np.float32).reshape(-1, 4))).cuda()
    res = torch.empty((len(pts),), dtype=torch.float32, device=dev.device)
    torch.cuda.synchronize()
    D = api.WINDING_DEVICE
    assert L.tb_winding_numbers(ctx, D, len(pts), dev.data_ptr() + 4, 2.0, res.data_ptr()) == INVALID                # misaligned
    assert L.tb_winding_numbers(ctx, D, len(pts), dev.data_ptr(), 2.0, res.data_ptr() + 2) == INVALID
    assert L.tb_winding_numbers(ctx, D, 1 << 27, dev.data_ptr(), 2.0, res.data_ptr()) == INVALID                     # short: 2^27 points are 2 GB
    assert L.tb_winding_numbers(ctx, D, len(pts), dev.data_ptr(), 2.0, out.ctypes.data & ~15) == INVALID             # a host pointer as a device pointer
    assert L.tb_winding_numbers(ctx, D, len(pts), pts.ctypes.data & ~15, 2.0, res.data_ptr()) == INVALID
    g = grid.c_struct()
    field = np.empty(8, np.float32)
    assert L.tb_bake_winding_field(ctx, 0, None, 2.0, field.ctypes.data) == INVALID and L.tb_bake_winding_field(ctx, 0, C.byref(g), 2.0, None) == INVALID
    assert L.tb_bake_winding_field(ctx, api.WINDING_HOST_WALK, C.byref(g), 2.0, field.ctypes.data) == INVALID
    assert L.tb_bake_winding_field(ctx, D, C.byref(g), 2.0, field.ctypes.data & ~3) == INVALID
    assert L.tb_bake_distance_field_winding(ctx, api.NEAREST_SIGNED, C.byref(g), np.inf, 2.0, field.ctypes.data) == INVALID
    assert L.tb_bake_distance_field_winding(ctx, 0, C.byref(g), np.inf, 0.5, field.ctypes.data) == INVALID
    assert same_bytes(wn_tb.WindingNumbers(pts, beta=2.0), want)                                   # and it still works
