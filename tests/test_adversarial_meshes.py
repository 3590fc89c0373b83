"""Tree builders, walks and the refit on adversarial small meshes, against ground truth.  The meshes, the ray sets and the
yardsticks -- a float64 brute force over every triangle, which shares no tree and no box test with the walks -- come from tests/adversarial_cases.py;
refit_layout_a is dynamic_cases', the bit-exact expectations ray_query_cases' on the CPU oracle.  Every scene is one api.Mesh of at most 512
triangles, loaded through HostScene.from_meshes / LoadMeshes."""
import numpy as np
import pytest

import adversarial_cases as ac
import dynamic_cases as dc
import mesh_cases as mc
import ray_query_cases as rq

gpu = pytest.mark.gpu
W, H, FRAMES = 32, 24, 2
HOST_BUILDERS = (0, 1, 3)             # LBVH, the SAH builder, LBVH + treelet passes
WALK_BUILDERS = (0, 1, 3, 4)          # and the treelet passes on the device
REFIT_BUILDERS = (0, 3)
REFILL_COUNTS = (1, 63, 64, 65, 1500)
RENDERED = ("rand7", "same70", "flat512", "expo40")
# What the 40 KB budget of an LDS-resident scene (lds_image.h LdsSceneBytes) lets in, by (case, builder), with the emissive quad: 80 + 6 * 48 + 12 + 96 B a
# triangle and 1 KB of stacks per level.  rand7: 9 triangles, 5 levels.  expo40 under builder 0: 42 triangles, 20 KB, and 16 or 17 levels.  expo40 under
# builder 4 is 27 levels deep, same70 is 72 triangles (34 KB) and 8 levels or more, flat512 is 514 triangles: these render from memory either way.
LDS_RESIDENT = {("rand7", 0), ("rand7", 4), ("expo40", 0)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def meshes_of(name, light=False):
    from tracerboy_amd import api
    tri = ac.triangles(name)
    p, i = ac.soup(tri)
    out = [api.Mesh(p, i)]
    if light:                                                        # an emissive quad above the bounds, facing down
        lo, hi = p.min(0), p.max(0)
        c, size = (lo + hi) / 2, float(max((hi - lo).max(), 0.5))
        qp, qi, qn = mc.quad(y=float(hi[1]) + 0.5 * size, h=0.6 * size)
        qp = (qp + np.float32([c[0], 0.0, c[2]])).astype(np.float32)
        out.append(api.Mesh(qp, qi, normals=qn, material=2))
    return out


_hosts = {}


def host(name, builder):
    """The case built on the host, made once: (HostScene, view, layout-A image, triangles())."""
    from tracerboy_amd import api
    key = (name, builder)
    if key not in _hosts:
        hs = api.HostScene.from_meshes(meshes_of(name), mc.MATERIALS(), bvh_builder=builder)
        view = hs.view()
        _hosts[key] = (hs, view, dc.bvh_bytes(view), hs.triangles())
    return _hosts[key]


def by_primitive(view, image=None):
    """(N, 3, 3): the triangles by primitive number, through the view's own hit-group record and index buffer (positions as the image holds them)."""
    image = dc.bvh_bytes(view) if image is None else image
    _, _, meta = dc._sections(image)
    assert (meta[:, 0] == 0).all() and sorted(meta[:, 1]) == list(range(len(meta)))
    tri = np.zeros((len(meta), 3, 3), np.float32)
    tri[meta[:, 1]] = dc.positions_of(view, image)[dc.sorted_tri_vertices(view, image)]
    return tri


def check_closest(name, view, t, u, v, prim, moved=False, image=None):
    o, d, want, edge = ac.truth(name, moved)
    tri = by_primitive(view, image)
    assert same_bytes(tri, np.ascontiguousarray(ac.partner(name) if moved else ac.triangles(name)))   # the scene holds the soup, in its order
    both = ac.check_against_brute_force(t, want, edge)
    ac.check_hit_points(tri, o, d, t, u, v, prim, both)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------

def test_catalogue_is_seeded_and_as_documented():
    for n in ac.RAND_SIZES + ac.PARTNER_SIZES:
        assert len(ac.triangles("rand%d" % n)) == n
    sizes = {name: len(ac.triangles(name)) for name in ("same70", "nested40", "expo40", "flat512", "sliver64", "zero32", "split65")}
    assert sizes == dict(same70=70, nested40=40, expo40=40, flat512=512, sliver64=64, zero32=32, split65=65)
    assert len(np.unique(ac.triangles("same70").reshape(70, 9), axis=0)) == 1
    flat = ac.triangles("flat512")
    assert (flat[:, :, 1] == 0).all()
    zero = ac.triangles("zero32")
    area = np.linalg.norm(np.cross(zero[:, 1] - zero[:, 0], zero[:, 2] - zero[:, 0]), axis=1)
    assert (area[::4] == 0).all() and (np.delete(area, np.arange(0, 32, 4)) > 0).all() and (zero[::8, 0] == zero[::8, 2]).all()
    for name in ac.NAMES:                                            # seeded: made twice, the same bytes
        assert same_bytes(np.ascontiguousarray(ac.CASES[name]()), np.ascontiguousarray(ac.triangles(name)))
        assert ac.partner(name).shape == ac.triangles(name).shape
    o, d = ac.rays(ac.triangles("rand7"))
    axial = (np.abs(d) == 1).any(axis=1) & ((d == 0).sum(axis=1) == 2)
    assert len(o) == 1500 and axial.sum() == 250 and all((np.abs(d[axial]).argmax(axis=1) == a).sum() > 40 for a in range(3))
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", ac.NAMES)
def test_host_trees_are_valid_and_the_oracles(built, name):
    import oracle_lib as ol
    for builder in HOST_BUILDERS:
        hs, view, image, g = host(name, builder)
        assert ol.validate_bvh(image, g) == (0, hs.info().bvhMaxDepth), builder
        if builder != 1:
            assert same_bytes(image, ol.build_lbvh(g, builder)), builder
    if ac.passes_that_run(len(ac.triangles(name))) == 0:
        assert same_bytes(host(name, 3)[2], host(name, 0)[2])
    if name == "expo40":                                             # the depths the case is there for
        depths = [host(name, b)[0].info().bvhMaxDepth for b in HOST_BUILDERS]
        assert depths[0] == 16 and depths[2] == 27 and 20 <= depths[1] <= 32      # (the SAH builder's is its heuristics': 28 as measured)
    if name == "same70":
        assert host(name, 3)[0].info().bvhMaxDepth == 20
    if name == "rand1":
        assert host(name, 0)[0].info().bvhMaxDepth == 1


@pytest.mark.parametrize("name", ac.NAMES)
def test_oracle_walk_finds_the_geometrically_nearest_hit(built, name):
    """tbo_trace_closest on the trees of builders 0, 1 and 3 against the brute force: no clear hit lost, t within rtol 2e-5 / atol 2e-6, no hit
    invented, the hit point on the reported triangle; clear hits are at least 95 % of the hits and at least 50."""
    import oracle_lib as ol
    o, d, want, edge = ac.truth(name)
    for builder in HOST_BUILDERS:
        hs, view, image, g = host(name, builder)
        assert same_bytes(g["positions"][g["tri_vertex_index"]], np.ascontiguousarray(ac.triangles(name)))
        got = ol.trace_closest(view, o, d)
        check_closest(name, view, got["t"], got["bary"][:, 0], got["bary"][:, 1], got["prim"], image=image)


def test_brute_force_notices_a_box_that_culls_a_real_hit(built):
    """What the comparison with the oracle's walk cannot see: on flat512 with every leaf box halved about its centre -- an image tbo_trace_closest
    still walks without complaint -- hits are lost, and the brute-force assertions say so; a distance off by 1e-4 of itself is caught as well."""
    import oracle_lib as ol
    hs, view, image, g = host("flat512", 0)
    o, d, want, edge = ac.truth("flat512")
    good = ol.trace_closest(view, o, d)["t"]
    ac.check_against_brute_force(good, want, edge)
    broken = image.copy()
    nodes, prims, _ = dc._sections(broken)
    n = len(prims)
    nodes[n - 1:, 4:7] = (nodes[n - 1:, 4:7].view(np.float32) * np.float32(0.5)).view(np.uint32)
    lossy = ol.trace_closest(dc.with_bvh(view, broken), o, d)["t"]
    assert ((good > 0) & (lossy < 0)).sum() > 100
    with pytest.raises(AssertionError, match="hits lost"):
        ac.check_against_brute_force(lossy, want, edge)
    with pytest.raises(AssertionError, match="t off"):
        ac.check_against_brute_force(np.where(good > 0, good * np.float32(1.0001), good), want, edge)
    with pytest.raises(AssertionError, match="hits invented"):
        ac.check_against_brute_force(np.where(good > 0, good, np.float32(1.0)), want, edge)


@pytest.mark.parametrize("name", ac.NAMES)
def test_yardstick_refits_every_case(built, name):
    """refit_layout_a gives back the loaded image from the load positions, and after each of the three moves -- all vertices on the centroid, the
    partner's positions, back -- an image tbo_validate_bvh accepts at the load's depth, on which the oracle's walk is right by the brute force; back at
    the load positions, the loaded bytes."""
    import oracle_lib as ol
    for builder in REFIT_BUILDERS:
        hs, view, image, g = host(name, builder)
        depth = hs.info().bvhMaxDepth
        pos = dc.positions_of(view, image)
        assert same_bytes(pos, ac.soup(ac.triangles(name))[0])
        assert same_bytes(dc.refit_layout_a(view, pos), image)
        previous = image
        for move, new in enumerate((ac.collapsed(pos), ac.soup(ac.partner(name))[0], pos)):
            previous = dc.refit_layout_a(view, new, image=previous)
            assert ol.validate_bvh(previous, dc.tri_dict(view, previous, new)) == (0, depth)
            if move == 1:                                            # the loose tree of the exchanged positions loses nothing (the GPU test's condition)
                o, d, want, edge = ac.truth(name, moved=True)
                got = ol.trace_closest(dc.with_bvh(view, previous), o, d)
                check_closest(name, view, got["t"], got["bary"][:, 0], got["bary"][:, 1], got["prim"], moved=True, image=previous)
        assert same_bytes(previous, image)


# ---- with a GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def adv_tb(built):
    """A context of this module's own: the tests load under builder options and move its scenes, which the session's context must not keep."""
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    yield tb
    tb.close()


def load(tb, name, builder, light=False, **options):
    """A fresh load of the case under bvh_builder = builder and `options`, which then go back to their defaults: (view, layout-A image)."""
    defaults = {k: tb.GetOption(k) for k in options}
    tb.SetOption("bvh_builder", builder)
    for k, v in options.items():
        tb.SetOption(k, v)
    try:
        tb.LoadMeshes(meshes_of(name, light), mc.MATERIALS())
    finally:
        tb.SetOption("bvh_builder", 0)
        for k, v in defaults.items():
            tb.SetOption(k, v)
    view = tb.HostSceneView()
    return view, dc.bvh_bytes(view)


@gpu
@pytest.mark.parametrize("name", ac.NAMES)
def test_gpu_builders_give_the_host_builders_bytes(adv_tb, name):
    """bvh_builder 2 is host builder 0 and bvh_builder 4, loaded twice, host builder 3: the image and the depth.  Where the scene is too small for
    any treelet pass (fewer than 7 triangles), 4 is 0 as well."""
    want0, want3 = host(name, 0), host(name, 3)
    view, image = load(adv_tb, name, 2)
    assert same_bytes(image, want0[2]) and adv_tb.SceneInfo().bvhMaxDepth == want0[0].info().bvhMaxDepth
    for _ in range(2):
        view, image = load(adv_tb, name, 4)
        assert same_bytes(image, want3[2]) and adv_tb.SceneInfo().bvhMaxDepth == want3[0].info().bvhMaxDepth
    if ac.passes_that_run(len(ac.triangles(name))) == 0:
        assert same_bytes(image, want0[2])
    view, image = load(adv_tb, name, 0)                              # and what the context builds on the host is what HostScene builds
    assert same_bytes(image, want0[2])


def query_rays(name, tmax=np.inf, moved=False):
    from tracerboy_amd import api
    o, d, want, edge = ac.truth(name, moved)
    return api.make_query_rays(o, d, tmax)


@gpu
@pytest.mark.parametrize("builder", WALK_BUILDERS)
@pytest.mark.parametrize("name", ac.NAMES)
def test_closest_hits_are_the_oracles_and_the_geometrys(adv_tb, name, builder):
    """TraceRays(RAYS_CLOSEST): bit-equal to the oracle's walk of the context's own view (the existing rule), and -- what that rule cannot see, the
    oracle walking the same tree with the same box test -- right by the brute force: nothing lost, nothing invented, t and the hit point in tolerance."""
    import oracle_lib as ol
    from tracerboy_amd import api
    view, image = load(adv_tb, name, builder)
    rays = query_rays(name)
    got = adv_tb.TraceRays(rays, api.RAYS_CLOSEST)
    want = rq.expected_hits(rays, ol.trace_closest(view, rays["Origin"], rays["Direction"]))
    for field in api.QUERY_HIT_DTYPE.names:
        assert same_bytes(got[field], want[field]), field
    check_closest(name, view, got["T"], got["U"], got["V"], got["Prim"], image=image)


def occluded_sets(name):
    """The three ray sets of the occluded checks and what the brute force expects of each: TMax = inf, 0.5 t and 2 t of the brute-force hits (inf where
    it has none); compare: the rays whose hit is clear and not within near_tmax's 1e-4 t of TMax -- by construction none is."""
    o, d, want, edge = ac.truth(name)
    hit = np.isfinite(want)
    compare = ~hit | (edge > ac.CLEAR_EDGE)
    t32 = np.where(hit, want, np.inf).astype(np.float32)
    sets = []
    for factor in (None, 0.5, 2.0):
        tmax = np.full(len(o), np.inf, np.float32) if factor is None else (np.float32(factor) * t32).astype(np.float32)
        with np.errstate(invalid="ignore"):
            near = hit & (np.abs(want - tmax) <= 1e-4 * want)
            expect = (hit & (want < np.minimum(tmax.astype(np.float64), float(rq.MAX_T))) & (tmax > rq.MIN_T)).astype(np.uint8)
        assert not near.any()
        sets.append((query_rays(name, tmax), expect, compare & ~near))
    return sets


@gpu
@pytest.mark.parametrize("builder", WALK_BUILDERS)
@pytest.mark.parametrize("name", ac.NAMES)
def test_occlusion_is_the_geometrys_in_every_form_of_the_any_hit_walk(adv_tb, monkeypatch, name, builder):
    """TraceRays(RAYS_OCCLUDED) against the brute force at three TMax, as shipped (one ray per lane below 32 768 triangles) and with TB_RQ_REFILL = 8,
    the refilling form, which otherwise never sees a tree this small or fewer rays than one pool; and for 1, 63, 64, 65 and 1500 rays, prefixes of the
    sets, the refilling form's bytes are those of the one-ray-per-lane form (0) and of the closest-hit walk's t < TMax (-1)."""
    from tracerboy_amd import api
    load(adv_tb, name, builder)
    for rays, expect, compare in occluded_sets(name):
        assert compare.sum() >= ac.MIN_CLEAR_HITS
        monkeypatch.delenv("TB_RQ_REFILL", raising=False)
        got = adv_tb.TraceRays(rays, api.RAYS_OCCLUDED)
        assert np.array_equal(got[compare], expect[compare]), np.flatnonzero(compare & (got != expect))[:8]
        for n in REFILL_COUNTS:
            answers = {}
            for form in ("8", "0", "-1"):
                monkeypatch.setenv("TB_RQ_REFILL", form)
                answers[form] = adv_tb.TraceRays(np.ascontiguousarray(rays[:n]), api.RAYS_OCCLUDED)
            assert len(answers["8"]) == n and same_bytes(answers["8"], answers["0"]) and same_bytes(answers["8"], answers["-1"]), n
        assert np.array_equal(answers["8"][compare], expect[compare])                                  # (the last count is the whole set)


def lds_scene_bytes(view, depth):
    """lds_image.h LdsSceneBytes for a one-level view"""
    r16 = lambda b: (b + 15) // 16 * 16
    n = view.numIndices // 3
    shading = r16(view.numHitGroups * 16) + r16(view.numIndices * 4) + r16(view.numVertexFloats * 4) + r16(view.numMaterials * 96) + r16(view.numLights * 112)
    return r16(max(n - 1, 1) * 80) + r16(n * 6 * 48) + shading + max(depth, 2) * 256 * 4


@gpu
@pytest.mark.parametrize("builder", (0, 4))
@pytest.mark.parametrize("name", RENDERED)
def test_small_renders_are_the_oracles_from_lds_and_from_memory(adv_tb, settings, name, builder):
    """The case under an emissive quad, through the default camera, 32 x 24, 2 frames, MaxBounces 4: the accumulation is the oracle's on the context's
    view with scene_in_lds = 1 and with 0.  The first runs the LDS-resident walk for the cases of LDS_RESIDENT, the second the walk from memory."""
    import oracle_lib as ol
    assert settings.MaxBounces == 4
    active = []
    for in_lds in (1, 0):
        view, image = load(adv_tb, name, builder, light=True, scene_in_lds=in_lds)
        assert view.numLights == 2
        adv_tb.InvalidateHistory()
        adv_tb.Render(W, H, FRAMES, settings, 0.0)
        got = adv_tb.ReadAccumulation().copy()
        active.append(adv_tb.GetOption("scene_in_lds_active"))
        want = ol.render(view, adv_tb.FrameConstants(W, H, 0, settings, 0.0), W, H, FRAMES, threads=8)["output"]
        assert same_bytes(got, want), (in_lds, int((got != want).any(axis=2).sum()))
        assert (got[:, :, :3] != 0).any(axis=2).sum() >= 1                                             # the camera sees the lit mesh: 2, 10, 46 and 1 pixels
    fits = lds_scene_bytes(view, adv_tb.SceneInfo().bvhMaxDepth) <= 40 * 1024
    assert fits == ((name, builder) in LDS_RESIDENT)
    assert active == [1 if fits else 0, 0]


@gpu
@pytest.mark.parametrize("builder", REFIT_BUILDERS)
@pytest.mark.parametrize("name", [n for n in ac.NAMES if len(ac.triangles(n)) >= 2])
def test_refit_follows_collapse_exchange_and_return(adv_tb, monkeypatch, name, builder):
    """UpdatePositions + CommitGeometry under both forms of the bottom-up pass, three moves: every vertex onto the centroid (every leaf a point, every
    box the pad), onto another case's positions of as many triangles, back.  After each the image is the yardstick's refit of the one before and
    valid at the load's depth; on the exchanged and the returned positions the closest hits are right by the brute force -- a refitted tree is loose,
    but it may lose nothing --; back at the load positions the image is the loaded one."""
    import oracle_lib as ol
    from tracerboy_amd import api
    here, there = ac.soup(ac.triangles(name))[0], ac.soup(ac.partner(name))[0]
    for form in ("0", "1"):
        monkeypatch.setenv("TB_REFIT_FORM", form)
        view, loaded = load(adv_tb, name, builder)
        depth = adv_tb.SceneInfo().bvhMaxDepth
        assert same_bytes(loaded, host(name, builder)[2])
        previous = loaded
        for move, new in enumerate((ac.collapsed(here), there, here)):
            adv_tb.UpdatePositions(new); adv_tb.CommitGeometry()
            view = adv_tb.HostSceneView(); got = dc.bvh_bytes(view)
            assert same_bytes(got, dc.refit_layout_a(view, new, image=previous)), (form, move)
            assert ol.validate_bvh(got, dc.tri_dict(view, got, new)) == (0, depth), (form, move)
            if move:
                hits = adv_tb.TraceRays(query_rays(name, moved=move == 1), api.RAYS_CLOSEST)
                check_closest(name, view, hits["T"], hits["U"], hits["V"], hits["Prim"], moved=move == 1, image=got)
            previous = got
        assert same_bytes(previous, loaded), form
