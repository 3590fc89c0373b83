"""The inputs and the yardsticks of tests/test_adversarial_meshes.py: numpy only.

A case is a triangle soup, (N, 3, 3) float32, handed over as ONE api.Mesh of 3N vertices and the indices arange(3N) with mesh_cases.MATERIALS(), so
vertex 3 t + k is corner k of triangle t and a hit's Prim is the soup's triangle number.  Every case is seeded and at most 512 triangles; what each is
aimed at stands with its maker.  brute_force_closest is geometry alone -- Moeller-Trumbore in float64 against every triangle -- and so shares no box
test, no tree and no visit order with the walks it judges; check_against_brute_force holds a walk's answers against it by the rule and the tolerances
of test_oracle_known_answers.py::test_traversal_finds_the_geometrically_nearest_hit."""
import numpy as np

F32 = np.float32
CLEAR_EDGE = 1e-4                     # a hit is "clear" when its barycentrics keep this distance from the triangle's edges
T_RTOL, T_ATOL = 2e-5, 2e-6
MIN_CLEAR_SHARE, MIN_CLEAR_HITS = 0.95, 50
RAY_SEED = 60
TREELET_THRESHOLDS = (7, 14, 28)

RAND_SIZES = (1, 2, 3, 6, 7, 8, 13, 14, 15, 27, 28, 29, 63, 64, 65, 255, 256, 257)
PARTNER_SIZES = (70, 40, 32, 512)    # rand cases that exist to give same70, nested40 / expo40, zero32 and flat512 a second set of positions


def rand(n, seed=None):
    """n triangles, centres uniform in [-1, 1]^3, corners within 0.3 of the centre.  N = 1: the root is a leaf; 6 / 7 / 8, 13 / 14 / 15 and
    27 / 28 / 29: either side of the treelet passes' thresholds; 63 / 64 / 65: a wave; 255 / 256 / 257: a workgroup of the builders' kernels."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    centre = rng.uniform(-1, 1, (n, 1, 3))
    return (centre + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(F32)


def same70():
    """One triangle 70 times: every Morton code is equal, so delta() falls back on the index bits throughout, and every SAH cost of a treelet ties."""
    return np.repeat(F32([[[-0.5, -0.25, 0.125], [0.75, -0.125, -0.25], [0.0, 0.875, 0.25]]]), 70, axis=0)


def nested40():
    """40 concentric scaled copies of one triangle, 0.05 apart along z: the centroids coincide in x and y, the boxes nest."""
    base = np.array([[-1.0, -0.6, 0.0], [1.0, -0.6, 0.0], [0.0, 1.2, 0.0]])           # centroid (0, 0, 0)
    k = np.arange(40)[:, None, None]
    return (base[None] * (1.0 - 0.02 * k) + np.array([0.0, 0.0, 0.05]) * k).astype(F32)


def expo40():
    """Triangles of size 0.2 * 2^-k at x = 2^-k, k < 40: the Morton grid (1 / 1024 of the extent) collapses the tail, and the trees are deep."""
    s = (2.0 ** -np.arange(40))[:, None, None]
    shape = np.array([[0.0, -0.1, -0.1], [0.0, 0.1, -0.1], [0.0, 0.0, 0.1]])          # depth 16, 28 and 27 under builders 0, 1 and 3
    return (np.array([1.0, 0.0, 0.0]) * s + shape[None] * s).astype(F32)


def flat512():
    """A 16 x 16 grid of quads in the plane y = 0: the scene has no extent in y (bvh_morton's dim clamp), and every box is the 0.001 pad thick."""
    g = np.linspace(-1.0, 1.0, 17)
    tri = []
    for i in range(16):
        for j in range(16):
            a, b, c, d = (g[i], 0.0, g[j]), (g[i + 1], 0.0, g[j]), (g[i + 1], 0.0, g[j + 1]), (g[i], 0.0, g[j + 1])
            tri += [[a, b, c], [a, c, d]]
    return F32(tri)


def sliver64(seed=1064):
    """8 needle triangles along the scene's diagonal (boxes as large as the scene around almost no area) over 56 tiny ones."""
    rng = np.random.default_rng(seed)
    diag = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    needles = []
    for k in range(8):
        off = rng.uniform(-0.4, 0.4, 3); off -= diag * (off @ diag)
        side = np.cross(diag, rng.normal(size=3)); side *= 0.03 / np.linalg.norm(side)
        needles.append([off - 1.6 * diag, off + 1.6 * diag + side, off + 1.6 * diag - side])
    centre = rng.uniform(-1, 1, (56, 1, 3))
    tiny = centre + rng.uniform(-0.02, 0.02, (56, 3, 3))
    return np.concatenate([np.array(needles), tiny]).astype(F32)


def zero32(seed=1032):
    """32 random triangles; every 4th has two equal corners (a segment), every 8th three (a point): leaves of no area, which nothing can hit."""
    tri = rand(32, seed)
    tri[::4, 1] = tri[::4, 0]
    tri[::8, 2] = tri[::8, 0]
    return tri


def split65(seed=1165):
    """Added on reading bvh_hierarchy: 33 copies of one triangle and 32 of another far away.  Two runs of colliding codes, 33 and 32 long, so delta()
    compares codes at exactly one place and index bits across a power of two on either side of it."""
    tri = rand(2, seed)
    tri[1] += F32([3.0, 0.0, 0.0])
    return np.concatenate([np.repeat(tri[:1], 33, axis=0), np.repeat(tri[1:], 32, axis=0)])


CASES = {"rand%d" % n: (lambda n=n: rand(n)) for n in RAND_SIZES + PARTNER_SIZES}
CASES.update(same70=same70, nested40=nested40, expo40=expo40, flat512=flat512, sliver64=sliver64, zero32=zero32, split65=split65)
NAMES = list(CASES)
# the positions a case is moved onto by the refit tests: another case of as many triangles
PARTNERS = {"rand64": "sliver64", "sliver64": "rand64", "same70": "rand70", "rand70": "same70", "nested40": "rand40", "expo40": "nested40", "rand40": "expo40",
            "zero32": "rand32", "rand32": "zero32", "flat512": "rand512", "rand512": "flat512", "rand65": "split65", "split65": "rand65"}
_made = {}


def triangles(name):
    if name not in _made:
        t = np.ascontiguousarray(CASES[name](), F32)
        assert t.ndim == 3 and t.shape[1:] == (3, 3) and len(t) <= 512 and np.isfinite(t).all()
        t.setflags(write=False)
        _made[name] = t
    return _made[name]


def partner(name):
    """(N, 3, 3): other positions for the case's vertices -- the paired case's, or for a rand case without one a second draw of as many triangles."""
    tri = triangles(name)
    other = triangles(PARTNERS[name]) if name in PARTNERS else rand(len(tri), 2000 + len(tri))
    assert other.shape == tri.shape and not np.array_equal(other, tri)
    return other


def soup(tri):
    """positions (3N, 3) float32 and indices (N, 3) uint32 of the one mesh"""
    return np.ascontiguousarray(tri.reshape(-1, 3), F32), np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3)


def collapsed(positions):
    """every vertex on the centroid of all of them"""
    return np.ascontiguousarray(np.tile(positions.astype(np.float64).mean(axis=0).astype(F32), (len(positions), 1)))


def passes_that_run(n):
    """how many of the three treelet passes a scene of n triangles is large enough for (bvh_gpu_build, BuildTreelets: minTris <= N)"""
    return sum(1 for m in TREELET_THRESHOLDS if m <= n)


# ---- rays ------------------------------------------------------------------------------------------------------------------------------------

def rays(tri, n=1500, seed=RAY_SEED):
    """(origins, directions), (n, 3) float32 each.  Origins are uniform in the bounds grown by 30 % of max(extent, 0.5) per axis.  The first two
    thirds are aimed at the centroid of a random triangle with a jitter of 2 % of the extent; of the rest one half has a random direction and the other
    is exactly axis-parallel, along +-x, +-y or +-z -- and every second of those starts on the axis through such a jittered centroid, so that
    axis-parallel rays (one infinite reciprocal, two slabs of inf * 0 where the origin lies on a box's plane) also find something.  Every prefix
    of the set holds all three kinds in turn: the kinds are dealt out by a seeded permutation."""
    rng = np.random.default_rng(seed)
    tri = tri.astype(np.float64)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    grow = 0.3 * np.maximum(hi - lo, 0.5)
    o = rng.uniform(lo - grow, hi + grow, (n, 3))
    aim = tri[rng.integers(0, len(tri), n)].mean(axis=1) + rng.normal(scale=0.02, size=(n, 3)) * (hi - lo)
    d = rng.normal(size=(n, 3))
    aimed, axial = 2 * n // 3, n - (n - 2 * n // 3) // 2
    d[:aimed] = (aim - o)[:aimed]
    axis = rng.integers(0, 3, n); sign = rng.choice([-1.0, 1.0], n)
    for k in range(axial, n):
        d[k] = 0.0; d[k, axis[k]] = sign[k]
        if k & 1:
            cross = [a for a in range(3) if a != axis[k]]
            o[k, cross] = aim[k, cross]
    norm = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(norm > 0, d / np.where(norm > 0, norm, 1.0), [1.0, 0.0, 0.0])
    o, d = o.astype(F32), d.astype(F32)
    d[axial:] = np.sign(d[axial:])                                   # exactly one component of +-1
    order = rng.permutation(n)
    return np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])


def brute_force_closest(tri, o, d, tmin=0.001):
    """Nearest intersection of each ray with ANY triangle, Moeller-Trumbore in float64: geometry, not the reference's arithmetic.
    tri (T, 3, 3), o / d (R, 3) -> t (R,) (inf on a miss), edge (R,) = how close the winning hit is to a triangle edge."""
    tri = tri.astype(np.float64); o = o.astype(np.float64); d = d.astype(np.float64)
    best_t = np.full(len(o), np.inf); best_edge = np.zeros(len(o))
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    for r0 in range(0, len(o), 64):
        oo, dd = o[r0:r0 + 64, None, :], d[r0:r0 + 64, None, :]
        p = np.cross(dd, e2[None]); det = (e1[None] * p).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = oo - tri[None, :, 0]; u = (s * p).sum(-1) * inv
            q = np.cross(s, e1[None]); v = (dd * q).sum(-1) * inv; t = (e2[None] * q).sum(-1) * inv
            ok = (np.abs(det) > 1e-14) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin)   # (a triangle of no area: inf and NaN, never ok)
            t = np.where(ok, t, np.inf)
            k = t.argmin(axis=1); rows = np.arange(t.shape[0])
            best_t[r0:r0 + 64] = t[rows, k]
            best_edge[r0:r0 + 64] = np.minimum(np.minimum(u[rows, k], v[rows, k]), 1 - u[rows, k] - v[rows, k])
    return best_t, best_edge


_truth = {}


def truth(name, moved=False):
    """(origins, directions, t, edge) of the case -- of its partner's positions with `moved` -- made once and shared; the arrays are read-only."""
    key = (name, moved)
    if key not in _truth:
        tri = partner(name) if moved else triangles(name)
        o, d = rays(tri)
        t, edge = brute_force_closest(tri, o, d)
        for a in (o, d, t, edge):
            a.setflags(write=False)
        _truth[key] = (o, d, t, edge)
    return _truth[key]


def counts(want_t, edge):
    hit = np.isfinite(want_t)
    return int(hit.sum()), int((hit & (edge > CLEAR_EDGE)).sum())


def check_against_brute_force(got_t, want_t, edge, need_hits=True):
    """The assertions of test_traversal_finds_the_geometrically_nearest_hit on a walk's distances got_t (negative: a miss).  need_hits: the two
    conditions that keep the exclusion of unclear hits from hiding a failure -- a prefix of a ray set, or a degenerate move, may go without."""
    hit = np.isfinite(want_t)
    both = hit & (edge > CLEAR_EDGE)                                  # the nearest hit is well inside its triangle
    if need_hits:
        assert both.sum() >= MIN_CLEAR_SHARE * hit.sum() and both.sum() >= MIN_CLEAR_HITS, (int(both.sum()), int(hit.sum()))
    lost = np.flatnonzero(both & ~(got_t > 0))
    assert len(lost) == 0, ("hits lost", lost[:8], want_t[lost[:8]])
    far = np.flatnonzero(both & ~np.isclose(got_t, want_t, rtol=T_RTOL, atol=T_ATOL))
    assert len(far) == 0, ("t off", far[:8], got_t[far[:8]], want_t[far[:8]])
    invented = np.flatnonzero(~hit & ~(got_t < 0))
    assert len(invented) == 0, ("hits invented", invented[:8], got_t[invented[:8]])
    return both


def check_hit_points(tri, o, d, t, u, v, prim, which):
    """T, U, V give the same point on the reported triangle as on the ray, for the rays `which`: the distance between o + t d and
    (1 - u - v) v0 + u v1 + v v2 stays within the tolerance the distances themselves are held to, T_ATOL + T_RTOL * t."""
    w = np.flatnonzero(which)
    assert (prim[w] < len(tri)).all()
    p = tri[prim[w]].astype(np.float64)
    uu, vv, tt = u[w].astype(np.float64)[:, None], v[w].astype(np.float64)[:, None], t[w].astype(np.float64)
    on_tri = (1 - uu - vv) * p[:, 0] + uu * p[:, 1] + vv * p[:, 2]
    on_ray = o[w].astype(np.float64) + tt[:, None] * d[w].astype(np.float64)
    gap = np.linalg.norm(on_tri - on_ray, axis=1)
    bad = np.flatnonzero(gap > T_ATOL + T_RTOL * tt)
    assert len(bad) == 0, ("hit point off its triangle", w[bad[:8]], gap[bad[:8]])
    assert (u[w] >= 0).all() and (v[w] >= 0).all() and (u[w] + v[w] <= 1 + 1e-6).all()
