"""The inputs and the yardsticks of tests/test_nearest_points.py: numpy only.

points() makes a case's query points; distance64() is geometry alone -- per triangle the projection onto its plane where that falls inside, else the
nearest of its three segments, in float64 -- and so shares neither the Voronoi-region method nor any arithmetic with include/tb_nearest.h, no tree
and no visit order with the walks it judges; aspect() and DISTANCE_C state the one allowance of the comparison."""
import numpy as np

F32 = np.float32
POINT_SEED = 70
TAIL_KINDS = ("inf", "zero", "nan", "negative", "half", "twice", "not_finite", "far")
TAIL_EACH = 6
# |Distance - d64| <= DISTANCE_C * 2^-23 * M * aspect(Prim): M the largest coordinate magnitude of scene and point, aspect = (longest edge)^2 / (2 area)
# of the winning triangle.  Measured on the CPU (scripts/nearest_slack.py): the worst ratio of the host brute force over every case of
# adversarial_cases.NAMES but zero32 and the point seeds 70, 71, 72 is 10.771 (sliver64, seed 71; below 2.1 on every other case); DISTANCE_C is the
# next power of two above twice that.
DISTANCE_C_MEASURED = 10.771
DISTANCE_C = 32.0
ULP = 2.0 ** -23


def bounds(tri):
    flat = tri.astype(np.float64).reshape(-1, 3)
    return flat.min(0), flat.max(0)


def extent(tri):
    lo, hi = bounds(tri)
    return float((hi - lo).max())


def _segment(P, a, b):
    ab = b - a
    L = (ab * ab).sum(-1)
    s = ((P - a) * ab).sum(-1) / np.where(L > 0, L, 1.0)
    s = np.where(L > 0, np.clip(s, 0.0, 1.0), 0.0)
    return np.linalg.norm(P - (a + s[..., None] * ab), axis=-1)


def distance64(tri, p):
    """(n,) float64: the distance of every point to the nearest of the triangles (T, 3, 3)."""
    tri = tri.astype(np.float64); p = p.astype(np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    nrm = np.cross(b - a, c - a); nn = (nrm * nrm).sum(-1)
    safe = np.where(nn > 0, nn, 1.0)
    out = np.empty(len(p))
    for r0 in range(0, len(p), 128):
        P = p[r0:r0 + 128, None, :]
        t = ((P - a) * nrm).sum(-1) / safe
        Q = P - t[..., None] * nrm
        inside = (nn > 0) & ((np.cross(b - a, Q - a) * nrm).sum(-1) >= 0) & ((np.cross(c - b, Q - b) * nrm).sum(-1) >= 0) & \
            ((np.cross(a - c, Q - c) * nrm).sum(-1) >= 0)
        edges = np.minimum(np.minimum(_segment(P, a, b), _segment(P, b, c)), _segment(P, c, a))
        out[r0:r0 + 128] = np.where(inside, np.abs(t) * np.sqrt(nn), edges).min(axis=1)
    return out


def aspect(tri):
    """(T,) float64: (longest edge)^2 / (2 area) per triangle; inf for a triangle of no area."""
    tri = tri.astype(np.float64)
    e = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], axis=1)
    longest = (e * e).sum(-1).max(axis=1)
    twice_area = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
    with np.errstate(divide="ignore"):
        return np.where(twice_area > 0, longest / np.where(twice_area > 0, twice_area, 1.0), np.inf)


def scale(tri, p):
    """(n,) float64: the largest coordinate magnitude of the scene and each point"""
    return np.maximum(np.abs(tri.astype(np.float64)).max(), np.abs(p.astype(np.float64)).max(axis=1))


def points(tri, n=1500, seed=POINT_SEED):
    """(positions (n, 3) float32, max_distance (n,) float32, kinds (n,) of str).  Of the first n - 48: one half uniform in the bounds grown by 30 % of
    max(extent, 0.5) per axis ("uniform"); the other a random point of a random triangle displaced by a normal-distributed offset of 10^U(-6, -1) x
    the extent ("near") -- every 7th of these exactly that surface point ("surface"), every 7th exactly a vertex ("vertex").  All with MaxDistance
    +inf.  Then the fixed tail, TAIL_EACH points of each of TAIL_KINDS: uniform positions with MaxDistance +inf, 0, NaN, -1, half and twice the true
    distance; a position that is not finite; a point 10^6 extents outside."""
    rng = np.random.default_rng(seed)
    t64 = tri.astype(np.float64)
    lo, hi = bounds(tri)
    ext = max(extent(tri), 1e-3)
    grow = 0.3 * np.maximum(hi - lo, 0.5)
    tail = TAIL_EACH * len(TAIL_KINDS)
    body = n - tail
    assert body >= 14
    nu = body // 2; ns = body - nu
    pos = np.empty((n, 3), F32); kinds = np.empty(n, dtype=object)
    pos[:nu] = rng.uniform(lo - grow, hi + grow, (nu, 3)); kinds[:nu] = "uniform"
    k = rng.integers(0, len(tri), ns)
    w = rng.random((ns, 2)); fold = w.sum(1) > 1; w[fold] = 1.0 - w[fold]
    on = t64[k, 0] + w[:, :1] * (t64[k, 1] - t64[k, 0]) + w[:, 1:] * (t64[k, 2] - t64[k, 0])
    off = rng.normal(size=(ns, 3)) * (10.0 ** rng.uniform(-6, -1, (ns, 1))) * ext
    corner = rng.integers(0, 3, ns)
    i = np.arange(ns)
    near = (on + off).astype(F32); kinds[nu:body] = "near"
    near[i % 7 == 0] = on[i % 7 == 0].astype(F32); kinds[nu:body][i % 7 == 0] = "surface"
    near[i % 7 == 3] = tri[k, corner][i % 7 == 3]; kinds[nu:body][i % 7 == 3] = "vertex"
    pos[nu:body] = near
    maxd = np.full(n, np.inf, F32)
    base = rng.uniform(lo - grow, hi + grow, (tail, 3)).astype(F32)
    true = distance64(tri, base)
    centre = (lo + hi) / 2
    for j, kind in enumerate(TAIL_KINDS):
        for e in range(TAIL_EACH):
            t = j * TAIL_EACH + e; at = body + t
            pos[at] = base[t]; kinds[at] = kind
            if kind == "zero": maxd[at] = 0.0
            elif kind == "nan": maxd[at] = np.nan
            elif kind == "negative": maxd[at] = -1.0
            elif kind == "half": maxd[at] = F32(0.5 * true[t])
            elif kind == "twice": maxd[at] = F32(2.0 * true[t])
            elif kind == "not_finite": pos[at, e % 3] = (np.nan, np.inf, -np.inf)[(e // 3 + e) % 3]
            elif kind == "far":
                d = rng.normal(size=3); d /= np.linalg.norm(d)
                pos[at] = (centre + d * 1e6 * ext).astype(F32)
    return np.ascontiguousarray(pos), maxd, kinds


_made = {}


def case_points(name, tri, seed=POINT_SEED):
    """points() of a named case, made once and shared; the arrays are read-only"""
    key = (name, seed)
    if key not in _made:
        pos, maxd, kinds = points(tri, seed=seed)
        pos.setflags(write=False); maxd.setflags(write=False)
        _made[key] = (pos, maxd, kinds)
    return _made[key]
