"""The arithmetic of light probes (kernels/probe_launch.h) restated in numpy, and the cases of tests/test_light_probes.py.
Every operation is one rounded binary32 operation in the order the header writes it; the kernels agree with these functions on bits."""
import os

import numpy as np

from tracerboy_amd import api

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = {"cornell-box": os.path.join(GOLDEN, "scenes", "cornell-box", "scene.pbrt"),
          "mix-glass": os.path.join(GOLDEN, "scenes", "mix-glass", "scene.pbrt"),
          "instances": os.path.join(GOLDEN, "scenes", "instances", "scene.pbrt")}

C0, C1, C2, C3, C4 = F32(0.28209479177387814), F32(0.4886025119029199), F32(1.0925484305920792), F32(0.31539156525252005), F32(0.5462742152960396)
PI = F32(3.1415926535)
FOUR_PI = F32(4.0) * PI
A0, A1, A2 = PI, F32(2.0943951), F32(0.7853982)
ONE, ZERO = F32(1), F32(0)


def _octahedron(M, T):
    """(px, py, z, h) of the M x M texel centres in the number type T, texel t = y * M + x"""
    T1, half = T(1), T(0.5)
    h = T(2.0) / T(M)
    c = (np.arange(M).astype(T) + half) * h - T1
    u = np.tile(c, M); v = np.repeat(c, M)
    au, av = np.abs(u), np.abs(v)
    z = (T1 - au) - av
    sgn = lambda a: np.where(a < 0, T(-1), T1).astype(T)
    px = np.where(z < 0, (T1 - av) * sgn(u), u).astype(T)
    py = np.where(z < 0, (T1 - au) * sgn(v), v).astype(T)
    return px, py, z, h


def directions(M, T=F32):
    """(dirs (M * M, 3), solid angles (M * M,), len2) of a map; T = np.float64 evaluates the same formulas in double"""
    px, py, z, h = _octahedron(M, T)
    len2 = ((px * px) + (py * py)) + z * z
    ln = np.sqrt(len2)
    d = np.stack([px / ln, py / ln, z / ln], axis=1)
    w = (h * h) / (len2 * ln)
    assert d.dtype == T and w.dtype == T
    return d, w, len2


def basis(d):
    """Y0 .. Y8 of unit vectors (..., 3): (..., 9), in the number type of d"""
    T = d.dtype.type
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c0, c1, c2, c3, c4 = (T(C0), T(C1), T(C2), T(C3), T(C4)) if T is F32 else (T(0.28209479177387814), T(0.4886025119029199), T(1.0925484305920792),
                                                                                T(0.31539156525252005), T(0.5462742152960396))
    Y = np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * ((T(3) * (z * z)) - T(1)), c2 * (x * z),
                  c4 * ((x * x) - (y * y))], axis=-1)
    assert Y.dtype == d.dtype
    return Y


def rays(positions, M, first_number=0):
    """(radiance records, distance records), each (n, M * M), of probes at `positions` numbered from first_number"""
    p = np.asarray(positions, F32)
    n, texels = p.shape[0], M * M
    d, _, _ = directions(M)
    rad = np.zeros((n, texels), api.RADIANCE_RAY_DTYPE); qry = np.zeros((n, texels), api.QUERY_RAY_DTYPE)
    ok = np.isfinite(p).all(axis=1)
    rad["Origin"][ok] = p[ok, None, :]; rad["Direction"][ok] = d[None]
    rad["SeedX"][ok] = (np.uint32(first_number) + np.arange(n, dtype=np.uint32)).astype(F32)[ok, None]
    rad["SeedY"][ok] = np.arange(texels, dtype=np.uint32).astype(F32)[None]
    qry["Origin"][ok] = p[ok, None, :]; qry["Direction"][ok] = d[None]; qry["TMax"][ok] = np.inf
    return rad, qry


def project(positions, M, sums, hits):
    """The records of probe_project: lane l folds the rays l, l + 64, ... in ascending order, six butterfly steps combine the lanes."""
    p = np.asarray(positions, F32)
    n, texels = p.shape[0], M * M
    sums = np.asarray(sums, F32).reshape(n, texels, 4); hits = np.asarray(hits).reshape(n, texels)
    d, w, _ = directions(M)
    Y = basis(d)
    lanes = np.arange(64)
    acc = np.zeros((n, 64, 27), F32); W = np.zeros((n, 64), F32); D = np.zeros((n, 64), F32); H = np.zeros((n, 64), F32); B = np.zeros((n, 64), F32)
    Dmin = np.full((n, 64), np.inf, F32)
    with np.errstate(all="ignore"):
        for r in range((texels + 63) // 64):
            t = lanes + 64 * r
            live = t < texels
            t = np.minimum(t, texels - 1)
            s = sums[:, t, :]; a = s[..., 3]
            counts = live[None] & (a > 0)
            q = ((s[..., :3] / a[..., None]) * w[t][None, :, None]).astype(F32)                   # (n, 64, 3)
            add = (q[:, :, None, :] * Y[t][None, :, :, None]).astype(F32).reshape(n, 64, 27)      # j * 3 + c
            acc = np.where(counts[..., None], acc + add, acc)
            W = np.where(counts, W + w[t][None], W)
            T = hits["T"][:, t]; N = hits["Normal"][:, t, :]
            met = live[None] & (T >= 0)
            D = np.where(met, D + T, D); H = np.where(met, H + ONE, H); Dmin = np.where(met, np.fmin(Dmin, T), Dmin)
            dot = ((N[..., 0] * d[t, 0][None]) + (N[..., 1] * d[t, 1][None])) + N[..., 2] * d[t, 2][None]
            B = np.where(met & (dot > 0), B + ONE, B)
        for distance in (32, 16, 8, 4, 2, 1):
            o = lanes ^ distance
            acc = acc + acc[:, o]; W = W + W[:, o]; D = D + D[:, o]; H = H + H[:, o]; B = B + B[:, o]
            Dmin = np.fmin(Dmin, Dmin[:, o])
        assert acc.dtype == F32 and W.dtype == F32 and D.dtype == F32
        acc, W, D, H, B, Dmin = acc[:, 0], W[:, 0], D[:, 0], H[:, 0], B[:, 0], Dmin[:, 0]
        placed = np.isfinite(p).all(axis=1)
        lit = placed & (W != 0); met = placed & (H != 0)
        out = np.zeros(n, api.PROBE_DTYPE)
        out["SH"] = np.where(lit[:, None], (FOUR_PI * acc) / W[:, None], ZERO).astype(F32).reshape(n, 9, 3)
        out["Weight"] = np.where(placed, W, ZERO); out["Hits"] = np.where(placed, H, ZERO); out["Backfaces"] = np.where(placed, B, ZERO)
        out["MinDistance"] = np.where(met, Dmin, F32(-1)); out["MeanDistance"] = np.where(met, D / H, F32(-1))
    return out


def irradiance(sh, normals):
    """E of records: sh (..., 9, 3) float32, normals (..., 3) unit vectors; (..., 3)"""
    sh = np.asarray(sh, F32); Y = basis(np.asarray(normals, F32))[..., None]               # (..., 9, 1)
    s = lambda j: sh[..., j, :]
    y = lambda j: Y[..., j, :]
    with np.errstate(all="ignore"):
        e = (((A0 * s(0)) * y(0)) + (A1 * (((s(1) * y(1)) + (s(2) * y(2))) + (s(3) * y(3))))) \
            + (A2 * (((((s(4) * y(4)) + (s(5) * y(5))) + (s(6) * y(6))) + (s(7) * y(7))) + (s(8) * y(8))))
    assert e.dtype == F32
    return e


def sample(grid, M, backface_limit, probes, points, normals):
    """probe_sample: (n, 4) = (E_r, E_g, E_b, Wsum)"""
    probes = np.asarray(probes).view(api.PROBE_DTYPE).reshape(-1)
    P = np.asarray(points, F32); n = P.shape[0]
    origin, spacing, count = np.asarray(grid.origin, F32), np.asarray(grid.spacing, F32), np.asarray(grid.count, np.int64)
    with np.errstate(all="ignore"):
        g = (P - origin[None]) / spacing[None]
        g = np.fmin(np.fmax(g, ZERO), (count - 1).astype(F32)[None]).astype(F32)
        i0 = np.where(count[None] == 1, 0, np.minimum(np.floor(g).astype(np.int64), count[None] - 2))
        f = g - i0.astype(F32)
        most = F32(backface_limit) * F32(M * M)
        S = np.zeros((n, 27), F32); Wsum = np.zeros(n, F32)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            ix, iy, iz = (np.minimum(i0[:, a] + dd, count[a] - 1) for a, dd in ((0, dx), (1, dy), (2, dz)))
            wc = ((f[:, 0] if dx else ONE - f[:, 0]) * (f[:, 1] if dy else ONE - f[:, 1])) * (f[:, 2] if dz else ONE - f[:, 2])
            rec = probes[(iz * count[1] + iy) * count[0] + ix]
            ok = (rec["Weight"] > 0) & (rec["Backfaces"] <= most)
            S = np.where(ok[:, None], S + (wc[:, None] * rec["SH"].reshape(n, 27)), S)
            Wsum = np.where(ok, Wsum + wc, Wsum)
        assert S.dtype == F32 and Wsum.dtype == F32
        some = Wsum != 0
        E = irradiance((S / np.where(some, Wsum, ONE)[:, None]).reshape(n, 9, 3), normals)
    out = np.zeros((n, 4), F32)
    out[some, :3] = E[some]; out[some, 3] = Wsum[some]
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------

def synthetic_maps(n, M, seed):
    """Seeded answers of the two queries for n probes: sums spanning 24 orders of magnitude without a NaN, an infinity or a subnormal product; every
    fourth ray with no accepted sample; misses among the hits; probe 0 (where n > 1, else none) all misses."""
    rng = np.random.default_rng(seed)
    texels = M * M
    sums = np.zeros((n, texels, 4), F32)
    sums[..., :3] = (10.0 ** rng.uniform(-12, 12, (n, texels, 3))).astype(F32)
    sums[..., 3] = rng.integers(1, 1 << 12, (n, texels)).astype(F32)
    sums[..., 3][rng.random((n, texels)) < 0.25] = 0
    hits = np.zeros((n, texels), api.QUERY_HIT_DTYPE)
    hits["T"] = (10.0 ** rng.uniform(-3, 5, (n, texels))).astype(F32)
    nrm = rng.normal(size=(n, texels, 3)); hits["Normal"] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F32)
    miss = rng.random((n, texels)) < 0.3
    if n > 1:
        miss[0] = True
    hits["T"][miss] = -1; hits["Normal"][miss] = 0
    return sums, hits


def box(lo, hi, inward):
    """A closed axis-aligned box as (positions (24, 3), indices (12, 3), normals (24, 3)): four vertices of its own per face, so that a face's normal
    is its vertices' normal.  inward: the triangles' winding and the normals point into the box, else out of it."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    corner = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]             # counter-clockwise seen from outside
    centre = (lo + hi) / 2
    p, nrm, tri = [], [], []
    for q in quads:
        v = corner[list(q)]
        g = np.cross(v[1] - v[0], v[2] - v[0]); g = g / np.linalg.norm(g)
        assert np.dot(g, v.mean(0) - centre) > 0                                                              # the winding is what it says
        base = len(p)
        p += list(v); nrm += [(-g if inward else g)] * 4
        tri += [[base, base + 2, base + 1], [base, base + 3, base + 2]] if inward else [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return np.ascontiguousarray(p, F32), np.uint32(tri), np.ascontiguousarray(nrm, F32)
