"""The yardstick and the inputs of tests/test_lightmap_bake.py: the rules of kernels/bake_launch.h restated in numpy.

Every array is float32 and every line below is ONE rounded operation (+ - * / sqrt), in the order the header writes them; min, max, floor, abs, the
negation and the product with 0.5 are exact.  cover() -> the 64-bit keys of an atlas, texels() -> the ray records and texel records, resolve() and
dilate() -> the picture.  The triangle sets and the planar-projection atlas are seeded and built here with numpy alone."""
import ctypes as C
import os

import numpy as np

from conftest import GOLDEN, CORNELL
from tracerboy_amd import api

F32 = np.float32
NO_KEY = np.uint64(0xffffffffffffffff)
NONE = 0xffffffff
PI = F32(3.1415926535)
HALF, ONE, ZERO = F32(0.5), F32(1.0), F32(0.0)
TILE = 8
PROC_TRIANGLES, PROC_SEED = 40000, 1234                               # tests/ray_query_cases.py's procedural scene
ATLAS_W, ATLAS_H, ATLAS_SAMPLES, ATLAS_SEED = 48, 40, 4, 23
MATERIAL_MAPS = os.path.join(GOLDEN, "scenes", "material-maps", "scene.pbrt")
DYNAMIC = os.path.join(GOLDEN, "scenes", "dynamic")


def edge(ax, ay, bx, by, qx, qy):
    l = (bx - ax) * (qy - ay)
    r = (by - ay) * (qx - ax)
    return l - r


def offset(ax, ay, bx, by):
    return -(HALF * (np.abs(bx - ax) + np.abs(by - ay)))


class Setup:
    """Per triangle, in the rasteriser's order: ok, v (T, 3), px, py (T, 3), A, swapped, the clipped box x0, y0, x1, y1 (ints; undefined where not ok)."""


def setup(W, H, uv, tri):
    with np.errstate(all="ignore"):
        uv = np.ascontiguousarray(uv, F32).reshape(-1, 2); v = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3).astype(np.int64)
        s = Setup()
        px = uv[v, 0] * F32(W); py = uv[v, 1] * F32(H)                # (T, 3)
        finite = np.isfinite(px).all(1) & np.isfinite(py).all(1)
        A = edge(px[:, 0], py[:, 0], px[:, 1], py[:, 1], px[:, 2], py[:, 2])
        ok = finite & np.isfinite(A) & (A != 0)
        s.swapped = ok & (A < 0)
        order = np.where(s.swapped[:, None], [0, 2, 1], [0, 1, 2])
        s.v = np.take_along_axis(v, order, 1); s.px = np.take_along_axis(px, order, 1); s.py = np.take_along_axis(py, order, 1)
        s.A = edge(s.px[:, 0], s.py[:, 0], s.px[:, 1], s.py[:, 1], s.px[:, 2], s.py[:, 2])
        lox, hix = np.floor(s.px.min(1)), np.floor(s.px.max(1)); loy, hiy = np.floor(s.py.min(1)), np.floor(s.py.max(1))
        ok &= ~((hix < 0) | (hiy < 0) | (lox > F32(W) - ONE) | (loy > F32(H) - ONE))
        clip = lambda a, top: np.where(ok, np.clip(np.where(ok, a, 0), 0, top - 1), 0).astype(np.int64)
        s.x0, s.x1, s.y0, s.y1 = clip(lox, W), clip(hix, W), clip(loy, H), clip(hiy, H)
        s.ok = ok
        return s


def tile_counts(W, H, uv, tri):
    """Work items of bake_cover per triangle: the 8 x 8 tiles of the atlas its clipped box touches."""
    s = setup(W, H, uv, tri)
    return np.where(s.ok, (s.x1 // TILE - s.x0 // TILE + 1) * (s.y1 // TILE - s.y0 // TILE + 1), 0)


def cover(W, H, uv, tri):
    """(H, W) uint64 keys: (class << 32) | triangle of the smallest claim on each texel, all ones where nobody claims it."""
    s = setup(W, H, uv, tri)
    keys = np.full(W * H, NO_KEY, np.uint64)
    t = np.flatnonzero(s.ok)
    if not len(t):
        return keys.reshape(H, W)
    bw = s.x1[t] - s.x0[t] + 1; area = bw * (s.y1[t] - s.y0[t] + 1)
    who = np.repeat(t, area)                                           # one entry per (triangle, candidate texel)
    local = np.arange(area.sum()) - np.repeat(np.cumsum(area) - area, area)
    x = s.x0[who] + local % np.repeat(bw, area); y = s.y0[who] + local // np.repeat(bw, area)
    with np.errstate(all="ignore"):
        cx = x.astype(F32) + HALF; cy = y.astype(F32) + HALF
        p = lambda k: (s.px[who, k], s.py[who, k])
        e0 = edge(*p(1), *p(2), cx, cy); e1 = edge(*p(2), *p(0), cx, cy); e2 = edge(*p(0), *p(1), cx, cy)
        centre = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        touch = ~centre & (e0 >= offset(*p(1), *p(2))) & (e1 >= offset(*p(2), *p(0))) & (e2 >= offset(*p(0), *p(1)))
    claim = centre | touch
    key = (np.where(centre, 0, 1).astype(np.uint64) << np.uint64(32)) | who.astype(np.uint64)
    np.minimum.at(keys, (y * W + x)[claim], key[claim])
    return keys.reshape(H, W)


def _blend(a, b, c, w0, w1, w2):
    l = a * w0
    m = b * w1
    r = c * w2
    return (l + m) + r


def _len2(n):
    xx = n[:, 0] * n[:, 0]
    yy = n[:, 1] * n[:, 1]
    zz = n[:, 2] * n[:, 2]
    return (xx + yy) + zz


def texels(W, H, positions, normals, uv, tri, keys=None):
    """(rays, texel records) of shape (H, W): RADIANCE_RAY_DTYPE and BAKE_TEXEL_DTYPE, as bake_texels writes them."""
    keys = cover(W, H, uv, tri) if keys is None else keys
    P = np.ascontiguousarray(positions, F32).reshape(-1, 3); N = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    s = setup(W, H, uv, tri)
    rays = np.zeros(W * H, api.RADIANCE_RAY_DTYPE); rec = np.zeros(W * H, api.BAKE_TEXEL_DTYPE); rec["triangle"] = NONE
    at = np.flatnonzero(keys.reshape(-1) != NO_KEY)
    if not len(at):
        return rays.reshape(H, W), rec.reshape(H, W)
    k = keys.reshape(-1)[at]
    t = (k & np.uint64(0xffffffff)).astype(np.int64); cls = (k >> np.uint64(32)).astype(np.uint32)
    x = at % W; y = at // W
    with np.errstate(all="ignore"):
        cx = x.astype(F32) + HALF; cy = y.astype(F32) + HALF
        p = lambda j: (s.px[t, j], s.py[t, j])
        e0 = edge(*p(1), *p(2), cx, cy); e1 = edge(*p(2), *p(0), cx, cy)
        w0 = e0 / s.A[t]
        w1 = e1 / s.A[t]
        w2 = (ONE - w0) - w1
        c0, c1, c2 = (np.where(w > 0, w, ZERO) for w in (w0, w1, w2))
        total = (c0 + c1) + c2
        edge_texel = cls == 1
        w0 = np.where(edge_texel, c0 / total, w0); w1 = np.where(edge_texel, c1 / total, w1); w2 = np.where(edge_texel, c2 / total, w2)
        P0, P1, P2 = (P[s.v[t, j]] for j in range(3)); N0, N1, N2 = (N[s.v[t, j]] for j in range(3))
        o = _blend(P0, P1, P2, w0[:, None], w1[:, None], w2[:, None])
        n = _blend(N0, N1, N2, w0[:, None], w1[:, None], w2[:, None])
        len2 = _len2(n)
        shaded = np.isfinite(len2) & (len2 > 0)
        sw = s.swapped[t][:, None]
        Q1 = np.where(sw, P2, P1); Q2 = np.where(sw, P1, P2)          # the caller's winding
        a = Q1 - P0; b = Q2 - P0
        g = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        n = np.where(shaded[:, None], n, g)
        len2 = np.where(shaded, len2, _len2(g))
        good = np.isfinite(len2) & (len2 > 0)
        d = n / np.sqrt(len2)[:, None]
        good &= np.isfinite(o).all(1) & np.isfinite(d).all(1)
    i = at[good]
    rays["Origin"][i] = o[good]; rays["Direction"][i] = d[good]; rays["SeedX"][i] = x[good].astype(F32); rays["SeedY"][i] = y[good].astype(F32)
    rec["triangle"][i] = t[good].astype(np.uint32); rec["cls"][i] = cls[good]; rec["w0"][i] = w0[good]
    rec["w1"][i] = np.where(s.swapped[t], w2, w1)[good]
    return rays.reshape(H, W), rec.reshape(H, W)


def resolve(rec, sums):
    """(H, W, 4): rgb = (PI * sum) / a3 and alpha 1 on texels with a triangle and a3 > 0, zeros elsewhere."""
    s = np.ascontiguousarray(sums, F32).reshape(rec.shape + (4,))
    with np.errstate(all="ignore"):
        scaled = PI * s[..., :3]
        rgb = scaled / s[..., 3:4]
    lit = (rec["triangle"] != NONE) & (s[..., 3] > 0)
    out = np.zeros(rec.shape + (4,), F32)
    out[lit, :3] = rgb[lit]; out[lit, 3] = ONE
    return out


def dilate(rgba, passes):
    """`passes` fill passes (pass p gives alpha 2^-p), neighbours summed in row-major order from 0."""
    cur = np.ascontiguousarray(rgba, F32).copy()
    H, W = cur.shape[:2]
    for p in range(1, passes + 1):
        pad = np.zeros((H + 2, W + 2, 4), F32); pad[1:-1, 1:-1] = cur  # outside the atlas: alpha 0, never counted
        total = np.zeros((H, W, 3), F32); m = np.zeros((H, W), np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                use = q[..., 3] > 0
                total = np.where(use[..., None], total + q[..., :3], total)
                m += use
        fill = ~(cur[..., 3] > 0) & (m > 0)
        with np.errstate(all="ignore"):
            mean = total / m.astype(F32)[..., None]
        nxt = cur.copy()
        nxt[fill, :3] = mean[fill]; nxt[fill, 3] = F32(2.0 ** -p)
        cur = nxt
    return cur


# ---- triangle sets: (positions (n, 3), normals (n, 3), uvs (n, 2), triangles (t, 3)) ----------------------------------------------------------

def soup(uv_triangles, seed=1):
    """Unshared vertices for (t, 3, 2) UV triangles: positions on a seeded slanted plane over the UV square, normals seeded and not unit."""
    uvt = np.asarray(uv_triangles, F32).reshape(-1, 3, 2)
    rng = np.random.default_rng(seed)
    uv = uvt.reshape(-1, 2)
    pos = np.stack([uv[:, 0] * F32(3.0), uv[:, 1] * F32(2.0), uv[:, 0] + uv[:, 1]], 1).astype(F32)
    nrm = (rng.normal(size=pos.shape) + [0, 0, 3]).astype(F32)
    return pos, nrm, uv.copy(), np.arange(len(uv), dtype=np.uint32).reshape(-1, 3)


def in_texels(points, W, H):
    """UVs of points given in texel units."""
    return (np.asarray(points, np.float64) / [W, H]).astype(F32)


def hand_right_triangle(W=8, H=8):
    return soup(in_texels([[[0, 0], [4, 0], [0, 4]]], W, H))


def hand_quad(W=8, H=8):
    """Two triangles that share the diagonal (0, 0) - (6, 6) of a quad."""
    return soup(in_texels([[[0, 0], [6, 0], [6, 6]], [[0, 0], [6, 6], [0, 6]]], W, H))


def hand_degenerate(W=8, H=8):
    """A triangle of area 0 and one with a NaN UV."""
    uvt = in_texels([[[1, 1], [3, 3], [5, 5]], [[1, 1], [4, 1], [1, 4]]], W, H)
    uvt[1, 2, 0] = np.nan
    return soup(uvt)


def hand_small(W=8, H=8):
    """A 0.2-texel triangle inside texel (2, 3), off its centre."""
    return soup(in_texels([[[2.1, 3.1], [2.3, 3.1], [2.1, 3.3]]], W, H))


def mirrored(case):
    pos, nrm, uv, tri = case
    return pos, nrm, uv, np.ascontiguousarray(tri[:, [0, 2, 1]])


def reversed_order(case):
    pos, nrm, uv, tri = case
    return pos, nrm, uv, np.ascontiguousarray(tri[::-1])


def random_triangles(n=300, seed=5, large=0.3):
    """Seeded triangles with UVs in [-0.25, 1.25]: a share of large ones that leave the atlas on every side, the rest small."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.25, 1.25, (n, 1, 2)); size = np.where(rng.random((n, 1, 1)) < large, 0.6, 0.08)
    uvt = np.clip(centre + rng.uniform(-1, 1, (n, 3, 2)) * size, -0.25, 1.25).astype(F32)
    return soup(uvt, seed)


def skewed(W, H, small=200, seed=6):
    """`small` sub-texel triangles FIRST (the lower indices), then one quad over the whole atlas as two triangles."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (small, 1, 2)) * [W, H]
    tiny = c + rng.uniform(-0.3, 0.3, (small, 3, 2))
    quad = [[[0, 0], [W, 0], [W, H]], [[0, 0], [W, H], [0, H]]]
    return soup(in_texels(np.concatenate([tiny, quad]), W, H), seed)


def zero_normals(case):
    """Every second triangle's vertex normals are zero: the geometric normal stands in."""
    pos, nrm, uv, tri = case
    nrm = nrm.copy(); nrm[tri[::2].reshape(-1)] = 0
    return pos, nrm, uv, tri


def collapsed_positions(case):
    """Every second triangle's positions coincide and its normals are zero: no direction can be made, the texel is uncovered."""
    pos, nrm, uv, tri = zero_normals(case)
    pos = pos.copy(); pos[tri[::2, 1]] = pos[tri[::2, 0]]; pos[tri[::2, 2]] = pos[tri[::2, 0]]
    return pos, nrm, uv, tri


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------

def vertex_records(view):
    """(numVertices, 8) float32: normal, uv, tangent of the scene's vertex records."""
    return np.ctypeslib.as_array(view.vertexBuffer, shape=(view.numVertexFloats // 8, 8)).copy()


def geometry_ranges(view):
    """(first vertex, count) per geometry (hit-group record), as tb_geometry_vertex_range gives them."""
    groups = np.ctypeslib.as_array(C.cast(view.hitGroups, C.POINTER(C.c_uint32)), shape=(view.numHitGroups, 18))
    nv = view.numVertexFloats // 8
    firsts = sorted(set(int(o) // 32 for o in groups[:, 10])) + [nv]
    return [(int(groups[g, 10]) // 32, firsts[firsts.index(int(groups[g, 10]) // 32) + 1] - int(groups[g, 10]) // 32) for g in range(view.numHitGroups)]


def planar_atlas(positions, ranges, seed=ATLAS_SEED, margin=0.08):
    """Lightmap UVs by planar projection: geometry g gets cell g of a square grid, its vertices projected along its thinnest axis (the two kept axes
    in a seeded order) onto the cell less a margin.  Faces seen edge-on come out with area 0 and faces behind one another overlap: both are cases
    the rasteriser has rules for."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(positions, np.float64).reshape(-1, 3)
    cols = int(np.ceil(np.sqrt(max(len(ranges), 1))))
    uv = np.zeros((len(pos), 2), np.float64)
    for g, (first, count) in enumerate(ranges):
        flip = rng.random() < 0.5
        if not count:
            continue
        p = pos[first:first + count]
        ext = p.max(0) - p.min(0)
        axes = np.argsort(-ext, kind="stable")[:2]
        if flip:
            axes = axes[::-1]
        q = (p[:, axes] - p.min(0)[axes]) / np.maximum(ext[axes], 1e-30)
        cell = np.array([g % cols, g // cols], np.float64)
        uv[first:first + count] = (cell + margin + q * (1 - 2 * margin)) / cols
    return uv.astype(F32)
