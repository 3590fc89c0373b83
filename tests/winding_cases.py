"""The inputs and the yardsticks of tests/test_winding_numbers.py: numpy only.

The closed meshes are made as triangle soups, (N, 3, 3) float32, wound so that tb_face_vector (include/tb_normals.h) points outward -- the winding
number inside is +1 -- and handed over like the cases of tests/adversarial_cases.py, whose soups are the other cases: there w is arbitrary, and they
are compared on bits and for accuracy only.  winding64 is the float64 sum of 2 arctan2 over every triangle: it shares no tree, no order and no fp32
with the code it judges.  The points are tests/nearest_cases.py's."""
import numpy as np

import adversarial_cases as ac
import nearest_cases as nc

F32 = np.float32
SEEDS = (nc.POINT_SEED, nc.POINT_SEED + 1, nc.POINT_SEED + 2)
ON_SURFACE_KINDS = ("surface", "vertex", "not_finite")
# A point is OFF THE SURFACE when its kind is none of these and its float64 distance to the nearest triangle (nearest_cases.distance64) is at least
# 2^-23 M, M the largest coordinate magnitude of scene and point (nearest_cases.scale): one step of the binary32 grid the coordinates live on.  The
# kinds alone do not decide it: a "near" point is a surface point plus an offset of as little as 10^-6 extents, which the rounding of the position to
# binary32 can swallow whole or leave in the triangle's plane -- of the 138 888 points of ACCURACY_NAMES x SEEDS that the kinds call off-surface, 404
# lie nearer than that, one of them (tetra4, seed 72) at distance 0.  Below one grid step the representable neighbours of the position lie on both
# sides of the triangle, float64 arithmetic on the rounded position (winding64) still picks a side, and no binary32 evaluation of a . (b x c) can be
# asked to pick the same one: at three of the 404 (tetra4 / 72 at 0, rand8 / 70 at 0.0018, rand3 / 72 at 0.011 grid steps) the library's exact
# form is off by 1.  The bound comes from the number format, not from those three: the other 401 points agree to 5 x 10^-5 and are left out all the same.

# |w - winding64| of the exact form -- the host brute force, and the host walk at beta = inf under the builders 0, 1 and 3 -- over every case here and
# every case of adversarial_cases.NAMES but zero32, the point seeds 70, 71, 72, every off-surface point, none left out.  Measured on the CPU with the
# library's host code (scripts/winding_accuracy.py): the worst is W_EXACT_MEASURED, at W_EXACT_WORST; W_EXACT_TOL is the next power of two above
# twice that.
W_EXACT_MEASURED = 1.107448e-03
W_EXACT_WORST = "rand512, seed 72, the walk at beta = inf over builder 1's tree"
W_EXACT_TOL = 2.0 ** -8
# The same for the host walk with far subtrees as dipoles, builders 0, 1 and 3, at beta = 2 and 4 -- and at 3: the worst at 2 is 0.0643, twice that
# is above 2^-3, so W_BETA_TOL[2] is 2^-2, which is not BELOW 0.25 as a default beta must be; 3 is the smallest of 3 and 4 whose tolerance is, and is
# the default (api.WINDING_BETA).
W_BETA_MEASURED = {2.0: 6.426066e-02, 3.0: 1.050484e-02, 4.0: 3.413101e-03}
W_BETA_WORST = {2.0: "nested40, seed 72, builder 3", 3.0: "split65, seed 71, builder 0", 4.0: "split65, seed 71, builder 1"}
W_BETA_TOL = {2.0: 2.0 ** -2, 3.0: 2.0 ** -5, 4.0: 2.0 ** -7}
DEFAULT_BETA = 3.0
assert not W_BETA_TOL[2.0] < 0.25 and W_BETA_TOL[DEFAULT_BETA] < 0.25


def _quads(corners, quads):
    return F32([[corners[q[0]], corners[q[a]], corners[q[a + 1]]] for q in quads for a in (1, 2)])


def cube12(lo=0.0, hi=1.0):
    """the cube [lo, hi]^3, 12 triangles, every face vector outward"""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float64)   # index = 4 x + 2 y + z
    return _quads(c, [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)])   # -x, +x, -y, +y, -z, +z


def reverse(tri):
    return np.ascontiguousarray(tri[:, ::-1])


def tetra4():
    """a regular tetrahedron: convex, and every edge is the meeting of two faces at 70.5 degrees"""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    return F32([[v[0], v[1], v[2]], [v[0], v[2], v[3]], [v[0], v[3], v[1]], [v[1], v[3], v[2]]])


def _prism(poly, caps, z0, z1):
    """a counter-clockwise polygon (n, 2), triangulated by `caps` (index triples, counter-clockwise), extruded from z0 to z1"""
    at = lambda k, z: [poly[k][0], poly[k][1], z]
    tri = []
    for a, b, c in caps:
        tri.append([at(a, z0), at(c, z0), at(b, z0)])               # bottom: faces -z
        tri.append([at(a, z1), at(b, z1), at(c, z1)])               # top: faces +z
    n = len(poly)
    for i in range(n):
        j = (i + 1) % n
        tri.append([at(i, z0), at(j, z0), at(j, z1)])
        tri.append([at(i, z0), at(j, z1), at(i, z1)])
    return F32(tri)


def star40():
    """a five-armed star (ten corners, radii 1 and 0.35) extruded by 0.3: acute edges at the tips, reflex ones between them; the caps are fans
    around the centre"""
    ang = np.arange(10) * np.pi / 5
    rad = np.where(np.arange(10) % 2 == 0, 1.0, 0.35)
    poly = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    sides = _prism(poly, [], 0.0, 0.3)
    caps = []
    for i in range(10):
        (px, py), (qx, qy) = poly[i], poly[(i + 1) % 10]
        caps += [[[0, 0, 0], [qx, qy, 0], [px, py, 0]], [[0, 0, 0.3], [px, py, 0.3], [qx, qy, 0.3]]]
    return np.concatenate([F32(caps), sides])


def lprism20():
    """an L-shaped prism: one reflex edge"""
    poly = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)
    return _prism(poly, [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)], 0.0, 1.0)


def torus256(nu=16, nv=8, R=1.0, r=0.4):
    u = np.arange(nu + 1) * 2 * np.pi / nu; v = np.arange(nv + 1) * 2 * np.pi / nv
    P = lambda i, j: [(R + r * np.cos(v[j % nv])) * np.cos(u[i % nu]), (R + r * np.cos(v[j % nv])) * np.sin(u[i % nu]), r * np.sin(v[j % nv])]
    tri = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1)
            tri += [[a, b, c], [a, c, d]]
    return F32(tri)


def shell():
    """cube12 with a reversed half-size cube inside: w = 1 in the wall, 0 in the cavity"""
    return np.concatenate([cube12(), reverse(cube12(0.25, 0.75))])


def twice():
    """cube12 twice over: w = 2 inside"""
    return np.concatenate([cube12(), cube12()])


def open5():
    """cube12 without its top (+z): not closed, w falls off smoothly through the hole"""
    return np.ascontiguousarray(cube12()[:10])


CLOSED = {"tetra4": tetra4, "cube12": cube12, "star40": star40, "lprism20": lprism20, "torus256": torus256, "shell": shell, "twice": twice}
OWN = dict(CLOSED, open5=open5)
INSIDE = {"tetra4": (0, 0, 0), "cube12": (0.5, 0.5, 0.5), "star40": (0.1, 0.05, 0.15), "lprism20": (0.5, 1.5, 0.5), "torus256": (1.0, 0.0, 0.0),
          "shell": (0.125, 0.5, 0.5), "twice": (0.5, 0.5, 0.5)}
INSIDE_W = {"twice": 2.0}
SIZES = {"tetra4": 4, "cube12": 12, "star40": 40, "lprism20": 20, "torus256": 256, "shell": 24, "twice": 24, "open5": 10}
NAMES = list(OWN) + list(ac.NAMES)
ACCURACY_NAMES = [n for n in NAMES if n != "zero32"]
_made = {}


def winding64(tri, p):
    """(n,) float64: the winding number of the triangles (T, 3, 3) at every point, the sum of 2 arctan2(a . (b x c), |a||b||c| + (a . b)|c| +
    (b . c)|a| + (c . a)|b|) / 4 pi"""
    tri = tri.astype(np.float64); p = np.asarray(p, np.float64)
    out = np.empty(len(p))
    for r0 in range(0, len(p), 256):
        P = p[r0:r0 + 256, None, :]
        a, b, c = tri[None, :, 0] - P, tri[None, :, 1] - P, tri[None, :, 2] - P
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[r0:r0 + 256] = (2.0 * np.arctan2(num, den)).sum(axis=1)
    return out / (4.0 * np.pi)


def triangles(name):
    if name in ac.CASES:
        return ac.triangles(name)
    if name not in _made:
        t = np.ascontiguousarray(OWN[name](), F32)
        assert t.shape == (SIZES[name], 3, 3) and np.isfinite(t).all()
        if name in CLOSED:                                           # closed and outward: an edge and its reverse pair up, and w inside is +1
            e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).reshape(-1, 6)
            fwd = sorted(map(tuple, e)); back = sorted(map(tuple, e[:, [3, 4, 5, 0, 1, 2]]))
            assert fwd == back, name
            assert abs(winding64(t, np.array([INSIDE[name]]))[0] - INSIDE_W.get(name, 1.0)) < 1e-12, name
        t.setflags(write=False)
        _made[name] = t
    return _made[name]


def off_surface(tri, pos, kinds):
    off = ~np.isin(kinds, ON_SURFACE_KINDS)
    idx = np.flatnonzero(off)
    off[idx] = nc.distance64(tri, pos[idx]) >= nc.ULP * nc.scale(tri, pos[idx])
    # the distance rule takes a few points out (0.3 % overall; most where one triangle is the whole scene and 2^-23 M is largest against the smallest
    # offsets, 10^-6 extents), never a case's worth: a change of nc.scale or nc.distance64 that emptied the tests would show here
    assert off.sum() >= 0.98 * len(idx), (int(off.sum()), len(idx))
    return off


_truth = {}


def truth(name, seed=nc.POINT_SEED, tri=None, key=None):
    """(positions, kinds, off-surface mask, winding64) of the case's points -- `tri` with `key`: of other positions for it, the moved tests' --
    made once and shared; the arrays are read-only"""
    k = (key or name, seed)
    if k not in _truth:
        t = triangles(name) if tri is None else tri
        pos, maxd, kinds = nc.case_points("winding/" + (key or name), t, seed)
        off = off_surface(t, pos, kinds)
        w = np.full(len(pos), np.nan)
        w[off] = winding64(t, pos[off])
        w.setflags(write=False); off.setflags(write=False)
        _truth[k] = (pos, kinds, off, w)
    return _truth[k]
