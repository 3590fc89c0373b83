"""The yardstick and the inputs of tests/test_mesh_scenes.py.

smooth_normals restates include/tb_normals.h in numpy float32: every line is ONE rounded operation, in the order tb_vec.h writes them; fma32 is a
correctly rounded float32 fused multiply-add (the product of two float32 is exact in float64; the sum is rounded to odd there, which makes the final
rounding to float32 the single rounding of the exact value -- pinned against exact rationals by the tests).  The meshes are the smallest shapes on
which the rule can go wrong, built here with numpy alone; cut_meshes turns a host scene's view back into the arrays it could have come from."""
import ctypes as C

import numpy as np

from tracerboy_amd import _ctypes_abi as abi, api

F32 = np.float32
MAT_NO_SPECULAR, MAT_LIGHT, MAT_NO_ALPHA = 0x4, 0x10, 0x20
INVALID_TEXTURE = 0xffffffff
DISPLACE_SEED = 41
THRESHOLD = F32(0.0000000001)


def fma32(a, b, c):
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                                     # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                                 # TwoSum: s + e is the exact sum
        even = ((np.ascontiguousarray(s).view(np.int64) & 1) == 0).reshape(np.shape(s))
        fix = np.isfinite(s) & (e != 0) & even                        # round to odd: the inexact sum's other neighbour
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def dot(a, b):
    """tb3_dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))"""
    xx = a[..., 0] * b[..., 0]
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], xx))


def cross(a, b):
    """tb3_cross: each component a product minus a product, unfused"""
    def comp(p, q, r, s):
        l = p * q
        m = r * s
        return l - m
    return np.stack([comp(a[..., 1], b[..., 2], a[..., 2], b[..., 1]), comp(a[..., 2], b[..., 0], a[..., 0], b[..., 2]),
                     comp(a[..., 0], b[..., 1], a[..., 1], b[..., 0])], axis=-1).astype(F32)


def face_vectors(positions, indices):
    p = np.ascontiguousarray(positions, F32); i = np.ascontiguousarray(indices, np.uint32).astype(np.int64)
    with np.errstate(all="ignore"):
        e1 = p[i[:, 2]] - p[i[:, 0]]
        e2 = p[i[:, 2]] - p[i[:, 1]]
        return cross(e1, e2)


def smooth_normals(positions, indices, start=None):
    """(n, 3) normals by the rule; a vertex that no triangle names keeps `start`'s row ((0, 1, 0) without one)."""
    p = np.ascontiguousarray(positions, F32); idx = np.ascontiguousarray(indices, np.uint32).astype(np.int64)
    f = face_vectors(p, idx)
    acc = np.zeros_like(p); named = np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for t in range(len(idx)):                                     # ascending primitive index, corners 0, 1, 2
            for k in range(3):
                v = idx[t, k]
                acc[v] = acc[v] + f[t]
                named[v] = True
        d = dot(acc, acc)
        inv = F32(1.0) / np.sqrt(d).astype(F32)
        unit = (acc * inv[:, None]).astype(F32)
    out = np.zeros_like(p) if start is None else np.array(start, F32)
    if start is None:
        out[:, 1] = 1.0
    fallback = d <= THRESHOLD                                         # NaN compares false: what is not finite is stored as it comes
    out[named] = np.where(fallback[named, None], F32([0, 1, 0]), unit[named])
    return out


# ---- materials -------------------------------------------------------------------------------------------------------------------------------

def matte(r, g, b):
    m = abi.TbMaterial()
    m.albedo = abi.TbFloat3(r, g, b); m.IOR = 1.5
    m.albedoIndex = m.alphaIndex = m.normalMapIndex = m.emissiveIndex = m.specularMapIndex = INVALID_TEXTURE
    m.Flags = MAT_NO_ALPHA | MAT_NO_SPECULAR
    return m


def emitter(r, g, b):
    m = matte(0, 0, 0)
    m.emissive = abi.TbFloat3(r, g, b); m.Flags |= MAT_LIGHT
    return m


MATERIALS = lambda: [matte(0.7, 0.6, 0.5), matte(0.2, 0.5, 0.7), emitter(17.0, 12.0, 4.0)]


# ---- meshes: (positions (n, 3) float32, indices (m, 3) uint32) ---------------------------------------------------------------------------------

def one_triangle():
    return F32([[-1, 0, 0], [1, 0, 0.25], [0, 2, -0.25]]), np.uint32([[0, 1, 2]])


def fan(n=70, seed=3):
    """n triangles around vertex 0, a valence above a wave's 64 lanes; the rim wobbles so that no two face vectors are equal."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 1.75 * np.pi, n + 1)
    rim = np.stack([np.cos(a) * (1 + 0.2 * rng.uniform(-1, 1, n + 1)), 0.3 * rng.uniform(-1, 1, n + 1), np.sin(a) * (1 + 0.2 * rng.uniform(-1, 1, n + 1))], 1)
    p = np.concatenate([[[0.0, 0.4, 0.0]], rim]).astype(F32)
    i = np.stack([np.zeros(n), np.arange(2, n + 2), np.arange(1, n + 1)], 1).astype(np.uint32)       # wound to face up
    return p, i


def unnamed_vertex():
    p, i = one_triangle()
    return np.concatenate([p, F32([[5, 5, 5]])]), i


def zero_area():
    """a triangle of no area alone on its vertices beside a real one: its three vertices get the fallback"""
    return F32([[-1, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [3, 3, 3], [4, 4, 4]]), np.uint32([[0, 1, 2], [3, 4, 5]])


def twice_named():
    """triangle 1 names vertex 2 twice"""
    return F32([[-1, 0, 0], [1, 0, 0.5], [0, 1, 0], [0.5, 2, 1]]), np.uint32([[0, 1, 2], [2, 2, 3]])


def blob(rings=16, segs=17, seed=5):
    """A closed displaced sphere: 2 + (rings - 1) * segs = 257 vertices, no multiple of 64 or 256; 2 * segs * (rings - 1) = 510 triangles."""
    rng = np.random.default_rng(seed)
    pts = [[0.0, 1.0, 0.0]]
    for r in range(1, rings):
        th = np.pi * r / rings
        for s in range(segs):
            ph = 2 * np.pi * s / segs
            pts.append([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])
    pts.append([0.0, -1.0, 0.0])
    p = np.array(pts) * (1 + 0.15 * rng.uniform(-1, 1, (len(pts), 1)))
    tri = []
    ring = lambda r, s: 1 + (r - 1) * segs + s % segs
    last = len(pts) - 1
    for s in range(segs):
        tri.append([0, ring(1, s + 1), ring(1, s)])
        tri.append([last, ring(rings - 1, s), ring(rings - 1, s + 1)])
    for r in range(1, rings - 1):
        for s in range(segs):
            a, b, c, d = ring(r, s), ring(r, s + 1), ring(r + 1, s), ring(r + 1, s + 1)
            tri.append([a, b, d]); tri.append([a, d, c])
    return p.astype(F32), np.uint32(tri)


def quad(y=3.0, h=0.6):
    """an emissive quad facing down, with its normals"""
    p = F32([[-h, y, -h], [h, y, -h], [h, y, h], [-h, y, h]])
    return p, np.uint32([[0, 1, 2], [0, 2, 3]]), np.tile(F32([0, -1, 0]), (4, 1))


RULE_CASES = {"one triangle": one_triangle, "fan of 70": fan, "unnamed vertex": unnamed_vertex, "zero area": zero_area, "twice named": twice_named,
              "blob of 257": blob}


def planar_uvs(p):
    """x, z of the bounds onto [0.05, 0.95]^2: an atlas for the bake"""
    lo, hi = p.min(0), p.max(0)
    return np.ascontiguousarray((0.05 + 0.9 * (p[:, [0, 2]] - lo[[0, 2]]) / np.maximum(hi[[0, 2]] - lo[[0, 2]], 1e-6)).astype(F32))


def fan_and_quad(offset=(0.0, 0.0, 0.0)):
    """[fan with smooth normals and UVs, emissive quad over it] and their materials"""
    fp, fi = fan(); qp, qi, qn = quad()
    fp = (fp + F32(offset)).astype(F32); qp = (qp + F32(offset)).astype(F32)
    quv = (0.96 + 0.03 * F32([[0, 0], [1, 0], [1, 1], [0, 1]])).astype(F32)
    return [api.Mesh(fp, fi, uvs=planar_uvs(fp), material=0, smooth=True), api.Mesh(qp, qi, normals=qn, uvs=quv, material=2)], MATERIALS()


def blob_fan_quad():
    """three meshes, so that the later ranges do not start at 0: the blob (smooth, mesh 0), the fan beside it (smooth, mesh 1), the quad over both"""
    bp, bi = blob()
    rest, materials = fan_and_quad(offset=(2.5, 0.0, 0.0))
    return [api.Mesh(bp, bi, uvs=planar_uvs(bp), material=1, smooth=True)] + rest, materials


def to_torch(meshes, device="cuda:0", int32=False):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = []
    for m in meshes:
        idx = torch.from_numpy(m.indices.astype(np.int32)).to(device) if int32 or not hasattr(torch, "uint32") else t(m.indices)
        out.append(api.Mesh(t(m.positions), idx, t(m.normals), t(m.uvs), m.material, m.smooth))
    return out


def displaced(positions, seed=DISPLACE_SEED, fraction=0.04):
    rng = np.random.default_rng(seed)
    ext = float(np.max(positions.max(0) - positions.min(0)))
    return (positions + rng.uniform(-1, 1, positions.shape) * fraction * ext).astype(F32)


# ---- a host scene's view back into arrays ------------------------------------------------------------------------------------------------------

def hit_groups(view):
    return np.ctypeslib.as_array(C.cast(view.hitGroups, C.POINTER(C.c_uint32)), shape=(view.numHitGroups, 18)).copy()


def vertex_buffer(view):
    return np.ctypeslib.as_array(view.vertexBuffer, shape=(view.numVertexFloats // 8, 8)).copy()


def index_buffer(view):
    return np.ctypeslib.as_array(view.indexBuffer, shape=(view.numIndices,)).copy()


def materials_of(view):
    return [abi.TbMaterial.from_buffer_copy(view.materials[i]) for i in range(view.numMaterials)]


def material_bytes(view):
    return np.frombuffer(C.string_at(view.materials, view.numMaterials * C.sizeof(abi.TbMaterial)), np.uint8).copy()


def lights_of(view):
    """(numLights, 26) words: LightType 0, LightColor 1:4, SurfaceArea 4, P0..P2 5:14, N0..N2 14:23, Direction 23:26"""
    if not view.numLights:
        return np.zeros((0, 26), np.uint32)
    return np.frombuffer(C.string_at(view.lights, view.numLights * 104), np.uint32).reshape(-1, 26).copy()


def cut_meshes(hs):
    """(meshes, materials) of a one-level host scene: per hit-group record its vertices (positions from triangles(), normals and UVs from the vertex
    records, passed as given) and its mesh-local indices."""
    view = hs.view(); tri = hs.triangles()
    groups = hit_groups(view); vb = vertex_buffer(view); ib = index_buffer(view)
    nv = len(vb)
    firsts = sorted(int(o) // 32 for o in groups[:, 10]) + [nv]
    meshes = []
    for g in range(view.numHitGroups):
        first = int(groups[g, 10]) // 32; end = firsts[firsts.index(first) + 1]
        ntri = int((tri["tri_geometry"] == g).sum())
        i0 = int(groups[g, 12]) // 4
        meshes.append(api.Mesh(np.ascontiguousarray(tri["positions"][first:end]), np.ascontiguousarray(ib[i0:i0 + 3 * ntri].reshape(-1, 3)),
                               normals=np.ascontiguousarray(vb[first:end, 0:3]), uvs=np.ascontiguousarray(vb[first:end, 3:5]), material=int(groups[g, 8])))
    return meshes, materials_of(view)


def vertex_ranges(meshes):
    first, out = 0, []
    for m in meshes:
        out.append((first, int(m.positions.shape[0]))); first += int(m.positions.shape[0])
    return out


def default_camera(positions):
    """The documented default camera in float32, operation by operation (procedural.cpp SetLookAtCamera, 35 degrees): a dict of the tb_camera fields."""
    import math
    p = np.concatenate([np.ascontiguousarray(q, F32) for q in positions])
    mn, mx = p.min(0), p.max(0)
    c = ((mn + mx) * F32(0.5)).astype(F32)
    ext = (mx - mn).astype(F32)
    diagonal = np.sqrt(dot(ext, ext)).astype(F32)
    d = F32(2.0) * diagonal if diagonal > 0 else F32(1.0)
    eye = np.array([c[0], c[1] + F32(0.35) * d, c[2] + d], F32)
    normalize = lambda v: (v * (F32(1.0) / np.sqrt(dot(v, v)).astype(F32))).astype(F32)
    view = normalize((c - eye).astype(F32))
    right = normalize(cross(F32([0, 1, 0]), view))
    up = cross(view, right)
    focal = F32(1.0 / math.tan(35.0 * math.pi / 360.0))
    pos = (eye + view * (focal + F32(0.01))).astype(F32)
    return dict(Position=pos, LookAt=(pos + view).astype(F32), Right=right, Up=up, LensHeight=F32(2.0), FocalDistance=focal)
