"""Inputs and expected values for tests/test_radiance_queries.py: seeded, built with numpy and the CPU oracle alone.

The contract's seed is hash13(SeedX, SeedY, s) moved by seed_advance in steps of 1, each a rounded fp32 addition, because that is how the renderer
gets there (path_begin's two GetBlueNoise calls without blue noise are sixteen rand() steps; hemisphere mode adds two more) and a chain of
rounded additions is not the one addition: start_seed restates the contract, one_addition_differs counts the pixels of the camera cases where
hash13 + 16 in one addition would have been another number."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol
from conftest import GOLDEN
from tracerboy_amd import api

F32 = np.float32
SCENES = {name: os.path.join(GOLDEN, "scenes", name, "scene.pbrt") for name in ("cornell-box", "mix-glass", "Teapot", "instances")}
PROC_TRIANGLES, PROC_SEED = 40000, 1234                               # tests/ray_query_cases.py's procedural scene
W, H, FRAMES = 32, 24, 4
WINDOW = (7, 5, 12, 8)                                                # 5 x 3 pixels
CHUNK = 64                                                            # RAD_CHUNK (kernels/rad_launch.h)
SIZES = (1, 63, 64, 65, 257, 8 * CHUNK + 1)


def hash13(x, y, z):
    """The oracle's hash13 on arrays of equal length, fp32."""
    L = ol.lib()
    x, y, z = np.broadcast_arrays(np.asarray(x, F32), np.asarray(y, F32), np.asarray(z, F32))
    return np.array([L.tbo_hash13(float(a), float(b), float(c)) for a, b, c in zip(x.ravel(), y.ravel(), z.ravel())], F32).reshape(x.shape)


def stepped(seed, steps):
    """seed + 1 + 1 + ... (steps times) in fp32: how rand() moves it."""
    s = np.asarray(seed, F32).copy()
    for _ in range(int(steps)):
        s = (s + F32(1.0)).astype(F32)
    return s


def start_seed(seed_x, seed_y, sample, advance):
    """The contract's seed of a sample (include/tracerboy_hip.h): hash13 moved by floor(advance) steps of 1 (at most 1024), then by the rest."""
    h = hash13(seed_x, seed_y, F32(sample))
    steps = min(int(np.floor(advance)), 1024) if advance >= 1 else 0
    return (stepped(h, steps) + (F32(advance) - F32(steps))).astype(F32)


def one_addition_differs(seed_x, seed_y, sample, advance):
    """Boolean per ray: hash13 + advance in ONE addition is another number than the stepped seed -- why the contract steps."""
    return (hash13(seed_x, seed_y, F32(sample)) + F32(advance)).astype(F32) != start_seed(seed_x, seed_y, sample, advance)


def unit(v):
    v = np.asarray(v, F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def random_rays(lo, hi, n, seed):
    """n rays from points inside the bounds in uniformly random unit directions, default seeds (i % 4096, i // 4096)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(np.float32(lo), np.float32(hi), (n, 3)).astype(F32)
    return api.make_radiance_rays(o, unit(rng.normal(size=(n, 3))))


def surface_points(view, lo, hi, n, seed):
    """n points on the scene's surfaces with the unit normals that face where the finding ray came from: the oracle's closest hits of random rays,
    offset by nothing (MIN_T keeps a path off the surface it starts on)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(np.float32(lo), np.float32(hi), (8 * n, 3)).astype(F32); d = unit(rng.normal(size=(8 * n, 3)))
    hit = ol.trace_closest(view, o, d)
    nrm = hit["normal"]
    ok = np.flatnonzero((hit["t"] > 0) & (np.abs(np.linalg.norm(nrm, axis=1) - 1) < 1e-3))[:n]
    assert len(ok) == n
    p = (o[ok] + d[ok] * hit["t"][ok, None]).astype(F32)
    facing = np.where((nrm[ok] * d[ok]).sum(1, keepdims=True) > 0, -nrm[ok], nrm[ok]).astype(F32)
    return p, unit(facing)


def cosine_directions(seeds, time, normals):
    """tbo_sample_directions(2, seed, time, NULL, normal, 0, 1, ...) per ray: GenerateCosineWeightedDirection of the two numbers drawn at seed."""
    L = ol.lib()
    fp = C.POINTER(C.c_float)
    L.tbo_sample_directions.restype = None
    L.tbo_sample_directions.argtypes = [C.c_int, C.c_float, C.c_float, fp, fp, C.c_float, C.c_uint32, fp, fp]
    out = np.empty((len(seeds), 3), F32)
    normals = np.ascontiguousarray(normals, F32)
    for i, s in enumerate(np.asarray(seeds, F32)):
        L.tbo_sample_directions(2, float(s), float(time), None, normals[i].ctypes.data_as(fp), 0.0, 1, out[i].ctypes.data_as(fp), None)
    return out


def light_of(view):
    """The first area light's centroid and the emissive colour of its material cannot be read off TbLight alone: centroid only."""
    l = view.lights[0]
    p = np.array([[l.P0.x, l.P0.y, l.P0.z], [l.P1.x, l.P1.y, l.P1.z], [l.P2.x, l.P2.y, l.P2.z]], F32)
    return p.mean(axis=0).astype(F32)


def sequential_sum(value, count):
    """0 + v + v + ... in fp32, count times, per channel."""
    acc = np.zeros_like(np.asarray(value, F32))
    for _ in range(count):
        acc = (acc + np.asarray(value, F32)).astype(F32)
    return acc
