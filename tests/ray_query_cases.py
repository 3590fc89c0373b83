"""Ray sets and expected answers for tests/test_ray_queries.py: seeded, built from a scene view with the CPU oracle alone.

A case is a fixture scene (or, for the any-hit walk's refilling form, which runs from RQ_REFILL_TRIANGLES = 32 768 triangles, the procedural scene
of 40 000), option "alpha_test" and whether instances stay two-level.  Its ray set, about 4 700 rays:
  - the camera rays of a 64 x 48 frame;
  - 512 uniformly random rays from points inside the scene's bounds;
  - from every 8th camera hit one ray to a random point on a light triangle (the top face of the bounds where the scene has none), with
    TMax = 0.999 x the distance;
  - for 96 of the rays that hit, at t, copies with TMax in {0.5 t, 2 t, +inf, 1e6, 0.001, 0, NaN};
  - the degenerate rays ray_cannot_hit is about: a zero direction, a NaN component, axis-parallel directions;
  - a tenth of all rays disabled.
The expected answers restate include/tracerboy_hip.h: a ray is traced iff it is not disabled and TMax > MIN_T (a NaN is not); a hit counts iff
t < TMax (closest mode) / t < min(TMax, MAX_T) (occluded mode)."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol
from conftest import GOLDEN
from tracerboy_amd import api

MIN_T, MAX_T = np.float32(0.001), np.float32(999999.0)
SCENES = os.path.join(GOLDEN, "scenes")
# name -> (scene file -- None: tb_load_procedural(0, PROC_TRIANGLES, PROC_SEED) --, option alpha_test, option flatten_instances)
PROC_TRIANGLES, PROC_SEED = 40000, 1234
CASES = {
    "cornell": (os.path.join(SCENES, "cornell-box", "scene.pbrt"), 0, 1),
    "alpha0": (os.path.join(SCENES, "alpha-card", "scene.pbrt"), 0, 1),
    "alpha1": (os.path.join(SCENES, "alpha-card", "scene.pbrt"), 1, 1),
    "instanced": (os.path.join(SCENES, "alpha-card", "instanced.pbrt"), 0, 0),
    "proc40k": (None, 0, 1),
}
TMAX_FACTORS = 7  # copies per chosen ray


def _unit(v):
    v = np.asarray(v, np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def camera_rays(pf, lens_height, width, height):
    o = np.zeros((width * height, 3), np.float32); d = np.zeros((width * height, 3), np.float32)
    oo = (C.c_float * 3)(); dd = (C.c_float * 3)()
    k = 0
    for y in range(height):
        for x in range(width):
            ol.lib().tbo_camera_ray(C.byref(pf), lens_height, width, height, x + 0.5, y + 0.5, 0.3, 0.7, C.byref(oo), C.byref(dd))
            o[k] = oo[:]; d[k] = dd[:]; k += 1
    return o, d


def light_points(view, lo, hi, rng, n):
    """n random points on the scene's light triangles; on the top face of the bounds where it has none."""
    tris = []
    for i in range(view.numLights):
        l = view.lights[i]
        p = np.array([[l.P0.x, l.P0.y, l.P0.z], [l.P1.x, l.P1.y, l.P1.z], [l.P2.x, l.P2.y, l.P2.z]], np.float32)
        if l.SurfaceArea > 0 and np.isfinite(p).all() and np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0])) > 0:
            tris.append(p)
    if not tris:
        pts = rng.uniform(lo, hi, (n, 3)).astype(np.float32); pts[:, 1] = hi[1]
        return pts
    tris = np.stack(tris)[rng.integers(0, len(tris), n)]
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = u + v > 1; u = np.where(flip, 1 - u, u); v = np.where(flip, 1 - v, v)
    return (tris[:, 0] + u[:, None] * (tris[:, 1] - tris[:, 0]) + v[:, None] * (tris[:, 2] - tris[:, 0])).astype(np.float32)


def build_rays(view, pf, lens_height, scene_min, scene_max, seed=20):
    """The case's rays (api.QUERY_RAY_DTYPE) and the oracle's closest hits of their (origin, direction) pairs (ol.trace_closest's dict)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(scene_min), np.float32(scene_max)
    co, cd = camera_rays(pf, lens_height, 64, 48)
    ro = rng.uniform(lo, hi, (512, 3)).astype(np.float32); rd = _unit(rng.normal(size=(512, 3)))
    cam = ol.trace_closest(view, co, cd)
    hit = np.flatnonzero(cam["t"] > 0)[::8]
    p = (co[hit] + cd[hit] * cam["t"][hit, None]).astype(np.float32)
    to = light_points(view, lo, hi, rng, len(hit)) - p
    dist = np.linalg.norm(to, axis=1).astype(np.float32)
    keep = dist > 0
    p, to, dist = p[keep], to[keep], dist[keep]
    so, sd, st = p, (to / dist[:, None]).astype(np.float32), (np.float32(0.999) * dist).astype(np.float32)
    o = np.concatenate([co, ro, so]); d = np.concatenate([cd, rd, sd])
    tmax = np.concatenate([np.full(len(co) + len(ro), np.inf, np.float32), st])
    base = ol.trace_closest(view, o, d)
    chosen = rng.permutation(np.flatnonzero(base["t"] > 0))[:96]
    t = base["t"][chosen]
    factors = [np.float32(0.5) * t, np.float32(2.0) * t, np.full_like(t, np.inf), np.full_like(t, 1e6), np.full_like(t, 0.001), np.zeros_like(t),
               np.full_like(t, np.nan)]
    assert len(factors) == TMAX_FACTORS
    o = np.concatenate([o] + [o[chosen]] * TMAX_FACTORS); d = np.concatenate([d] + [d[chosen]] * TMAX_FACTORS)
    tmax = np.concatenate([tmax] + factors)
    # degenerate rays: zero directions, a NaN in one component of the origin or the direction, axis-parallel directions
    go = rng.uniform(lo, hi, (64, 3)).astype(np.float32); gd = _unit(rng.normal(size=(64, 3)))
    gd[:8] = 0.0
    for k in range(8, 24):
        (go if k & 1 else gd)[k, k % 3] = np.nan
    gd[24:] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 40)] * rng.choice(np.float32([-1, 1]), 40)[:, None]
    o = np.concatenate([o, go]); d = np.concatenate([d, gd]); tmax = np.concatenate([tmax, np.full(64, np.inf, np.float32)])
    rays = api.make_query_rays(o, d, tmax, disabled=rng.random(len(o)) < 0.1)
    return rays, ol.trace_closest(view, o, d)


def traced(rays):
    with np.errstate(invalid="ignore"):
        return ((rays["Flags"] & 1) == 0) & (rays["TMax"] > MIN_T)


def expected_hits(rays, oracle):
    """The records closest mode has to give, bit for bit: the oracle's hit where the ray is traced and t < TMax, the miss record elsewhere."""
    with np.errstate(invalid="ignore"):
        keep = traced(rays) & (oracle["t"] >= 0) & (oracle["t"] < rays["TMax"])
    e = np.zeros(len(rays), api.QUERY_HIT_DTYPE)
    e["T"] = -1.0; e["Prim"] = 0xffffffff; e["Geom"] = 0xffffffff; e["Material"] = -1
    e["T"][keep] = oracle["t"][keep]; e["U"][keep] = oracle["bary"][keep, 0]; e["V"][keep] = oracle["bary"][keep, 1]
    e["Prim"][keep] = oracle["prim"][keep]; e["Geom"][keep] = oracle["geom"][keep]; e["Material"][keep] = oracle["material"][keep]
    e["UV"][keep] = oracle["uv"][keep]; e["Normal"][keep] = oracle["normal"][keep]
    return e


def expected_occluded(rays, oracle):
    with np.errstate(invalid="ignore"):
        return (traced(rays) & (oracle["t"] >= 0) & (oracle["t"] < np.minimum(rays["TMax"], MAX_T))).astype(np.uint8)


def near_tmax(rays, oracle):
    """Rays whose TMax lies within rounding of the oracle's hit distance: the any-hit walk culls boxes against TMax, the closest walk against a
    shrinking closest distance, and only there can the two differ.  Left out of the occluded comparison; by construction there are none."""
    with np.errstate(invalid="ignore"):
        return traced(rays) & (oracle["t"] >= 0) & (np.abs(oracle["t"] - rays["TMax"]) <= np.float32(1e-4) * oracle["t"])


def scheduling_rays(scene_min, scene_max, n=1 << 17, seed=21):
    """n rays whose walks end many steps apart: half from inside the bounds with the renderer's range (most end at an early leaf), a quarter of
    the same kind with a short TMax (most find nothing, soon), a quarter aimed from far outside at a box three times the bounds (many cross the
    scene's box and miss everything)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(scene_min), np.float32(scene_max)
    centre, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    q = n // 4
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32); d = _unit(rng.normal(size=(n, 3)))
    tmax = np.full(n, np.inf, np.float32)
    tmax[2 * q:3 * q] = np.float32(0.02 * diag)
    o[3 * q:] = centre + 2 * diag * _unit(rng.normal(size=(n - 3 * q, 3)))
    d[3 * q:] = _unit(rng.uniform(centre - 1.5 * (hi - lo), centre + 1.5 * (hi - lo), (n - 3 * q, 3)) - o[3 * q:])
    order = rng.permutation(n)  # the kinds interleaved: every wave holds some of each
    return api.make_query_rays(o[order], d[order], tmax[order])


def host_case(name, settings):
    """The case built without a device: (rays, oracle) from a host scene.  Sets the oracle's alpha test; the caller resets it."""
    path, alpha, flatten = CASES[name]
    hs = api.HostScene(path, flatten_instances=bool(flatten)) if path else api.HostScene(procedural=(0, PROC_TRIANGLES, PROC_SEED))
    ol.set_alpha_test(alpha)
    info = hs.info()
    return build_rays(hs.view(), hs.frame_constants(settings), hs.camera().LensHeight, info.sceneMin[:], info.sceneMax[:])
