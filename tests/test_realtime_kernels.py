"""The three kernels of rt_kernels.hip (temporal accumulation, one a-trous pass, albedo composite) on synthetic surfaces and edge values.

CPU part: the oracle's fp32 restatement (oracle/rt_ref.cpp) against the float64 restatement of tests/realtime_ref.py, which was written from
the shaders and shares no arithmetic with it -- an error the oracle and the kernel had in common would show here.  The cases of the GPU part
are built and their branch pre-checks asserted on the CPU too.
GPU part: the kernels through tb_run_temporal / tb_run_denoise_pass / tb_run_composite against the oracle, bit for bit (or NaN on both
sides), on every size that is ragged against the 8 x 8 tile and on inputs no render produces.  Every case asserts on the oracle's output
first that the branch it is meant to reach is reached."""
import copy
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import oracle_lib as ol
import realtime_ref as rr
from tracerboy_amd import _ctypes_abi as abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORNELL = os.path.join(GOLDEN, "scenes", "cornell-box", "scene.pbrt")
F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)

# Tolerances of the CPU part: 4 x the largest error of the oracle against the float64 restatement measured on exactly these inputs.
TEMPORAL_ABS_MEASURED = 9.47e-6    # 100 x 70, second move, moments on; 7.6e-7 at 9 x 17, 2.3e-6 at 37 x 23; left out: 0, 0 and 1 of 7000 pixels
FILTER_REL_MEASURED = 3.01e-6      # OffsetMultiplier 1, exponent 128; 7.5e-8 at 64 where only the centre tap is left
COMPOSITE_REL_MEASURED = 1.31e-7
TEMPORAL_ABS_TOL, FILTER_REL_TOL, COMPOSITE_REL_TOL = 4 * TEMPORAL_ABS_MEASURED, 4 * FILTER_REL_MEASURED, 4 * COMPOSITE_REL_MEASURED
DECISION_DISTANCE = 1e-4      # a pixel closer than this to a discontinuity of the temporal operation is not compared with float64
MAX_EXCLUDED_SHARE = 0.02

MOVES = [(0.15, 0.0705, 0.0), (0.6, 0.282, 0.0)]
CPU_TEMPORAL_SIZES = [(9, 17), (37, 23), (100, 70)]
CPU_FILTER_MULTS = [1, 2, 4, 16, 64]
SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (37, 23), (64, 1), (1, 64)]   # width x height; the tile is 8 x 8


# ---- surfaces ---------------------------------------------------------------------------------------------------------------------------
def camera(position=(0, 0, 5), look_at=(0, 0, 0), right=(1, 0, 0), up=(0, 1, 0)):
    """simple_camera() of test_realtime_chain.py by default"""
    c = abi.tb_camera()
    c.Position[:] = position; c.LookAt[:] = look_at; c.Right[:] = right; c.Up[:] = up
    c.LensHeight = 2.0; c.FocalDistance = 3.0
    return c


def moved(cam, shift):
    return camera([p + s for p, s in zip(cam.Position[:], shift)], [p + s for p, s in zip(cam.LookAt[:], shift)], cam.Right[:], cam.Up[:])


def constants(w, h, cam, prev, moments, history_weight=0.95, ignore=0):
    k = abi.TbTemporalConstants()
    k.ResolutionX, k.ResolutionY = w, h
    k.CameraFocalDistance, k.CameraLensHeight = cam.FocalDistance, cam.LensHeight
    k.IgnoreHistory, k.HistoryWeight, k.OutputMomentInformation = ignore, history_weight, 1 if moments else 0
    for name in ("Position", "LookAt", "Up", "Right"):
        setattr(k, "Camera" + name, getattr(cam, name)); setattr(k, "PrevFrameCamera" + name, getattr(prev, name))
    return k


def focal_point(cam):
    pos, look = np.array(cam.Position[:], np.float64), np.array(cam.LookAt[:], np.float64)
    d = (look - pos) / np.linalg.norm(look - pos)
    return pos - cam.FocalDistance * d


def plane_positions(w, h, cam, slope=0.3):
    """world positions (xyz, pixel footprint 0.01) of the plane z = slope * x seen through cam: the pinhole is the focal point, the lens plane
    goes through Position -- plane_world_positions of test_realtime_chain.py for any camera and a tilted plane"""
    pos, focal = np.array(cam.Position[:], np.float64), focal_point(cam)
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs + 0.5) / w * 2 - 1; v = 1 - (ys + 0.5) / h * 2
    lens = pos + u[..., None] * np.array(cam.Right[:]) * (cam.LensHeight * w / h / 2) + v[..., None] * np.array(cam.Up[:]) * (cam.LensHeight / 2)
    d = lens - focal
    t = (slope * focal[0] - focal[2]) / (d[..., 2] - slope * d[..., 0])
    wp = np.zeros((h, w, 4), F32); wp[..., :3] = focal + d * t[..., None]; wp[..., 3] = 0.01
    return wp


def plane_normals(w, h, slope=0.3):
    n = np.zeros((h, w, 4), F32); n[..., :3] = np.array([-slope, 0, 1]) / np.hypot(slope, 1)
    return n


def temporal_surfaces(w, h, prev_cam, cam, seed):
    """dict of the input surfaces: the tilted plane through both cameras, its unit normal, random colours and moment history in [0, 1)"""
    rng = np.random.default_rng(seed)
    s = {"history": rng.random((h, w, 4)).astype(F32), "current": rng.random((h, w, 4)).astype(F32), "world_pos": plane_positions(w, h, cam),
         "prev_world_pos": plane_positions(w, h, prev_cam), "moment_history": rng.random((h, w, 4)).astype(F32), "normals": plane_normals(w, h)}
    return s


ORDER = ("history", "current", "world_pos", "prev_world_pos", "moment_history", "normals")


def oracle_temporal(k, s):
    return ol.temporal(k, *[s[n] if n != "moment_history" or k.OutputMomentInformation else None for n in ORDER])


def accepted_by_oracle(k, s):
    """per pixel: the oracle blends history in (history 2, current 0, weight 1: the output is 2 where a tap was accepted, else 0)"""
    k2 = copy.copy(k); k2.HistoryWeight = 1.0; k2.OutputMomentInformation = 0
    s2 = dict(s, history=np.full_like(s["history"], 2), current=np.zeros_like(s["current"]))
    return oracle_temporal(k2, s2)[0][..., 0] != 0


def filter_surfaces(w, h, seed):
    """input (rgb in [0, 4), variance in [0, 0.5]), unit normals within 15 degrees of +z, the tilted plane with footprints in [0.005, 0.05],
    undenoised colours in [0, 4)"""
    rng = np.random.default_rng(seed)
    inp = (rng.random((h, w, 4)) * [4, 4, 4, 0.5]).astype(F32)
    theta, phi = rng.random((h, w)) * np.radians(15), rng.random((h, w)) * 2 * np.pi
    normals = np.zeros((h, w, 4), F32)
    normals[..., 0] = np.sin(theta) * np.cos(phi); normals[..., 1] = np.sin(theta) * np.sin(phi); normals[..., 2] = np.cos(theta)
    pos = plane_positions(w, h, camera()); pos[..., 3] = 0.005 + 0.045 * rng.random((h, w))
    und = (rng.random((h, w, 4)) * 4).astype(F32)
    return {"input": inp, "normals": normals, "positions": pos, "undenoised": und}


def filter_constants(w, h, mult, exponent=128.0, pos_mult=1.0, luma_mult=4.0):
    return abi.TbDenoiserConstants(w, h, mult, exponent, pos_mult, luma_mult, 1)


def oracle_filter(k, s):
    return ol.denoise(k, s["input"], s["normals"], s["positions"], s["undenoised"])


# ---- CPU: oracle against float64 ----------------------------------------------------------------------------------------------------------
def temporal_errors(w, h, shift, moments):
    """(largest absolute error over the compared pixels, pixels left out, pixels)"""
    prev = camera(); cam = moved(prev, shift)
    s = temporal_surfaces(w, h, prev, cam, seed=w * 1000 + h)
    k = constants(w, h, cam, prev, moments)
    out, mom = oracle_temporal(k, s)
    want, want_mom, info = rr.temporal(k, *[s[n] for n in ORDER])
    keep = info["decision"] >= DECISION_DISTANCE
    err = np.abs(out - want)[keep].max()
    if moments:   # m1, m2 in [0, 1), the sample count in [1, 2)
        err = max(err, np.abs(mom - want_mom)[keep].max())
    assert info["valid"].any()
    return float(err), int((~keep).sum()), w * h


@pytest.mark.parametrize("moments", [True, False])
@pytest.mark.parametrize("shift", MOVES)
@pytest.mark.parametrize("w,h", CPU_TEMPORAL_SIZES)
def test_temporal_oracle_against_float64(built, w, h, shift, moments):
    """measured (oracle vs float64, largest over the twelve cases): see TEMPORAL_ABS_MEASURED; excluded pixels: see the module's end"""
    err, excluded, n = temporal_errors(w, h, shift, moments)
    print("temporal %dx%d shift %s moments %d: abs err %.3g, %d of %d pixels left out" % (w, h, shift, moments, err, excluded, n))
    assert excluded <= MAX_EXCLUDED_SHARE * n
    assert err <= TEMPORAL_ABS_TOL


def test_temporal_static_camera_on_the_tilted_plane(built):
    """Static camera: every pixel reprojects onto itself.  Row 0 and column 0 land on fx or fy = 0 up to rounding, where int() and frac()
    disagree about the side (the reference's behaviour: the taps flip on the last bit) -- away from them history is accepted and
    out = lerp(cur, hist, 0.95), whichever side of the integer fx fell on: the tap on the other side has a weight of rounding size."""
    w, h = 37, 23
    cam = camera()
    s = temporal_surfaces(w, h, cam, cam, seed=5)
    k = constants(w, h, cam, cam, moments=True)
    out, mom = oracle_temporal(k, s)
    assert accepted_by_oracle(k, s)[1:, 1:].all()
    cur, hist = s["current"].astype(np.float64), s["history"].astype(np.float64)
    np.testing.assert_allclose(out[1:, 1:, :3], (cur + 0.95 * (hist - cur))[1:, 1:, :3], rtol=2e-4, atol=2e-5)
    # the moments of the same pixels: bilinear sample at the pixel's own centre = its own history
    mh = s["moment_history"].astype(np.float64)[1:, 1:]
    lum = rr.luma(cur)[1:, 1:]; f = 1 / np.minimum(mh[..., 2] + 1, 32)
    np.testing.assert_allclose(mom[1:, 1:, 0], mh[..., 0] + f * (lum - mh[..., 0]), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(mom[1:, 1:, 2], mh[..., 2] + 1, rtol=2e-4)
    # the float64 restatement marks exactly row 0 and column 0 as sitting on a decision there (and possibly more, never fewer)
    info = rr.temporal(k, *[s[n] for n in ORDER])[2]
    assert (info["decision"][0, :] < DECISION_DISTANCE).all() and (info["decision"][:, 0] < DECISION_DISTANCE).all()


def filter_error(mult, exponent):
    w, h = 37, 23
    s = filter_surfaces(w, h, seed=11)
    k = filter_constants(w, h, mult, exponent)
    out = oracle_filter(k, s).astype(np.float64)
    want = rr.denoise(k, s["input"], s["normals"], s["positions"], s["undenoised"])
    if mult >= 64:   # only the centre tap is inside the frame
        np.testing.assert_allclose(out, s["input"], rtol=1e-5)
    return float((np.abs(out - want) / np.abs(want)).max())


@pytest.mark.parametrize("exponent", [128.0, 1.0])
@pytest.mark.parametrize("mult", CPU_FILTER_MULTS)
def test_filter_oracle_against_float64(built, mult, exponent):
    """no pixel is left out: the filter is continuous in these inputs"""
    err = filter_error(mult, exponent)
    print("filter mult %d exponent %g: rel err %.3g" % (mult, exponent, err))
    assert err <= FILTER_REL_TOL


def composite_error():
    rng = np.random.default_rng(3)
    a, l, e = (rng.random((23, 37, 4)).astype(F32) for _ in range(3))
    l *= 4; a[0, :7, 3] = [0, 1, 0, 1, 0.5, 0, 1]
    out = ol.composite(a, l, e).astype(np.float64)
    want = rr.composite(a, l, e)
    return float((np.abs(out - want) / np.abs(want)).max())


def test_composite_oracle_against_float64(built):
    err = composite_error()
    print("composite: rel err %.3g" % err)
    assert err <= COMPOSITE_REL_TOL


# ---- the cases of the GPU part: inputs, the oracle's output and the branch pre-check, all on the CPU -----------------------------------------
def centre(w, h):
    return h // 2, w // 2


def cycle(values, n, start=0):
    return np.array([values[(i + start) % len(values)] for i in range(n)], F32)


def camera_cases():
    """(name, previous camera, current camera)"""
    base = camera()
    a = np.radians(30)
    yaw = camera(look_at=(-5 * np.sin(a), 0, 5 - 5 * np.cos(a)), right=(np.cos(a), 0, -np.sin(a)))
    roll = camera(right=(np.cos(a), np.sin(a), 0), up=(-np.sin(a), np.cos(a), 0))
    behind = camera(position=(0, 0, -5), look_at=(0, 0, -10))
    return [("moved-1", base, moved(base, MOVES[0])), ("moved-2", base, moved(base, MOVES[1])), ("yaw-30", yaw, base), ("roll-30", roll, base),
            ("behind", behind, base)]


@functools.lru_cache(maxsize=None)
def temporal_cases(w, h):
    """list of (label, constants, surfaces, (oracle out, oracle moments)); asserts every case's pre-check"""
    cases = []
    can_accept = min(w, h) > 1   # a frame one pixel wide or high has no valid neighbour: extent 0, nothing is ever accepted

    def add(label, k, s, check=None):
        want = oracle_temporal(k, s)
        if check is not None:
            check(want)
        cases.append((label, k, s, want))

    def rejected_at(s, where):
        return lambda want: np.testing.assert_array_equal(bits(want[0][where][..., :3]), bits(s["current"][where][..., :3]))

    # cameras x constants
    for name, prev, cam in camera_cases():
        s = temporal_surfaces(w, h, prev, cam, seed=17)
        k0 = constants(w, h, cam, prev, moments=True)
        accepted = accepted_by_oracle(k0, s)
        info = rr.temporal(k0, *[s[n] for n in ORDER])[2]
        if name.startswith("moved"):
            assert accepted.any() == can_accept, name
        elif name == "yaw-30":
            # the picture moves sideways by about 3 tan 30 = 1.7 lens half-heights: out of every frame but the widest, which the roll covers
            assert (w > 2 * h or not info["inside"].all()) and not accepted[~info["inside"]].any(), name
        elif name == "roll-30":
            assert not info["inside"].all() or (w, h) == (1, 1), name
            assert accepted.any() == can_accept and not accepted.all(), name
        else:
            # (the widest frame sees the plane climb past the previous camera's focal point at its ends)
            assert info["behind"].any() and (w > 2 * h or info["behind"].all()) and not accepted[info["behind"]].any(), name
        for ignore, moments, hw in itertools.product((0, 1), (True, False), (0.0, 0.95, 1.0)):
            k = constants(w, h, cam, prev, moments, hw, ignore)
            check = None
            if ignore:   # the current frame passes through, whatever the history
                check = lambda want, s=s, moments=moments: (np.testing.assert_array_equal(bits(want[0][..., :3]), bits(s["current"][..., :3])),
                                                            moments or np.testing.assert_array_equal(want[0][..., 3], 1))
            elif hw == 0.95 and name == "moved-1" and can_accept:
                check = lambda want, s=s: np.any(want[0][..., :3] != s["current"][..., :3]) or pytest.fail("no history blended in")
            add("%s ignore=%d moments=%d weight=%g" % (name, ignore, moments, hw), k, s, check)

    # planted pixels on the first moved camera
    name, prev, cam = camera_cases()[0]
    base = temporal_surfaces(w, h, prev, cam, seed=23)
    k = constants(w, h, cam, prev, moments=True)
    c = centre(w, h)
    focal = focal_point(prev).astype(F32)

    def planted(label, surface, value, check):
        s = dict(base); s[surface] = base[surface].copy(); s[surface][c][:3] = value
        add("planted " + label, k, s, check(s))

    rejected = lambda s: rejected_at(s, c)
    planted("denom == 0", "world_pos", focal + np.array(prev.Right[:], F32), rejected)       # the ray runs along the lens plane
    planted("NaN direction", "world_pos", focal, rejected)                                     # normalize(0)
    planted("NaN position", "world_pos", [NAN, NAN, NAN], rejected)
    planted("+inf position", "world_pos", [INF, 0, 0], rejected)
    planted("-inf position", "world_pos", [0, 0, -INF], rejected)
    planted("NaN previous position", "prev_world_pos", [NAN, 0, 0], lambda s: None)
    planted("inf previous position", "prev_world_pos", [INF, -INF, 0], lambda s: None)
    planted("miss (-0, 0, -0)", "normals", [-0.0, 0.0, -0.0], rejected)
    blended = lambda s: (lambda want: can_accept and (np.any(want[0][c][:3] != s["current"][c][:3]) or pytest.fail("NaN normal: no history")))
    planted("NaN normal is a hit", "normals", [NAN, 0, 0], blended)

    # disocclusion: previous positions pushed out of reach on a random half of the pixels: 0 to 4 of the four taps survive
    s = dict(base); s["prev_world_pos"] = base["prev_world_pos"].copy()
    mask = np.random.default_rng(29).random((h, w)) < 0.5
    s["prev_world_pos"][mask, 2] += 50
    taps = rr.temporal(k, *[s[n] for n in ORDER])[2]["taps"]
    if can_accept and w * h >= 35:
        assert {0, 4} <= set(taps.ravel()) and set(taps.ravel()) & {1, 2, 3}, sorted(set(taps.ravel()))   # partial sets: SummedWeight renormalises
    acc = accepted_by_oracle(k, s)
    assert acc.any() == can_accept and not acc.all()
    add("disocclusion", k, s)

    # a constant world-position field: extent 0, the strict < rejects every tap
    s = dict(base); s["world_pos"] = np.full((h, w, 4), F32(1.5)); s["prev_world_pos"] = s["world_pos"].copy()
    add("constant positions", k, s, rejected_at(s, np.s_[:, :]))

    # moment history: counts around the cap of 32 and beyond, m2 < m1^2; colours whose luminance or its square leave fp32
    s = dict(base); mh = base["moment_history"].copy().reshape(-1, 4); cur = base["current"].copy().reshape(-1, 4)
    mh[:, 2] = cycle([-1, 0, 30, 31, 32, 1000, INF, NAN], w * h)
    mh[::3, 0] = 0.9; mh[::3, 1] = 0.1
    cur[:, 0] = cycle([0.5, NAN, INF, -INF, 3e38, 1e-41, 0.25], w * h, start=3)
    s["moment_history"] = mh.reshape(h, w, 4); s["current"] = cur.reshape(h, w, 4)

    def edge_moments(want):
        out, mom = want
        assert not np.isfinite(mom).all() and (w * h < 8 or (np.isnan(mom).any() and np.isinf(mom).any() and np.isnan(out).any()))
        assert w * h < 8 or (out[..., 3] == 0).any()   # max(m2 - m1^2, 0) clamps
    add("edge moments", k, s, edge_moments)
    return cases


FILTER_MULTS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]


@functools.lru_cache(maxsize=None)
def filter_cases(w, h):
    cases = []
    base = filter_surfaces(w, h, seed=31)
    c = centre(w, h)

    def add(label, k, s, check=None):
        want = oracle_filter(k, s)
        if check is not None:
            check(want)
        cases.append((label, k, s, want))

    passes_through = lambda s: (lambda want: np.testing.assert_allclose(want, s["input"], rtol=1e-5))
    for mult, exponent, (pos_mult, luma_mult) in itertools.product(FILTER_MULTS, (0.0, 1.0, 128.0), ((1.0, 4.0), (0.0, 4.0), (1.0, 0.0), (0.0, 0.0))):
        check = None
        if exponent != 0.0 and (mult >= max(w, h) or pos_mult == 0.0):
            check = passes_through(base)     # only the centre tap is in the frame / has a position weight
        elif exponent == 128.0 and mult == 1 and min(w, h) > 1:
            check = lambda want: np.any(want != base["input"]) or pytest.fail("nothing filtered")
        add("mult=%d exponent=%g position=%g luma=%g" % (mult, exponent, pos_mult, luma_mult), filter_constants(w, h, mult, exponent, pos_mult, luma_mult), base, check)

    def variant(label, edit, check):
        s = {n: a.copy() for n, a in base.items()}
        edit(s)
        for mult in (1, 2):
            add("%s mult=%d" % (label, mult), filter_constants(w, h, mult), s, check(s))

    def put(surface, where, value):
        def edit(s):
            s[surface][where] = value
        return edit

    finite_rgb = lambda s: (lambda want: np.isfinite(want[c][:3]).all() or pytest.fail("colour not finite"))
    variant("centre variance 0", put("input", c + (3,), 0.0), finite_rgb)
    variant("centre variance negative", put("input", c + (3,), -0.25), finite_rgb)          # sqrt gives NaN, max(NaN, EPSILON) = EPSILON
    variant("centre variance NaN", put("input", c + (3,), NAN), lambda s: (lambda want: np.isfinite(want[c][:3]).all() and np.isnan(want[c][3]) or pytest.fail(str(want[c]))))
    variant("centre variance inf", put("input", c + (3,), INF), lambda s: (lambda want: np.isinf(want[c][3]) or pytest.fail(str(want[c]))))
    variant("centre variance denormal", put("input", c + (3,), 1e-41), finite_rgb)
    variant("zero normal at the centre", put("normals", c, 0.0), lambda s: (lambda want: np.testing.assert_array_equal(bits(want[c]), bits(s["input"][c]))))

    def zero_ring(s):
        y, x = c
        s["normals"][max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0; s["normals"][c] = base["normals"][c]
    variant("zero normals among the taps", zero_ring, finite_rgb)

    def antiparallel(s):
        s["normals"][:, w // 2:, :3] *= -1
    variant("antiparallel half-frame", antiparallel, lambda s: (lambda want: np.isfinite(want).all() or pytest.fail("not finite")))

    def scaled(f):
        def edit(s):
            s["normals"][..., :3] *= F32(f)
        return edit
    all_nan = lambda s: (lambda want: np.isnan(want).all() or pytest.fail("expected 0/0 or inf/inf everywhere"))
    variant("normals of length 0.4", scaled(0.4), all_nan)     # 0.16^128 underflows: every weight 0, the centre's too
    variant("normals of length 3e3", scaled(3e3), all_nan)     # 9e6^128 overflows
    variant("footprint 0", put("positions", np.s_[..., 3], 0.0), passes_through)

    def negated_footprint(s):
        s["positions"][..., 3] *= -1
    for mult in (1, 2):   # |ox * d + oy * d| is even in d
        want_base = oracle_filter(filter_constants(w, h, mult), base)
        variant_check = lambda s, wb=want_base: (lambda want: np.testing.assert_array_equal(bits(want), bits(wb)))
        s = {n: a.copy() for n, a in base.items()}; negated_footprint(s)
        add("negative footprint mult=%d" % mult, filter_constants(w, h, mult), s, variant_check(s))

    def bad_positions(s):
        s["positions"][c][:3] = [NAN, 0, 0]
        s["positions"][(c[0] + 1) % h, (c[1] + 1) % w][:3] = [INF, 0, -INF]
    variant("NaN and inf positions", bad_positions, lambda s: (lambda want: np.isnan(want[c]).any() or pytest.fail("NaN position had no effect")))

    def luminance_step(s):
        s["undenoised"][:, w // 2:, :3] *= F32(1e6); s["input"][..., 3] = 0
    variant("luminance step of 1e6 at variance 0", luminance_step, lambda s: (lambda want: np.isfinite(want).all() or pytest.fail("not finite")))
    return cases


@functools.lru_cache(maxsize=None)
def composite_cases(w, h):
    rng = np.random.default_rng(37)
    n = w * h
    a, l, e = (rng.random((n, 4)).astype(F32) for _ in range(3))
    a[:, 3] = cycle([-1, 0, 0.5, 1, 2, NAN, INF], n)
    l[:, 0] = cycle([1.0, NAN, INF, 1e-41, -INF], n, start=1); l[:, 1] = cycle([2.0, 1e-41, 0.0], n)
    e[:, 2] = cycle([0.5, INF, 1e-41, NAN, -1e-41, 0.0], n, start=2)
    a, l, e = (x.reshape(h, w, 4) for x in (a, l, e))
    want = ol.composite(a, l, e)
    assert (want[..., 3] == 1).all() and (n < 8 or (np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want[..., :3]).any()))
    return [("edge values", None, (a, l, e), want)]


@pytest.mark.parametrize("w,h", SIZES)
def test_cases_reach_their_branches_in_the_oracle(built, w, h):
    """builds every case of the GPU part (which asserts its pre-check on the oracle's output); the oracle survives every edge input"""
    assert len(temporal_cases(w, h)) >= 70 and len(filter_cases(w, h)) >= 140 and len(composite_cases(w, h)) == 1


# ---- GPU: kernel against oracle through the seam ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same(got, want, what):
    """equal bits, or NaN on both sides (x86 and gfx950 give the default NaN different signs)"""
    bad = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        at = tuple(np.argwhere(bad)[0][:2])
        pytest.fail("%s: %d values differ, first at (y, x) = %s: kernel %s, oracle %s" % (what, int(bad.sum()), at, got[at], want[at]))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_temporal_kernel_bit_exact(gpu_tb, w, h):
    for label, k, s, (want, want_mom) in temporal_cases(w, h):
        got, got_mom = gpu_tb.RunTemporal(k, *[s[n] if n != "moment_history" or k.OutputMomentInformation else None for n in ORDER])
        assert_same(got, want, "%dx%d %s" % (w, h, label))
        assert (got_mom is None) == (want_mom is None)
        if want_mom is not None:
            assert_same(got_mom, want_mom, "%dx%d %s, moments" % (w, h, label))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_filter_kernel_bit_exact(gpu_tb, w, h):
    for label, k, s, want in filter_cases(w, h):
        assert_same(gpu_tb.RunDenoisePass(k, s["input"], s["normals"], s["positions"], s["undenoised"]), want, "%dx%d %s" % (w, h, label))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_composite_kernel_bit_exact(gpu_tb, w, h):
    for label, _, (a, l, e), want in composite_cases(w, h):
        assert_same(gpu_tb.RunComposite(w, h, a, l, e), want, "%dx%d %s" % (w, h, label))


@pytest.mark.gpu
def test_gpu_hooks_leave_the_realtime_state_alone(built, settings):
    """two real-time frames, every hook on unrelated surfaces of another size, two more frames: stages 0-4 of frames 3 and 4 are those of
    an uninterrupted sequence on a fresh context"""
    from tracerboy_amd import api
    W, H = 40, 24
    s = copy.copy(settings); s.MaxBounces = 2
    dn = api.GetDefaultDenoiserSettings(); dn.WaveletIterations = 2

    def sequence(interrupt):
        with api.TracerBoy(0) as tb:
            tb.LoadScene(CORNELL)
            stages = []
            for frame in range(4):
                if frame == 2 and interrupt:
                    w, h = 9, 17
                    _, k, surf, want = temporal_cases(w, h)[0]
                    assert_same(tb.RunTemporal(k, *[surf[n] for n in ORDER])[0], want[0], "temporal hook")
                    _, k, surf, want = filter_cases(w, h)[0]
                    assert_same(tb.RunDenoisePass(k, surf["input"], surf["normals"], surf["positions"], surf["undenoised"]), want, "filter hook")
                    _, _, (a, l, e), want = composite_cases(w, h)[0]
                    assert_same(tb.RunComposite(w, h, a, l, e), want, "composite hook")
                tb.RenderRealTime(W, H, s, dn, 0.0)
                if frame >= 2:
                    stages.append([tb.ReadRealTimeStage(i) for i in range(5)])
            return stages

    plain, interrupted = sequence(False), sequence(True)
    for frame, (a, b) in enumerate(zip(plain, interrupted)):
        for stage in range(5):
            assert_same(b[stage], a[stage], "frame %d stage %d" % (frame + 3, stage))
    assert np.any(plain[1][4][..., :3] != plain[1][3][..., :3])   # history was blended in: the state that must survive exists


@pytest.mark.gpu
def test_gpu_hooks_refuse_bad_arguments(gpu_tb):
    from tracerboy_amd import api
    w, h = 7, 5
    _, k, s, _ = temporal_cases(w, h)[0]
    assert k.OutputMomentInformation
    surfaces = [s[n] for n in ORDER]
    L, ctx = gpu_tb._L, gpu_tb._ctx
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    out, mom = np.empty((h, w, 4), F32), np.empty((h, w, 4), F32)

    def refused(rc, word):
        assert rc == -1, rc   # TB_E_INVALID
        message = L.tb_last_error(ctx).decode()
        assert word in message, message

    def temporal(k, surfaces, out, mom):
        return L.tb_run_temporal(ctx, C.byref(k), *[ptr(a) for a in surfaces], ptr(out), ptr(mom))
    assert temporal(k, surfaces, out, mom) == 0
    for i, name in enumerate(ORDER):
        if name != "moment_history":
            refused(temporal(k, surfaces[:i] + [None] + surfaces[i + 1:], out, mom), "null")
    refused(temporal(k, surfaces, None, mom), "null")
    refused(temporal(k, surfaces[:4] + [None] + surfaces[5:], out, mom), "moment")
    refused(temporal(k, surfaces, out, None), "moment")
    k_off = copy.copy(k); k_off.OutputMomentInformation = 0
    assert temporal(k_off, surfaces[:4] + [None] + surfaces[5:], out, None) == 0     # not required without moments
    for field in ("ResolutionX", "ResolutionY"):
        k0 = copy.copy(k); setattr(k0, field, 0)
        refused(temporal(k0, surfaces, out, mom), "0")
    k_big = copy.copy(k); k_big.ResolutionX, k_big.ResolutionY = 4097, 4096
    refused(temporal(k_big, surfaces, out, mom), "2^24")

    _, kf, sf, _ = filter_cases(w, h)[0]
    fs = [sf[n] for n in ("input", "normals", "positions", "undenoised")]

    def run_filter(k, fs, out):
        return L.tb_run_denoise_pass(ctx, C.byref(k), *[ptr(a) for a in fs], ptr(out))
    assert run_filter(kf, fs, out) == 0
    for i in range(4):
        refused(run_filter(kf, fs[:i] + [None] + fs[i + 1:], out), "null")
    refused(run_filter(kf, fs, None), "null")
    k0 = copy.copy(kf); k0.OffsetMultiplier = 0
    refused(run_filter(k0, fs, out), "OffsetMultiplier")
    k0 = copy.copy(kf); k0.ResolutionY = 0
    refused(run_filter(k0, fs, out), "0")
    k_big = copy.copy(kf); k_big.ResolutionX, k_big.ResolutionY = 4096, 4097
    refused(run_filter(k_big, fs, out), "2^24")

    _, _, (a, l, e), _ = composite_cases(w, h)[0]
    assert L.tb_run_composite(ctx, w, h, ptr(a), ptr(l), ptr(e), ptr(out)) == 0
    for args in ((None, l, e, out), (a, None, e, out), (a, l, None, out), (a, l, e, None)):
        refused(L.tb_run_composite(ctx, w, h, *[ptr(x) for x in args]), "null")
    refused(L.tb_run_composite(ctx, 0, h, ptr(a), ptr(l), ptr(e), ptr(out)), "0")
    refused(L.tb_run_composite(ctx, w, 0, ptr(a), ptr(l), ptr(e), ptr(out)), "0")
    refused(L.tb_run_composite(ctx, 1 << 13, (1 << 11) + 1, ptr(a), ptr(l), ptr(e), ptr(out)), "2^24")
    with pytest.raises(api.TracerBoyError) as err:   # and through the wrappers: an exception with the code
        gpu_tb.RunComposite(0, h, a, l, e)
    assert err.value.code == -1
