"""The ray visualiser's overlay without a GPU: the known answers of the numpy restatement (tests/visualize_ref.py), worked
by hand; the library's host-only constants; struct sizes; the command-line tool's refusals.

The set-up of the known answers: a camera at the origin looking down -z, lens height 2, focal distance 1, a 16 x 16 picture.  The view ray of the
centre pixel (8, 8) has u = v = 0.5 exactly (no half-pixel offset), so it starts at the origin and runs along (0, 0, -1).  One recorded ray of
bounce 1 crosses that axis at right angles, at distance d = 2: from (-1, 0, -2) along +x, hit after 2.  Its cylinder of radius RayWidth is met at
d - RayWidth, where the cylinder's normal is (0, 0, 1): |n . rd| = 1, so the colour is lerp(0.2, green, 1) = green and the pixel becomes
scene + 0.75 (green - scene).  Its arrow head covers x in [0.6, 1] and is not on the axis."""
import ctypes
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import visualize_ref as ref
from conftest import CORNELL, ROOT

F = np.float32
W = H = 16
CX = CY = 8
D = 2.0
RAY_WIDTH = 0.01
GREEN, YELLOW = (0.0, 1.0, 0.0), (1.0, 1.0, 0.0)
SCENE_VALUE = (0.25, 0.5, 2.0, 1.0)                              # a value above 1 among them


def camera():
    return types.SimpleNamespace(Position=(0.0, 0.0, 0.0), LookAt=(0.0, 0.0, -1.0), Right=(1.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), LensHeight=2.0,
                                 FocalDistance=1.0)


def constants(**kw):
    return ref.constants(camera(), W, H, **{"ray_width": RAY_WIDTH, **kw})


def ray(origin, direction, hit_t, bounce):
    return np.array(list(origin) + list(direction) + [hit_t, bounce], np.float32)


def crossing(bounce=1.0, hit_t=2.0, d=D):
    return ray((-1.0, 0.0, -d), (1.0, 0.0, 0.0), hit_t, bounce)


def scene():
    s = np.empty((H, W, 4), np.float32)
    s[...] = SCENE_VALUE
    return s


def blended(colour):
    return [F(s) + F(0.75) * (F(c) - F(s)) for s, c in zip(SCENE_VALUE, colour)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_centre_view_ray_is_the_axis():
    ro, rd = ref.camera_rays(constants())
    assert [float(c[CY, CX]) for c in ro] == [0.0, 0.0, 0.0] and [float(c[CY, CX]) for c in rd] == [0.0, 0.0, -1.0]
    # uv.y is flipped and there is no half-pixel offset: pixel (0, 0) looks through the lens' top left corner, (-aspect, +1) x lens height / 2
    assert [float(c[0, 0]) for c in ro] == [-1.0, 1.0, 0.0]


def test_cylinder_hit_at_d_minus_width_is_green():
    k = constants()
    ro, rd = ref.camera_rays(k)
    t = ref.cylinder(ro, rd, ref.vec((-1, 0, -D)), ref.vec((1, 0, -D)), F(RAY_WIDTH))
    assert abs(float(t[CY, CX]) - (D - RAY_WIDTH)) < 1e-4          # k0 = 16 - 4 r^2 cancels against 16 in fp32: a few 1e-6 of h, 1e-5 of t
    out = ref.overlay(k, [crossing()], scene())
    assert np.allclose(out[CY, CX, :3], blended(GREEN)[:3], rtol=0, atol=2e-3)   # |n . rd| = 1 up to that cancellation
    assert out[CY, CX, 3] == F(SCENE_VALUE[3])
    assert np.array_equal(bits(out[0, 0]), bits(scene()[0, 0]))    # a pixel the ray does not cover keeps its bits


def test_occluder_in_front_leaves_the_bits_and_nan_stays_nan():
    k, s = constants(), scene()
    s[CY, CX, 0] = np.nan
    near = np.zeros((H, W, 4), np.float32); near[..., 2] = -1.0    # a surface at z = -1, nearer than the ray at d - width
    out = ref.overlay(k, [crossing()], s, near)
    assert np.array_equal(bits(out), bits(s))
    far = np.zeros((H, W, 4), np.float32); far[..., 2] = -3.0      # ... and behind it: the ray draws, and the NaN stays a NaN
    out = ref.overlay(k, [crossing()], s, far)
    assert np.isnan(out[CY, CX, 0]) and abs(float(out[CY, CX, 1]) - float(blended(GREEN)[1])) < 2e-3
    # a world position of all zeros (|xyz| <= 0.0001) is no occluder at all
    out = ref.overlay(k, [crossing()], scene(), np.zeros((H, W, 4), np.float32))
    assert abs(float(out[CY, CX, 1]) - float(blended(GREEN)[1])) < 2e-3


def test_bounce_above_ray_depth_is_skipped():
    out = ref.overlay(constants(ray_depth=1.5), [crossing(bounce=2.0)], scene())
    assert np.array_equal(bits(out), bits(scene()))


def test_half_a_bounce_below_ray_depth_is_half_the_length():
    # RayDepth - bounce = 0.5: the cylinder ends at x = 0 -- where its cap closes it on the axis -- and no longer reaches x = 0.5
    k = constants(ray_depth=1.5)
    ro, rd = ref.camera_rays(k)
    out = ref.overlay(k, [crossing(bounce=1.0)], scene())
    full = ref.overlay(constants(), [crossing(bounce=1.0)], scene())
    # the view ray of column c leaves the lens at x = c / 8 - 1 and meets z = -2 at three times that: columns 9, 10 and 6 at 0.375, 0.75 and -0.75
    covered_full = (bits(full) != bits(scene())).any(-1)[CY]
    covered_half = (bits(out) != bits(scene())).any(-1)[CY]
    assert covered_full[CX + 1] and covered_full[CX + 2]           # x = 0.375 and 0.75 at z = -2 lie on the full ray and its arrow head
    assert not covered_half[CX + 1:].any()                         # ... and beyond the half ray's end
    assert covered_half[CX - 2] and covered_full[CX - 2]           # x = -0.75 lies on both


def test_ray_count_one_draws_the_first_ray_only():
    nearer = crossing(bounce=3.0, d=1.5)                            # a second ray, nearer to the camera: it would win
    both = ref.overlay(constants(), [crossing(), nearer], scene())
    first = ref.overlay(constants(ray_count=1), [crossing(), nearer], scene())
    assert abs(float(both[CY, CX, 0]) - float(blended(YELLOW)[0])) < 2e-3
    assert np.array_equal(bits(first), bits(ref.overlay(constants(), [crossing()], scene())))


def test_bounce_three_is_yellow_and_a_negative_bounce_blue():
    out = ref.overlay(constants(), [crossing(bounce=3.0)], scene())
    assert np.allclose(out[CY, CX, :3], blended(YELLOW)[:3], rtol=0, atol=2e-3)
    out = ref.overlay(constants(), [crossing(bounce=-1.0)], scene())
    assert np.allclose(out[CY, CX, :3], blended((0.0, 0.0, 1.0))[:3], rtol=0, atol=2e-3)


def test_a_missed_ray_has_no_arrow_head():
    # a hit ray's head is the cone from x = 0.6 (radius 10 widths) to x = 1: at z = -2 the pixel column 10 (x = 0.75) sees the pure colour
    hit = ref.overlay(constants(), [crossing()], scene())
    assert np.array_equal(bits(hit[CY, CX + 2, :3]), bits(np.array(blended(GREEN)[:3], np.float32)))
    # the same ray as a miss is 9999999.9 long and has no head: that pixel sees the shaded cylinder, whose normal there is not along the view ray
    miss = ref.overlay(constants(), [crossing(hit_t=-1.0)], scene())
    assert not np.array_equal(bits(miss[CY, CX + 2]), bits(scene()[CY, CX + 2]))
    assert not np.array_equal(bits(miss[CY, CX + 2, :3]), bits(np.array(blended(GREEN)[:3], np.float32)))


def test_view_ray_parallel_to_the_cylinder_divides_by_zero():
    """A recorded ray along the view axis: ba = (0, 0, -1), bard = baba = 1, so k2 = baba - bard^2 = 0.  The literal arithmetic: k1 = 0, k0 = -r^2,
    h = 0, t = (-0 - 0) / 0 = NaN; y = NaN fails the body's test; the cap: t = (baba - baoc) / bard = 2, |k1 + k2 t| = 0 < h = 0 is false: no
    cylinder.  The arrow head's wide cap is met head on, at 1.8 = 0.8 of the ray's length from its origin at z = -1: the pixel is the pure colour."""
    k = constants()
    ro, rd = ref.camera_rays(k)
    start, end = ref.vec((0, 0, -1)), ref.vec((0, 0, -2))
    with np.errstate(all="ignore"):
        assert float(ref.cylinder(ro, rd, start, end, F(RAY_WIDTH))[CY, CX]) == -1.0
        head = ref.cone(ro, rd, ref.add(start, ref.mul(ref.vec((0, 0, -1)), F(1) * F(0.8))), end, F(RAY_WIDTH) * F(10), F(RAY_WIDTH))
    assert abs(float(head[CY, CX]) - 1.8) < 1e-6
    out = ref.overlay(k, [ray((0, 0, -1), (0, 0, -1), 1.0, 1.0)], scene())
    assert np.array_equal(bits(out[CY, CX, :3]), bits(np.array(blended(GREEN)[:3], np.float32)))


def test_rgba8_conversion():
    img = np.array([[[0.0, 0.5, 1.0, 1.0], [-1.0, 2.0, np.nan, 1.0], [0.25, 0.999, 0.001, 1.0]]], np.float32)
    assert ref.to_rgba8(img).tolist() == [[[0, 128, 255, 255], [0, 255, 0, 255], [64, 255, 0, 255]]]


# ---- the library, host only ------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_entry_points(built):
    from tracerboy_amd import _ctypes_abi as abi, api
    assert (ctypes.sizeof(abi.TbVisualizerRay), ctypes.sizeof(abi.TbVisualizeConstants), ctypes.sizeof(abi.TbPathFrame)) == (32, 80, 32)
    assert api.PATH_FRAME_DTYPE.itemsize == 32 and api.VISUALIZER_RAY_DTYPE.itemsize == 32 and abi.TB_MAX_VISUALIZER_RAYS == 1024
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracerboy_hip.h")).read(), flags=re.S)
    raw, bound = ctypes.CDLL(api.LIB_PATH), api.lib()
    for name in ("tb_record_paths", "tb_clear_paths", "tb_read_paths", "tb_visualize_rays", "tb_visualize_constants", "tb_run_visualize_rays",
                 "tb_default_visualize_settings"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in bound._tb_exports and getattr(bound, name).argtypes is not None, name
    blob = open(api.LIB_PATH, "rb").read()
    assert all(n in blob for n in (b"last_paths_us\0", b"last_visualize_us\0", b"visualize_depth_source\0"))
    for name in ("RecordPaths", "ReadPaths", "ClearPaths", "VisualizeRays", "RunVisualizeRays"):
        assert callable(getattr(api.TracerBoy, name)), name
    s = api.GetDefaultVisualizeSettings()
    assert (s.RayWidth, s.RayDepth, s.RayCount) == (float(F(0.01)), 10.0, 0)   # TracerBoy.h:303-306


def test_constants_for_the_cornell_box_camera(built, cornell_host):
    """The cornell-box file: Transform with the eye at z = 6.8 looking down -z, fov 19.5 degrees.  Lens height 2, so the focal distance is
    1 / tan(fov / 2) and the lens sits that + 0.01 in front of the eye (host_scene.cpp)."""
    from tracerboy_amd import api
    cam = cornell_host.camera()
    k = api.VisualizeConstants(cam, 800, 600)
    focal = 1.0 / math.tan(math.radians(19.5) / 2.0)
    assert (k.ResolutionX, k.ResolutionY, k.RayCount) == (800, 600, 999999) and k.CylinderRadius == float(F(0.01)) and k.RayDepth == 10.0
    assert abs(k.FocalLength - focal) < 1e-5 and k.LensHeight == 2.0 and k.Padding2 == 0.0
    assert list(k.CameraPosition)[:2] == [0.0, 1.0] and abs(k.CameraPosition[2] - (6.8 - focal - 0.01)) < 1e-5
    assert list(k.CameraLookAt)[:2] == [0.0, 1.0] and abs(k.CameraLookAt[2] - (k.CameraPosition[2] - 1.0)) < 1e-6
    assert [abs(v) for v in k.CameraRight] == [1.0, 0.0, 0.0] and [abs(v) for v in k.CameraUp] == [0.0, 1.0, 0.0] and k.CameraRight[0] == 1.0
    # the layout of VisualizeRaysSharedShaderStructs.h: float3 + scalar rows
    words = np.frombuffer(bytes(k), np.uint32)
    assert words[0] == 800 and words[1] == 600 and words[19] == 999999
    assert words[2:4].view(np.float32).tolist() == [k.CylinderRadius, k.FocalLength] and words[7:8].view(np.float32)[0] == 2.0
    assert words[11:12].view(np.float32)[0] == 10.0 and words[4:7].view(np.float32).tolist() == list(k.CameraPosition)
    # settings reach it, a count above 0 stays; the restatement's own constants are the same numbers
    s = api.GetDefaultVisualizeSettings(); s.RayWidth = 0.25; s.RayDepth = 2.5; s.RayCount = 7
    k2 = api.VisualizeConstants(cam, 17, 9, s)
    assert (k2.CylinderRadius, k2.RayDepth, k2.RayCount, k2.ResolutionX, k2.ResolutionY) == (0.25, 2.5, 7, 17, 9)
    mine = ref.constants(cam, 17, 9, 0.25, 2.5, 7)
    assert mine.RayCount == 7 and float(mine.FocalLength) == k2.FocalLength and [float(v) for v in mine.CameraUp] == list(k2.CameraUp)
    with pytest.raises(api.TracerBoyError):
        api.VisualizeConstants(cam, 0, 9)


def test_cli_mistakes_exit_2_before_any_device_call(built):
    cli = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # a device call would fail with status 1, not 2
    for args, message in ((["--visualize-rays", "12"], "--visualize-rays is X,Y"), (["--visualize-rays", "12,"], "--visualize-rays is X,Y"),
                          (["--visualize-rays", "a,b"], "--visualize-rays is X,Y"), (["--visualize-rays", "-1,2"], "--visualize-rays is X,Y"),
                          (["--visualize-frames", "0:4"], "need --visualize-rays"), (["--paths-out", "p.jsonl"], "need --visualize-rays"),
                          (["--visualize-rays", "1,2", "--visualize-frames", "4:4"], "--visualize-frames is A:B"),
                          (["--visualize-rays", "1,2", "--visualize-width", "0"], "--visualize-width"),
                          (["--visualize-rays", "1,2", "--visualize-depth", "nan"], "--visualize-depth"),
                          (["--visualize-rays", "1,2", "--visualize-count", "-3"], "--visualize-count"),
                          (["--visualize-rays", "1,2", "--upscale", "64x64"], "does not go with"),
                          (["--visualize-rays", "1,2", "--render-scale", "0.5"], "does not go with"),
                          (["--visualize-rays", "1,2", "--ranks", "2"], "does not go with"),
                          (["--visualize-rays", "48,2", "--width", "48", "--height", "32"], "lies outside the 48x32 frame")):
        r = subprocess.run([cli, CORNELL] + args, capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([cli], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and all(f in r.stderr for f in ("--visualize-rays", "--visualize-frames", "--visualize-width", "--visualize-depth",
                                                               "--visualize-count", "--paths-out"))
