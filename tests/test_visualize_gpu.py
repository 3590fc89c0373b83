"""The path inspector on the GPU: a pixel's paths recorded again (tb_record_paths), the reference's ray buffer, the overlay
kernel against the numpy restatement (tests/visualize_ref.py), the stage and the command-line tool.  Every comparison is on bits (a NaN for a NaN:
a host and a device NaN may differ in sign and payload, as in tests/test_math.py)."""
import copy
import json
import os
import subprocess
import types

import numpy as np
import pytest

import visualize_ref as ref
from conftest import CORNELL, GOLDEN
from test_still_denoise import CLI, bits, same
from test_visualize_ref import crossing, ray

pytestmark = pytest.mark.gpu

F32 = np.float32
TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6
TB_AOV_WORLD_POSITION0 = 3
JITTERED, REJECTED, TRUNCATED = 1, 2, 4
SCENES = {name: os.path.join(GOLDEN, "scenes", name, "scene.pbrt") for name in ("cornell-box", "mix-glass", "Teapot", "instances")}
W, H, FRAMES = 24, 16, 12


def context(scene, **opts):
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    for k, v in opts.items():
        tb.SetOption(k, v)
    tb.LoadScene(scene)
    return tb


@pytest.fixture(scope="module")
def s4(built, settings):
    s = copy.copy(settings); s.MaxBounces = 4; s.EnableBlueNoise = 0
    return s


@pytest.fixture(scope="module", params=sorted(SCENES))
def run(request, built, s4):
    """A plain render of FRAMES frames from frame 0 (instances: the two-level walk), its two surfaces read once."""
    name = request.param
    tb = context(SCENES[name], **({"flatten_instances": 0} if name == "instances" else {}))
    tb.Render(W, H, FRAMES, s4, 0.0)
    acc, jit = tb.ReadAccumulation(jittered=True)
    yield types.SimpleNamespace(tb=tb, name=name, acc=acc, jit=jit)
    tb.close()


def pixels_of(run):
    """The corners, the brightest pixel (it sees the light, or the brightest thing there is) and, where there is one, a pixel no frame of which hit
    anything: black sums under a weight (no scene here has an environment map)."""
    lum = run.acc[..., :3].sum(-1)
    y, x = np.unravel_index(int(np.argmax(lum)), lum.shape)
    px = [(0, 0), (W - 1, H - 1), (int(x), int(y)), (W // 2, H // 2)]   # ... and the centre, which looks at geometry in every scene
    empty = np.argwhere((run.acc[..., :3] == 0).all(-1) & (run.acc[..., 3] > 0))
    if run.name == "instances":
        assert len(empty), "instances has camera rays that leave the scene"
    if len(empty):
        px.append((int(empty[0][1]), int(empty[0][0])))
    return px


def fold(frames, only_flag=0):
    acc = np.zeros(4, F32)
    for f in frames:
        if only_flag and not (int(f["flags"]) & only_flag):
            continue
        acc = f["sum"].astype(F32) + acc                             # acc = o + acc, pt_stream.inc:93
    return acc


# ---- 1, 2: the recorded paths are the render's, every stored ray is a real ray ----------------------------------------------------------------
def test_recorded_sums_are_the_renders_pixels(run):
    tb = run.tb
    before = tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()
    for x, y in pixels_of(run):
        tb.ClearPaths()
        frames, total = tb.RecordPaths(x, y, 0, FRAMES)
        assert frames["frame"].tolist() == list(range(FRAMES)) and int(frames["flags"][0]) & JITTERED
        assert np.array_equal(bits(fold(frames)), bits(run.acc[y, x])), (run.name, x, y, fold(frames), run.acc[y, x])
        assert np.array_equal(bits(fold(frames, JITTERED)), bits(run.jit[y, x])), (run.name, x, y)
        assert total == int(frames["num_rays"].sum())
    assert (tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()) == before
    assert tb.GetOption("last_paths_us") > 0


def test_every_stored_ray_is_a_real_ray(run, s4):
    tb = run.tb
    seen = 0
    for x, y in pixels_of(run):
        tb.ClearPaths()
        frames, total = tb.RecordPaths(x, y, 0, FRAMES)
        rays = tb.ReadPaths()
        assert len(rays) == total <= FRAMES * (s4.MaxBounces - 1)
        at = 0
        for f in frames:                                             # first_ray / num_rays index exactly that frame's records, bounces 1, 2, ...
            n = int(f["num_rays"])
            assert n <= s4.MaxBounces - 1 and not int(f["flags"]) & TRUNCATED
            assert int(f["first_ray"]) == (at if n else 0xffffffff)
            assert rays["BounceCount"][at:at + n].tolist() == [float(b) for b in range(1, n + 1)]
            at += n
        assert at == total
        if not total:
            continue
        t = tb.TraceClosest(rays["Origin"], rays["Direction"])["t"]
        assert np.array_equal(bits(t), bits(rays["HitT"])), (run.name, x, y)   # -1 for a miss on both sides
        seen += total
    assert seen > 0
    if run.name == "instances":
        x, y = pixels_of(run)[-1]
        tb.ClearPaths()
        frames, total = tb.RecordPaths(x, y, 0, FRAMES)
        assert total == 0 and not frames["sum"][:, :3].any() and (frames["first_ray"] == 0xffffffff).all()


# ---- 3: order and cap -------------------------------------------------------------------------------------------------------------------------
def test_calls_append_in_frame_order(run):
    tb = run.tb
    x, y = pixels_of(run)[3]
    tb.ClearPaths()
    whole, total = tb.RecordPaths(x, y, 0, FRAMES)
    rays = tb.ReadPaths()
    assert total > 0
    tb.ClearPaths()
    assert len(tb.ReadPaths()) == 0
    a, ta = tb.RecordPaths(x, y, 0, 8)
    b, tb_ = tb.RecordPaths(x, y, 8, FRAMES - 8)
    assert ta + tb_ == total and tb.ReadPaths().tobytes() == rays.tobytes()
    assert np.concatenate([a, b]).tobytes() == whole.tobytes()       # the second call's first_ray counts on from the first call's rays
    tb.ClearPaths()
    again, _ = tb.RecordPaths(x, y, 0, FRAMES)                       # two identical calls give identical bytes
    assert again.tobytes() == whole.tobytes() and tb.ReadPaths().tobytes() == rays.tobytes()


def test_cap_and_clearing(built, s4):
    """4096 frames of a cornell-box wall pixel: up to MaxBounces - 1 = 3 rays a frame, far more than the buffer's 1024."""
    from tracerboy_amd import api
    with context(CORNELL) as tb:
        tb.Render(W, H, 1, s4, 0.0)
        x, y = W // 2, H // 2                                        # the back wall
        frames, total = tb.RecordPaths(x, y, 0, 4096)
        assert 1024 < total <= 4096 * (s4.MaxBounces - 1) and total == int(frames["num_rays"].sum())
        rays = tb.ReadPaths()
        assert len(rays) == 1024
        starts = np.concatenate([np.zeros(1, np.int64), np.cumsum(frames["num_rays"].astype(np.int64))[:-1]])
        cut = int(np.argmax(starts + frames["num_rays"] > 1024))     # the frame where the cap fell
        truncated = (frames["flags"] & TRUNCATED) != 0
        assert not truncated[:cut].any() and truncated[cut:][frames["num_rays"][cut:] > 0].all() and not truncated[frames["num_rays"] == 0].any()
        assert frames["first_ray"][cut] == (starts[cut] if starts[cut] < 1024 else 0xffffffff)
        assert (frames["first_ray"][cut + 1:] == 0xffffffff).all()
        tb.ClearPaths()
        short, short_total = tb.RecordPaths(x, y, 0, cut + 1)        # a run cut off at that frame stores the same 1024 rays
        assert short_total == int(starts[cut] + frames["num_rays"][cut]) and tb.ReadPaths().tobytes() == rays.tobytes()
        assert short.tobytes() == frames[:cut + 1].tobytes()
        _, more = tb.RecordPaths(x, y, 0, 4)                         # a full buffer drops everything, and says what it dropped
        assert more == int(frames["num_rays"][:4].sum()) and tb.ReadPaths().tobytes() == rays.tobytes()
        # whatever resets the history empties the buffer
        tb.ClearPaths(); assert len(tb.ReadPaths()) == 0
        tb.RecordPaths(x, y, 0, 4); assert len(tb.ReadPaths()) > 0
        tb.SetCamera(tb.GetCamera()); assert len(tb.ReadPaths()) == 0
        tb.RecordPaths(x, y, 0, 4); assert len(tb.ReadPaths()) > 0
        tb.LoadScene(CORNELL); assert len(tb.ReadPaths()) == 0
        tb.Render(W, H, 1, s4, 0.0)
        tb.RecordPaths(x, y, 0, 4); assert len(tb.ReadPaths()) > 0
        tb.Render(W + 8, H, 1, s4, 0.0); assert len(tb.ReadPaths()) == 0   # a resize


# ---- 4: the overlay kernel against the restatement --------------------------------------------------------------------------------------------
def synthetic_rays(n, seed):
    """Rays in front of the known-answer camera (tests/test_visualize_ref.py): origins in a box around the view axis, unit directions, hits and
    misses, bounces 1 to 4 and a feeler's negative count; the known-answer rays first."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), F32)
    r[:, 0:2] = rng.uniform(-1.5, 1.5, (n, 2)); r[:, 2] = rng.uniform(-6.0, -1.0, n)
    d = rng.normal(size=(n, 3)).astype(F32)
    r[:, 3:6] = d / np.sqrt((d * d).sum(-1, keepdims=True))
    r[:, 6] = np.where(rng.uniform(size=n) < 0.25, -1.0, rng.uniform(0.2, 3.0, n))
    r[:, 7] = rng.integers(1, 5, n)
    known = [crossing(), crossing(bounce=3.0, d=1.5), crossing(hit_t=-1.0, d=3.0), ray((0, 0, -1), (0, 0, -1), 1.0, 1.0), crossing(bounce=-1.0, d=2.5)]
    for i, k in enumerate(known[:n]):
        r[i] = k
    return r


@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (64, 48)])
def test_overlay_kernel_is_the_restatement(gpu_tb, w, h):
    from test_visualize_ref import camera
    rng = np.random.default_rng(w * 100 + h)
    scene = rng.uniform(0.0, 3.0, (h, w, 4)).astype(F32)             # values above 1 among them
    scene.reshape(-1, 4)[::5, 1] = np.nan
    world = np.zeros((h, w, 4), F32)
    world[..., 2] = rng.uniform(-5.0, -1.5, (h, w))                  # an occluder at varying depth; holes where there is none
    world[..., 0] = rng.uniform(-0.5, 0.5, (h, w))
    world.reshape(-1, 4)[::3] = 0
    for n in (0, 1, 65, 1024):
        rays = synthetic_rays(n, n + 1)
        for depth, count in ((10.0, 0), (2.5, 0), (10.0, 3)):
            if n == 1024 and (depth, count) != (10.0, 0):
                continue                                             # the restatement's loop over 1024 rays once per size
            k = ref.constants(camera(), w, h, ray_width=0.05, ray_depth=depth, ray_count=count)
            kc = _constants_struct(k)
            for wp in (None, world):
                got = gpu_tb.RunVisualizeRays(kc, rays, scene, wp)
                want = ref.overlay(k, rays, scene, wp)
                assert same(got, want), (w, h, n, depth, count, wp is not None, int((bits(got) != bits(want)).sum()))
                if n >= 65 and w > 1 and (depth, count) == (10.0, 0):
                    assert (bits(got) != bits(scene)).any()          # something was drawn
            if n == 0:
                assert same(got, scene)


def _constants_struct(k):
    from tracerboy_amd import _ctypes_abi as abi
    c = abi.TbVisualizeConstants()
    c.ResolutionX, c.ResolutionY, c.CylinderRadius, c.FocalLength = k.ResolutionX, k.ResolutionY, float(k.CylinderRadius), float(k.FocalLength)
    c.LensHeight, c.RayDepth, c.RayCount = float(k.LensHeight), float(k.RayDepth), k.RayCount
    for name in ("CameraPosition", "CameraLookAt", "CameraRight", "CameraUp"):
        for i in range(3):
            getattr(c, name)[i] = float(getattr(k, name)[i])
    return c


def test_overlay_known_answers_on_the_device(gpu_tb):
    from test_visualize_ref import camera, scene, blended, GREEN, CX, CY
    k = ref.constants(camera(), 16, 16, ray_width=0.01)
    got = gpu_tb.RunVisualizeRays(_constants_struct(k), np.stack([crossing()]), scene())
    assert np.allclose(got[CY, CX, :3], blended(GREEN)[:3], rtol=0, atol=2e-3) and same(got, ref.overlay(k, [crossing()], scene()))
    parallel = np.stack([ray((0, 0, -1), (0, 0, -1), 1.0, 1.0)])     # k2 == 0: the division by zero is the reference's, and the device's
    assert same(gpu_tb.RunVisualizeRays(_constants_struct(k), parallel, scene()), ref.overlay(k, parallel, scene()))


# ---- 5: the stage -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", [1, 2, 0])
def test_stage_equals_the_kernel_on_the_read_back_inputs(built, s4, source):
    from tracerboy_amd import api
    w, h, frames = 40, 24, 6
    with context(CORNELL, **({"aov": 1} if source == 1 else {})) as tb:
        tb.Render(w, h, frames, s4, 0.0)
        if source == 2:
            tb.RenderGuides(frames - 2, 2)
        for x, y in ((20, 12), (5, 20)):
            tb.RecordPaths(x, y, 0, frames)
        rays = tb.ReadPaths()
        assert len(rays) > 4
        vs = api.GetDefaultVisualizeSettings(); vs.RayWidth = 0.03
        with pytest.raises(api.TracerBoyError) as e:                 # no post-processed picture yet
            tb.VisualizeRays(vs)
        assert e.value.code == TB_E_INVALID and "tb_post_process" in str(e.value)
        post_f, post_b = tb.PostProcess()
        before = tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()
        got_f, got_b = tb.VisualizeRays(vs)
        assert tb.GetOption("visualize_depth_source") == source and tb.GetOption("last_visualize_us") > 0
        world = None
        if source == 1:
            world = tb.ReadAOV(TB_AOV_WORLD_POSITION0 + (frames - 1) % 2)
        elif source == 2:
            position, hits = tb.ReadGuide(2), tb.ReadGuide(1)[..., 3:4]
            with np.errstate(all="ignore"):
                world = np.where(hits > 0, position / hits, F32(0)).astype(F32)
        k = api.VisualizeConstants(tb.GetCamera(), w, h, vs)
        want = tb.RunVisualizeRays(k, rays, post_f, world)
        assert same(got_f, want) and same(want, ref.overlay(k, rays, post_f, world))
        drawn = (bits(got_f) != bits(post_f)).any(-1)
        assert drawn.sum() > 10                                      # the rays are in the picture
        assert np.array_equal(got_b, ref.to_rgba8(got_f))            # the 8-bit picture is the conversion of the float one
        again_f, again_b = tb.VisualizeRays(vs)                      # the post output was not drawn into: nothing is drawn twice
        assert same(again_f, got_f) and np.array_equal(again_b, got_b)
        assert (tb.AccumDigest(), tb.GetNumberOfSamplesSinceLastInvalidate()) == before
        if source == 0:                                              # without an occluder every ray draws on top
            assert same(got_f, tb.RunVisualizeRays(k, rays, post_f, None))
        tb.ClearPaths()
        assert same(tb.VisualizeRays(vs)[0], post_f)                 # an empty buffer: the picture itself


def test_refusals(built, s4):
    from tracerboy_amd import api

    def refused(call, code, word):
        with pytest.raises(api.TracerBoyError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    with api.TracerBoy(0) as tb:
        tb.width, tb.height = 32, 24
        refused(lambda: tb.RecordPaths(0, 0, 0, 1), TB_E_INVALID, "no scene")
        tb.LoadScene(CORNELL)
        refused(lambda: tb.RecordPaths(0, 0, 0, 1), TB_E_INVALID, "no size")
        tb.Render(32, 24, 2, s4, 0.0)
        refused(lambda: tb.RecordPaths(0, 0, 0, 0), TB_E_INVALID, "n_frames")
        refused(lambda: tb.RecordPaths(0, 0, 0, 4097), TB_E_INVALID, "n_frames")
        refused(lambda: tb.RecordPaths(32, 0, 0, 1), TB_E_INVALID, "outside")
        refused(lambda: tb.RecordPaths(0, 24, 0, 1), TB_E_INVALID, "outside")
        tb.RecordPaths(31, 23, 1000, 3)                              # any frame range
        tb.RenderRealTime(32, 24, s4, None, 0.0)
        refused(lambda: tb.RecordPaths(0, 0, 0, 1), TB_E_INVALID, "tb_render_realtime")
        tb.Render(32, 24, 2, s4, 0.0)
        tb.PostProcess()
        tb.SetTileAssignment(0, 2)
        tb.Render(128, 64, 1, s4, 0.0)
        refused(lambda: tb.RecordPaths(0, 0, 0, 1), TB_E_UNSUPPORTED, "tile assignment")
        refused(lambda: tb.VisualizeRays(), TB_E_UNSUPPORTED, "tile assignment")
    with api.TracerBoy(devices=[0, 0]) as g:                         # a two-member group on one device
        g.LoadScene(CORNELL)
        g.Render(64, 64, 1, s4, 0.0)
        refused(lambda: g.RecordPaths(0, 0, 0, 1), TB_E_UNSUPPORTED, "group")
        refused(lambda: g.VisualizeRays(), TB_E_UNSUPPORTED, "group")


# ---- 6: the command-line tool -----------------------------------------------------------------------------------------------------------------
def test_cli_visualize_rays(built, tmp_path):
    from tracerboy_amd import api
    from test_render_state import read_pfm
    w, h, spp, x, y = 48, 32, 8, 24, 20
    common = [CLI, CORNELL, "--width", str(w), "--height", str(h), "--spp", str(spp), "--depth", "4", "--blue-noise", "0"]
    plain, drawn, mean, paths = (str(tmp_path / n) for n in ("plain.png", "drawn.png", "mean.pfm", "paths.jsonl"))
    for extra in (["--out", plain], ["--out", mean],
                  ["--out", drawn, "--visualize-rays", "%d,%d" % (x, y), "--visualize-frames", "0:%d" % spp, "--visualize-width", "0.03", "--paths-out", paths]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    assert "paths: pixel (%d, %d), frames [0, %d)" % (x, y, spp) in r.stdout and "visualize: depth source 2" in r.stdout
    plain_img, drawn_img = api.DecodeImage(plain)[0], api.DecodeImage(drawn)[0]
    assert plain_img.shape == drawn_img.shape == (h, w, 4) and (plain_img != drawn_img).any()
    # the same calls through the API
    s = api.GetDefaultOutputSettings(); s.MaxBounces = 4; s.EnableBlueNoise = 0
    vs = api.GetDefaultVisualizeSettings(); vs.RayWidth = 0.03
    with context(CORNELL) as tb:
        tb.Render(w, h, spp, s, 0.0)
        tb.RenderGuides(spp - 1, 1)
        frames, total = tb.RecordPaths(x, y, 0, spp)
        rays = tb.ReadPaths()
        tb.PostProcess()
        _, want = tb.VisualizeRays(vs)
    assert np.array_equal(np.rint(drawn_img[..., :3] * 255).astype(np.uint8), want[..., :3])
    # the JSON lines: one per frame, their sums add up to the plain run's pixel, their rays are the buffer's
    lines = [json.loads(l) for l in open(paths)]
    assert [l["frame"] for l in lines] == list(range(spp)) and [l["flags"] for l in lines] == frames["flags"].tolist()
    acc = np.zeros(4, F32)
    for l in lines:
        acc = np.array(l["sum"], F32) + acc
    assert np.array_equal(bits(acc), bits(fold(frames)))
    inv = F32(1) / acc[3]
    assert np.array_equal(bits(acc[:3] * inv), bits(np.ascontiguousarray(read_pfm(mean)[y, x], F32)))
    flat = [r for l in lines for r in l["rays"]]
    assert len(flat) == total == len(rays) and [l["num_rays"] for l in lines] == frames["num_rays"].tolist()
    assert np.array_equal(bits(np.array([r["origin"] + r["direction"] + [r["hit_t"], r["bounce"]] for r in flat], F32)), bits(ref.ray_words(rays)))
