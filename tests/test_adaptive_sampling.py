"""-m gpu: adaptive sampling (option "adaptive") -- converged pixels skip their samples, the live ones run packed 256 to a
workgroup.  None of these tests uses the oracle: the plain path they compare against is held bit-exact to it by the rest of the suite.

The prediction: a pixel that skips once stays frozen (its sums and the threshold no longer change), so after any call an adaptive context's
pixel is the plain context's state at the first frame where the skip test held on that state, or the plain context's latest state.  The skip
test is restated here in NumPy float32, operation for operation.  Every threshold is taken from the data and checked to leave between 10 % and
90 % of the pixels live, so that no test passes vacuously."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TEAPOT = os.path.join(GOLDEN, "scenes", "Teapot", "scene.pbrt")
MIX = os.path.join(GOLDEN, "scenes", "mix-glass", "scene.pbrt")
INSTANCES = os.path.join(GOLDEN, "scenes", "instances", "scene.pbrt")
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
ALBEDO, LIVE_PIXELS = 1, 7
RULE_ADAPTIVE = 7
MIN = 16


def skip_test(o, q, thr):
    """c = o.rgb / o.a, j = q.rgb / q.a; black, or ((|dr| + |dg|) + |db|) / sqrt((c.r + c.g) + c.b) < thr."""
    with np.errstate(all="ignore"):
        c = o[..., :3] / o[..., 3:4]
        j = q[..., :3] / q[..., 3:4]
        black = (c[..., 0] <= 0) & (c[..., 1] <= 0) & (c[..., 2] <= 0)
        err = ((np.abs(j[..., 0] - c[..., 0]) + np.abs(j[..., 1] - c[..., 1])) + np.abs(j[..., 2] - c[..., 2])) / np.sqrt((c[..., 0] + c[..., 1]) + c[..., 2])
        return black, err, black | (err < np.float32(thr))


def skips(st, thr):
    return skip_test(st[0], st[1], thr)[2]


def threshold_for(st, share):
    """A float32 threshold under which about `share` of the pixels' errors lie."""
    black, err, _ = skip_test(st[0], st[1], 0.0)
    e = np.sort(err[~black & np.isfinite(err)])
    return float(np.float32(e[min(len(e) - 1, int(len(e) * share))]))


def checked_threshold(st, share):
    thr = threshold_for(st, share)
    live = 1.0 - skips(st, thr).mean()
    assert 0.1 <= live <= 0.9, "threshold %g leaves %.1f %% of the pixels live" % (thr, 100 * live)
    return thr


def state(tb):
    o, j = tb.ReadAccumulation(jittered=True)
    return o, j


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def frozen(states, thr):
    """states[0..k]: a plain context's surfaces before k one-frame steps and after each.  An adaptive context's after the same frames: states[j]
    for a pixel whose skip test first held on states[j] (j < k), states[k] elsewhere; and j (k: never)."""
    k = len(states) - 1
    o, q = states[-1][0].copy(), states[-1][1].copy()
    first = np.full(o.shape[:2], k)
    for j, (so, sq) in enumerate(states[:-1]):
        m = skips((so, sq), thr) & (first == k)
        o[m] = so[m]; q[m] = sq[m]; first[m] = j
    return o, q, first


def context(scene, adaptive=False, min_frames=None, opts=None):
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    for k, v in (opts or {}).items():
        tb.SetOption(k, v)
    tb.LoadScene(scene)
    if adaptive:
        tb.SetOption("adaptive", 1)
    if min_frames is not None:
        tb.SetOption("adaptive_min_frames", min_frames)
    return tb


def test_options_refusals_and_calls_below_the_threshold(settings):
    from tracerboy_amd import api
    s = copy.copy(settings); s.ConvergencePercentage = 0.5     # large: nearly every pixel would skip once skipping is allowed
    W, H = 64, 48
    with context(CORNELL) as a, context(CORNELL) as b:
        assert b.GetOption("adaptive") == 0 and b.GetOption("adaptive_min_frames") == 1024    # the defaults
        b.SetOption("adaptive", 1); b.SetOption("adaptive_min_frames", 6)
        assert b.GetOption("adaptive") == 1 and b.GetOption("adaptive_min_frames") == 6
        with pytest.raises(api.TracerBoyError) as e:
            b.SetOption("adaptive_min_frames", -1)
        assert e.value.code == -1 and b.GetOption("adaptive_min_frames") == 6
        with pytest.raises(api.TracerBoyError) as e:
            b.SetOption("count_rays", 1)
        assert e.value.code == -1 and "count_rays" in str(e.value) and b.GetOption("count_rays") == 0
        for n in (3, 2, 2):                                     # frames 0 .. 6: at or below the threshold, today's calls
            a.Render(W, H, n, s, 0.0); b.Render(W, H, n, s, 0.0)
            assert b.GetOption("last_adaptive") == 0 and b.LivePixels() == W * H
            assert b.GetOption("last_plan_rule_pipeline") == a.GetOption("last_plan_rule_pipeline") != RULE_ADAPTIVE
            assert same(state(a)[0], state(b)[0]) and same(state(a)[1], state(b)[1])
        b.Render(W, H, 1, s, 0.0)                               # frame 7: the refusals left a context that renders, adaptively
        assert b.GetOption("last_adaptive") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE
    with context(CORNELL) as c:
        c.SetOption("count_rays", 1)
        with pytest.raises(api.TracerBoyError) as e:
            c.SetOption("adaptive", 1)
        assert e.value.code == -1
        c.Render(16, 16, 1, s, 0.0)


# scene, frame, options, depth
CASES = {
    "cornell_64x48": (CORNELL, 64, 48, {}, 4),
    "cornell_37x23": (CORNELL, 37, 23, {}, 4),
    "cornell_200x120": (CORNELL, 200, 120, {}, 4),
    "teapot": (TEAPOT, 64, 48, {}, 4),
    "mix_glass_from_memory": (MIX, 64, 48, {"scene_in_lds": 0}, 6),
    "instances_two_level": (INSTANCES, 64, 48, {"flatten_instances": 0}, 4),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_frame_per_call_is_the_frozen_plain_render(settings, case):
    scene, W, H, opts, depth = CASES[case]
    s = copy.copy(settings); s.MaxBounces = depth
    with context(scene, opts=opts) as a, context(scene, True, MIN, opts) as b:
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        S = [state(a)]
        assert b.GetOption("last_adaptive") == 0 and same(S[0][0], state(b)[0])
        thr = checked_threshold(S[0], 0.5)
        s.ConvergencePercentage = thr                           # (not a history-relevant setting: the sums go on)
        for k in range(8):
            before = state(b)
            a.Render(W, H, 1, s, 0.0); b.Render(W, H, 1, s, 0.0)
            S.append(state(a))
            assert b.GetOption("last_adaptive") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE
            assert b.LivePixels() == int((~skips(before, thr)).sum()), "call %d" % k
            po, pq, _ = frozen(S, thr)
            got = state(b)
            assert same(got[0], po) and same(got[1], pq), "call %d: %d pixels differ from the prediction" % (k, int((bits(got[0]) != bits(po)).any(-1).sum()))


def test_feature_sets_and_scene_placements(settings):
    """The cases above cover at least three feature sets and both the scene-in-LDS and the from-memory launches."""
    ran = set()
    for case, (scene, W, H, opts, depth) in sorted(CASES.items()):
        s = copy.copy(settings); s.MaxBounces = depth; s.ConvergencePercentage = 0.01
        with context(scene, True, 2, opts) as b:
            b.Render(W, H, 5, s, 0.0)
            assert b.GetOption("last_adaptive") == 1
            ran.add((b.GetOption("last_variant"), b.GetOption("scene_in_lds_active")))
    assert len({v for v, _ in ran}) >= 3, ran
    assert {l for _, l in ran} == {0, 1}, ran


def test_several_frames_per_call_retire_lanes_mid_call(settings):
    W, H = 64, 48
    s = copy.copy(settings)
    with context(CORNELL) as a, context(CORNELL, True, MIN) as b:
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        S = [state(a)]
        thr = checked_threshold(S[0], 0.3)
        s.ConvergencePercentage = thr
        for _ in range(7):
            a.Render(W, H, 1, s, 0.0); S.append(state(a))
        b.Render(W, H, 7, s, 0.0)
        assert b.LivePixels() == int((~skips(S[0], thr)).sum())
        po, pq, first = frozen(S, thr)
        got = state(b)
        assert same(got[0], po) and same(got[1], pq), "%d pixels differ from the prediction" % int((bits(got[0]) != bits(po)).any(-1).sum())
        assert ((first >= 1) & (first <= 6)).sum() > 0, "no lane retired inside the call"


def test_reference_threshold_1024_frames(settings):
    W = H = 32
    s = copy.copy(settings)
    with context(CORNELL) as a, context(CORNELL, True) as b:
        a.Render(W, H, 1024, s, 0.0); b.Render(W, H, 1024, s, 0.0)
        a.Render(W, H, 1, s, 0.0); b.Render(W, H, 1, s, 0.0)     # frame 1024 never skips
        S = [state(a)]
        assert b.GetOption("last_adaptive") == 0 and same(S[0][0], state(b)[0]) and same(S[0][1], state(b)[1])
        thr = checked_threshold(S[0], 0.5)
        s.ConvergencePercentage = thr
        for k in range(5):                                      # frames 1025 .. 1029
            before = state(b)
            a.Render(W, H, 1, s, 0.0); b.Render(W, H, 1, s, 0.0)
            S.append(state(a))
            assert b.GetOption("last_adaptive") == 1 and b.LivePixels() == int((~skips(before, thr)).sum())
            po, pq, _ = frozen(S, thr)
            assert same(state(b)[0], po) and same(state(b)[1], pq), "frame %d" % (1025 + k)
        assert b.GetNumberOfSamplesSinceLastInvalidate() == 1030


@pytest.mark.parametrize("otype", [ALBEDO, LIVE_PIXELS])
def test_aovs_of_skipped_and_live_pixels(settings, otype):
    from tracerboy_amd import api
    W, H = 64, 48
    s = copy.copy(settings); s.OutputType = otype
    with context(TEAPOT, opts={"aov": 1}) as a, context(TEAPOT, True, MIN, {"aov": 1}) as b:
        cam = a.GetCamera()                                     # tilted up to the horizon: the floor's far edge against the sky, camera rays that miss
        d = np.array(cam.LookAt[:]) - np.array(cam.Position[:])
        for i in range(3):
            cam.LookAt[i] = cam.LookAt[i] + 0.4 * float(np.linalg.norm(d)) * cam.Up[i]
        a.SetCamera(cam); b.SetCamera(cam)
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        S0 = state(a)
        prev = {i: a.ReadAOV(i) for i in range(2, 8)}
        thr = checked_threshold(S0, 0.3)
        s.ConvergencePercentage = thr
        a.Render(W, H, 1, s, 0.0); b.Render(W, H, 1, s, 0.0)
        assert b.GetOption("last_adaptive") == 1
        A = {i: a.ReadAOV(i) for i in range(2, 8)}
        B = {i: b.ReadAOV(i) for i in range(2, 8)}
        skipped, live = skips(S0, thr), ~skips(S0, thr)
        o = S0[0]
        c = o / o[..., 3:4]
        one = np.array([0, 0, 0, 1], np.float32)
        # a skipped pixel: ClearAOVs + OutputLivePixels(skip); every other AOV as its last live sample left it
        assert same(B[2][skipped], np.broadcast_to(one, B[2][skipped].shape))
        assert same(B[5][skipped], (c if otype == LIVE_PIXELS else np.broadcast_to(one, o.shape))[skipped])
        for i in (3, 4, 6, 7):
            assert same(B[i][skipped], prev[i][skipped]), "AOV %d" % i
        # a live pixel: the plain render's sample
        for i in (2, 3, 4, 6, 7):
            assert same(B[i][live], A[i][live]), "AOV %d" % i
        if otype == ALBEDO:
            assert same(B[5][live], A[5][live])
        else:
            noalb = live & np.all(bits(A[5]) == bits(one), axis=-1)     # samples that stored no albedo: Teapot's missed camera rays
            assert noalb.sum() > 0
            tint = np.stack([c[..., 0], np.float32(0.2) * c[..., 1], np.float32(0.2) * c[..., 2], c[..., 3]], -1)
            want = np.where(noalb[..., None], tint, A[5])
            assert same(B[5][live], want[live])
        img, _ = b.PostProcess(api.GetDefaultPostProcessSettings(), outputType=LIVE_PIXELS, rgba8=True)
        assert img.shape == (H, W, 4)


def test_tile_ranks_add_up_to_the_whole_frame(settings):
    import torch
    from tracerboy_amd import api
    W, H = 200, 120
    s = copy.copy(settings)
    ctxs = [context(CORNELL, True, MIN) for _ in range(3)]
    try:
        whole, r0, r1 = ctxs
        r0.SetTileAssignment(0, 2, 64, 64); r1.SetTileAssignment(1, 2, 64, 64)
        for tb in ctxs:
            tb.Render(W, H, MIN + 1, s, 0.0)
        s.ConvergencePercentage = checked_threshold(state(whole), 0.5)
        for _ in range(3):
            for tb in ctxs:
                tb.Render(W, H, 2, s, 0.0)
            assert whole.GetOption("last_adaptive") == 1 and r0.GetOption("last_adaptive") == 1 and r1.GetOption("last_adaptive") == 1
            assert r0.LivePixels() + r1.LivePixels() == whole.LivePixels()
        packed = []
        for tb in (r0, r1):
            buf = torch.zeros((tb.OwnedPixels(W, H), 4), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            tb.PackOwnedTo(buf.data_ptr())
            packed.append(buf.cpu().numpy())
        assert same(api.unpack_gathered(W, H, 2, 64, 64, packed), state(whole)[0])
    finally:
        for tb in ctxs:
            tb.close()


def test_async_calls_give_the_synchronous_bits(settings):
    W, H = 64, 48
    s = copy.copy(settings)
    with context(CORNELL, True, MIN) as a, context(CORNELL, True, MIN) as b:
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        s.ConvergencePercentage = checked_threshold(state(a), 0.5)
        for n in (1, 3, 2, 5):
            a.Render(W, H, n, s, 0.0)
        for n in (1, 3, 2, 5):
            b.Render(W, H, n, s, 0.0, sync=False)
        b.Sync()
        assert b.GetOption("last_adaptive") == 1 and b.LivePixels() == a.LivePixels()
        assert same(state(a)[0], state(b)[0]) and same(state(a)[1], state(b)[1])


def test_adaptive_context_gives_back_every_device_byte(gpu_tb, settings):
    from tracerboy_amd import api
    before = gpu_tb.GetOption("debug_live_device_bytes")
    tb = api.TracerBoy(0)
    try:
        tb.LoadScene(CORNELL); tb.SetOption("adaptive", 1); tb.SetOption("adaptive_min_frames", 2)
        tb.Render(40, 24, 3, settings, 0.0); tb.Render(40, 24, 2, settings, 0.0)
        assert tb.GetOption("last_adaptive") == 1
        assert gpu_tb.GetOption("debug_live_device_bytes") > before
    finally:
        tb.close()
    assert gpu_tb.GetOption("debug_live_device_bytes") == before


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1]


def test_cli_schedule(tmp_path):
    from tracerboy_amd import api
    out = str(tmp_path / "x.pfm")
    W, H = 64, 48
    r = subprocess.run([CLI, CORNELL, "--width", str(W), "--height", str(H), "--spp", "4096", "--adaptive", "0.5", "--adaptive-after", "32",
                        "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [(int(f), int(l)) for f, l in re.findall(r"adaptive: (\d+) frames, (\d+) live pixels", r.stdout)]
    assert lines and lines[-1][1] == 0 and lines[-1][0] < 4096, r.stdout[-2000:]
    s = api.GetDefaultOutputSettings(); s.ConvergencePercentage = 0.5
    with context(CORNELL, True, 32) as tb:
        tb.Render(W, H, 33, s, 0.0)
        done = 33
        for frames, live in lines:
            tb.Render(W, H, frames - done, s, 0.0)
            done = frames
            assert tb.LivePixels() == live
        acc = tb.ReadAccumulation()
    w = acc[..., 3:4]
    with np.errstate(all="ignore"):
        rgb = acc[..., :3] * np.where(w > 0, np.float32(1.0) / w, np.float32(0.0))
    assert same(read_pfm(out), rgb)
