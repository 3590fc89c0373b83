"""-m gpu: adaptive sampling tested once per call (option "adaptive_test" = 1) -- a pixel that is live at a call's first frame
gets every frame of the call, a converged one none; the live pixels run through the frame-group kernels, driven by the live list (plan rule 8).

The prediction: a pixel that skips at a call's start keeps its sums, so it skips at every later start.  With S[0] a plain context's surfaces before
the first adaptive call and S[k] after the k-th, the adaptive context's surfaces after call k are frozen(S[:k + 1], thr) of
tests/test_adaptive_sampling.py: S[j] for a pixel whose test first held on S[j], S[k] elsewhere.  Every comparison is bit for bit, and every
threshold is taken from the data and checked to leave between 10 % and 90 % of the pixels live."""
import copy
import hashlib

import numpy as np
import pytest

from test_adaptive_sampling import CASES, MIN, TEAPOT, bits, checked_threshold, frozen, same, skips, state

pytestmark = pytest.mark.gpu
RULE_ADAPTIVE, RULE_ADAPTIVE_GROUPS = 7, 8
CALLS = (8, 8, 3, 1, 5)
PROC = ("procedural", 0, 200000, 1234)          # matte + environment, fetched from memory: the env set's occupancy copy
PW, PH = 256, 192


def context(scene, opts=None, adaptive=False, per_call=True, min_frames=MIN):
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    for k, v in (opts or {}).items():
        tb.SetOption(k, v)
    if isinstance(scene, tuple):
        tb.LoadProcedural(*scene[1:])
    else:
        tb.LoadScene(scene)
    if adaptive:
        tb.SetOption("adaptive", 1); tb.SetOption("adaptive_min_frames", min_frames); tb.SetOption("adaptive_test", 1 if per_call else 0)
    return tb


def warm_up(a, b, W, H, s):
    """Frames 0 .. MIN on both contexts -- b's call starts below the threshold and is plain -- and a threshold that leaves half of the pixels live."""
    a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
    S0 = state(a)
    assert b.GetOption("last_adaptive") == 0 and same(S0[0], state(b)[0]) and same(S0[1], state(b)[1])
    return S0


def run_calls(a, b, W, H, s, S, thr, owned=None):
    """CALLS on both contexts; after each, b against the prediction.  Returns (rule, frame group, copy waves) of b's calls."""
    ran = []
    for k, n in enumerate(CALLS):
        before = state(b)
        a.Render(W, H, n, s, 0.0); b.Render(W, H, n, s, 0.0)
        S.append(state(a))
        assert b.GetOption("last_adaptive") == 1, "call %d" % k
        ran.append((b.GetOption("last_plan_rule_pipeline"), b.GetOption("last_plan_frame_group"), b.GetOption("last_copy_waves")))
        live = ~skips(before, thr) if owned is None else ~skips(before, thr) & owned
        assert b.LivePixels() == int(live.sum()), "call %d" % k
        po, pq, _ = frozen(S, thr)
        if owned is not None:
            po = np.where(owned[..., None], po, 0).astype(np.float32); pq = np.where(owned[..., None], pq, 0).astype(np.float32)
        got = state(b)
        assert same(got[0], po) and same(got[1], pq), "call %d (%d frames): %d pixels differ from the prediction" % (
            k, n, int((bits(got[0]) != bits(po)).any(-1).sum() + (bits(got[1]) != bits(pq)).any(-1).sum()))
    return ran


def sequence(scene, W, H, depth, settings, opts=None, b_opts=None):
    s = copy.copy(settings); s.MaxBounces = depth
    with context(scene, opts) as a, context(scene, {**(opts or {}), **(b_opts or {})}, adaptive=True) as b:
        S = [warm_up(a, b, W, H, s)]
        plain_waves = b.GetOption("last_copy_waves")            # of b's own plain frame-group call
        thr = checked_threshold(S[0], 0.5)
        s.ConvergencePercentage = thr                           # (not a history-relevant setting: the sums go on)
        ran = run_calls(a, b, W, H, s, S, thr)
        return state(b), ran, plain_waves, b.GetOption("scene_in_lds_active")


def check_rules(ran, in_lds):
    for (rule, fg, _), n in zip(ran, CALLS):
        if n > 1 or in_lds:
            assert rule == RULE_ADAPTIVE_GROUPS and fg >= 1, (n, rule, fg)
        else:
            assert rule == RULE_ADAPTIVE, (n, rule)


def test_option_values():
    from tracerboy_amd import api
    from conftest import CORNELL
    with context(CORNELL) as tb:
        assert tb.GetOption("adaptive_test") == 0
        tb.SetOption("adaptive_test", 1)
        assert tb.GetOption("adaptive_test") == 1
        for bad in (2, -1):
            with pytest.raises(api.TracerBoyError) as e:
                tb.SetOption("adaptive_test", bad)
            assert e.value.code == -1 and tb.GetOption("adaptive_test") == 1
        tb.SetOption("adaptive_test", 0)
        assert tb.GetOption("adaptive_test") == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_calls_are_the_plain_render_frozen_at_call_starts(settings, case):
    scene, W, H, opts, depth = CASES[case]
    _, ran, _, in_lds = sequence(scene, W, H, depth, settings, opts)
    check_rules(ran, in_lds)


def test_scene_from_memory_in_the_occupancy_copy_small_groups_and_two_batches(settings):
    """200 k triangles fetched from memory: the occupancy copy runs, as in the plain frame-group call of the same context; the same surfaces with
    the group size forced to 2 and with a sample buffer so small that an 8-frame call is two batches."""
    got, ran, plain_waves, in_lds = sequence(PROC, PW, PH, 6, settings)
    assert not in_lds
    check_rules(ran, in_lds)
    assert plain_waves != 0
    for (rule, _, waves), n in zip(ran, CALLS):
        assert waves == (plain_waves if n > 1 else 0), (n, waves, plain_waves)
    small, ran2, _, _ = sequence(PROC, PW, PH, 6, settings, b_opts={"frame_group": 2})
    # (a forced group size forces the mode too, as in a plain call: the one-frame call is a frame-group call here)
    assert [fg for (_, fg, _) in ran2] == [2] * len(CALLS) and all(r == RULE_ADAPTIVE_GROUPS for r, _, _ in ran2)
    assert same(small[0], got[0]) and same(small[1], got[1])
    s = copy.copy(settings); s.MaxBounces = 6
    with context(PROC, {"pooled_samples": 4 * PW * PH}, adaptive=True) as b:   # four frames of samples: 8 frames = 4 + 4, 5 frames = 3 + 2
        b.Render(PW, PH, MIN + 1, s, 0.0)
        s.ConvergencePercentage = checked_threshold(state(b), 0.5)
        for n in CALLS:
            b.Render(PW, PH, n, s, 0.0)
            if n > 1:
                assert b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE_GROUPS and b.GetOption("last_kernel_frames") == {8: 4, 3: 3, 5: 3}[n]
        cut = state(b)
    assert same(cut[0], got[0]) and same(cut[1], got[1])


@pytest.mark.parametrize("case", ["cornell_200x120", "mix_glass_from_memory"])
def test_one_pixel_per_lane_kernel_gives_the_same_surfaces(settings, case):
    """frame_group = -1: rule 7, the per-frame kernel with its re-test switched off -- the semantics do not depend on the kernel that runs."""
    scene, W, H, opts, depth = CASES[case]
    groups, _, _, _ = sequence(scene, W, H, depth, settings, opts)
    dense, ran, _, _ = sequence(scene, W, H, depth, settings, opts, b_opts={"frame_group": -1})
    assert all(r == RULE_ADAPTIVE for r, _, _ in ran)
    assert same(groups[0], dense[0]) and same(groups[1], dense[1])


def test_aov_call_gives_the_same_surfaces_and_the_aovs_of_pixels_that_are_not_live(settings):
    from conftest import CORNELL
    W, H = 64, 48
    s = copy.copy(settings)
    groups, _, _, _ = sequence(CORNELL, W, H, 4, settings)
    with context(CORNELL, {"aov": 1}) as a, context(CORNELL, {"aov": 1}, adaptive=True) as b:
        S = [warm_up(a, b, W, H, s)]
        thr = checked_threshold(S[0], 0.5)
        s.ConvergencePercentage = thr
        one = np.array([0, 0, 0, 1], np.float32)
        for k, n in enumerate(CALLS):
            before, prev = state(b), {i: b.ReadAOV(i) for i in range(2, 8)}
            a.Render(W, H, n, s, 0.0); b.Render(W, H, n, s, 0.0)
            S.append(state(a))
            assert b.GetOption("last_adaptive") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE
            A, B = {i: a.ReadAOV(i) for i in range(2, 8)}, {i: b.ReadAOV(i) for i in range(2, 8)}
            dead = skips(before, thr)
            assert 0 < dead.sum() < dead.size
            # not live in the call: ClearAOVs, every other AOV as the pixel's last live sample left it; live: the plain call's AOVs
            assert same(B[2][dead], np.broadcast_to(one, B[2][dead].shape)) and same(B[5][dead], np.broadcast_to(one, B[5][dead].shape)), "call %d" % k
            for i in (3, 4, 6, 7):
                assert same(B[i][dead], prev[i][dead]), "call %d, AOV %d" % (k, i)
            for i in range(2, 8):
                assert same(B[i][~dead], A[i][~dead]), "call %d, AOV %d" % (k, i)
        got = state(b)
    assert same(got[0], groups[0]) and same(got[1], groups[1])


def test_per_frame_mode_is_untouched_by_the_option(settings):
    """adaptive_test = 0 set explicitly: the per-frame scenario of tests/test_adaptive_sampling.py (lanes retire inside a 7-frame call), same bits and
    rule as a context that never heard of the option."""
    from conftest import CORNELL
    W, H = 64, 48
    s = copy.copy(settings)
    with context(CORNELL) as a, context(CORNELL) as b, context(CORNELL, adaptive=True, per_call=False) as c:
        b.SetOption("adaptive", 1); b.SetOption("adaptive_min_frames", MIN)
        for tb in (a, b, c):
            tb.Render(W, H, MIN + 1, s, 0.0)
        S = [state(a)]
        thr = checked_threshold(S[0], 0.3)
        s.ConvergencePercentage = thr
        for _ in range(7):
            a.Render(W, H, 1, s, 0.0); S.append(state(a))
        b.Render(W, H, 7, s, 0.0); c.Render(W, H, 7, s, 0.0)
        assert b.GetOption("last_plan_rule_pipeline") == c.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE
        po, pq, first = frozen(S, thr)
        assert ((first >= 1) & (first <= 6)).sum() > 0
        for tb in (b, c):
            assert same(state(tb)[0], po) and same(state(tb)[1], pq)
        assert b.LivePixels() == c.LivePixels()


def test_call_that_starts_at_or_below_the_threshold_is_plain(settings):
    """... even if it ends above it -- where the per-frame mode's call is adaptive."""
    from conftest import CORNELL
    W, H = 64, 48
    s = copy.copy(settings); s.ConvergencePercentage = 0.5      # large: nearly every pixel would skip
    with context(CORNELL) as a, context(CORNELL, adaptive=True) as b, context(CORNELL, adaptive=True, per_call=False) as c:
        for n in (10, 7, 10):                                   # starts at frames 0, 10, 17 (= MIN + 1: the first call whose start is past the threshold)
            start = a.GetNumberOfSamplesSinceLastInvalidate()
            a.Render(W, H, n, s, 0.0); b.Render(W, H, n, s, 0.0); c.Render(W, H, n, s, 0.0)
            if start <= MIN:
                assert b.GetOption("last_adaptive") == 0 and b.LivePixels() == W * H
                for o in ("last_plan_rule_pipeline", "last_plan_frame_group", "last_plan_guided_groups", "last_copy_waves", "last_overlap"):
                    assert b.GetOption(o) == a.GetOption(o), o
                assert same(state(a)[0], state(b)[0]) and same(state(a)[1], state(b)[1])
            else:
                assert b.GetOption("last_adaptive") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE_GROUPS
            assert c.GetOption("last_adaptive") == (1 if start + n - 1 > MIN else 0)
        assert b.LivePixels() < W * H


def test_tile_rank_updates_only_its_pixels(settings):
    W, H = 200, 120
    s = copy.copy(settings)
    owned = np.zeros((H, W), bool)
    for t in range(8):                                          # 4 x 2 tiles of 64 x 64; rank 3 of 8 owns tile 3
        if t % 8 == 3:
            owned[(t // 4) * 64:(t // 4) * 64 + 64, (t % 4) * 64:(t % 4) * 64 + 64] = True
    # (Teapot: rank 3's tile is the frame's top right corner, where cornell-box sees nothing lit -- every pixel black -- and the procedural scene
    # the bare sky -- every error 0)
    with context(TEAPOT) as a, context(TEAPOT, adaptive=True) as b:
        b.SetTileAssignment(3, 8, 64, 64)
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        S = [state(a)]
        assert b.GetOption("last_adaptive") == 0 and b.LivePixels() == int(owned.sum()) == 8 * 64    # (the tile is cut by the frame's right edge)
        assert same(state(b)[0][owned], S[0][0][owned]) and not bits(state(b)[0])[~owned].any()
        thr = checked_threshold((S[0][0][owned], S[0][1][owned]), 0.5)
        s.ConvergencePercentage = thr
        ran = run_calls(a, b, W, H, s, S, thr, owned)
        check_rules(ran, b.GetOption("scene_in_lds_active"))


def test_every_pixel_dead_changes_no_byte(settings):
    from conftest import CORNELL
    W, H = 64, 48
    s = copy.copy(settings)
    with context(CORNELL, adaptive=True) as b:
        b.Render(W, H, MIN + 1, s, 0.0)
        before = state(b)
        s.ConvergencePercentage = 1e30
        assert skips(before, s.ConvergencePercentage).all()
        for n in (8, 1):
            b.Render(W, H, n, s, 0.0)
            assert b.GetOption("last_adaptive") == 1 and b.LivePixels() == 0
            assert same(state(b)[0], before[0]) and same(state(b)[1], before[1])
        assert b.GetNumberOfSamplesSinceLastInvalidate() == MIN + 10


def test_threshold_zero_drops_black_pixels_only(settings):
    from conftest import CORNELL
    s = copy.copy(settings)
    W, H = 64, 48
    # an environment-lit scene: no pixel is black (asserted), so the adaptive call is the plain frame-group call on every pixel
    with context(TEAPOT) as a, context(TEAPOT, adaptive=True) as b:
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        s.ConvergencePercentage = 0.0
        assert not skips(state(a), 0.0).any()
        a.Render(W, H, 8, s, 0.0); b.Render(W, H, 8, s, 0.0)
        assert b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE_GROUPS and b.LivePixels() == W * H
        assert same(state(a)[0], state(b)[0]) and same(state(a)[1], state(b)[1])
    # cornell-box: the pixels that see nothing lit are black and drop out, nothing else does
    s = copy.copy(settings); s.ConvergencePercentage = 0.0
    with context(CORNELL) as a, context(CORNELL, adaptive=True) as b:
        S = [warm_up(a, b, W, H, s)]
        black = skips(S[0], 0.0)
        assert 0 < black.sum() < black.size
        a.Render(W, H, 8, s, 0.0); b.Render(W, H, 8, s, 0.0)
        S.append(state(a))
        assert b.LivePixels() == int((~black).sum())
        po, pq, _ = frozen(S, 0.0)
        assert same(state(b)[0], po) and same(state(b)[1], pq)
        assert same(state(b)[0][~black], S[1][0][~black]) and same(state(b)[0][black], S[0][0][black])


def test_context_gives_back_every_device_byte(gpu_tb, settings):
    from conftest import CORNELL
    before = gpu_tb.GetOption("debug_live_device_bytes")
    s = copy.copy(settings); s.ConvergencePercentage = 0.01
    for scene, opts in ((CORNELL, None), (PROC, {"pooled_samples": 4 * 40 * 24})):
        tb = context(scene, opts, adaptive=True, min_frames=2)
        try:
            tb.Render(40, 24, 3, s, 0.0); tb.Render(40, 24, 8, s, 0.0); tb.Render(40, 24, 1, s, 0.0)
            assert tb.GetOption("last_adaptive") == 1
            assert gpu_tb.GetOption("debug_live_device_bytes") > before
        finally:
            tb.close()
        assert gpu_tb.GetOption("debug_live_device_bytes") == before


@pytest.mark.parametrize("which", ["cornell_200x120", "from_memory"])
def test_ten_renders_one_digest(settings, which):
    """The order in which workgroups claim list blocks must not reach the picture: ten renders from frame 0, one digest.  A differing digest fails at
    once; nothing is run again."""
    scene, W, H, opts, depth = CASES[which] if which in CASES else (PROC, PW, PH, {}, 6)
    s = copy.copy(settings); s.MaxBounces = depth
    digests = []
    with context(scene, opts, adaptive=True) as b:
        thr = None
        for _ in range(10):
            b.InvalidateHistory()
            s.ConvergencePercentage = 0.0
            b.Render(W, H, MIN + 1, s, 0.0)
            if thr is None:
                thr = checked_threshold(state(b), 0.5)
            s.ConvergencePercentage = thr
            for n in CALLS:
                b.Render(W, H, n, s, 0.0)
            assert b.GetOption("last_adaptive") == 1
            o, q = state(b)
            digests.append(hashlib.sha1(bits(o).tobytes() + bits(q).tobytes()).hexdigest())
            assert digests[-1] == digests[0], "render %d differs from render 0" % (len(digests) - 1)
    assert len(digests) == 10


def test_cli_adaptive_test_call(tmp_path):
    """--adaptive-test call: the CLI's schedule with the option set -- its progress lines and its picture are those of the same calls through the
    API; an unknown value is refused before anything is rendered."""
    import re
    import subprocess
    from conftest import CORNELL
    from tracerboy_amd import api
    from test_adaptive_sampling import CLI, read_pfm
    out = str(tmp_path / "x.pfm")
    W, H = 64, 48
    args = [CLI, CORNELL, "--width", str(W), "--height", str(H), "--spp", "4096", "--adaptive", "0.5", "--adaptive-after", "32", "--out", out]
    r = subprocess.run(args + ["--adaptive-test", "sometimes"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "frame or call" in r.stderr
    r = subprocess.run(args + ["--adaptive-test", "call"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [(int(f), int(l)) for f, l in re.findall(r"adaptive: (\d+) frames, (\d+) live pixels", r.stdout)]
    assert lines and lines[-1][1] == 0 and lines[-1][0] < 4096, r.stdout[-2000:]
    s = api.GetDefaultOutputSettings(); s.ConvergencePercentage = 0.5
    with context(CORNELL, adaptive=True, min_frames=32) as tb:
        tb.Render(W, H, 33, s, 0.0)
        done = 33
        for frames, live in lines:
            tb.Render(W, H, frames - done, s, 0.0)
            done = frames
            assert tb.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE_GROUPS and tb.LivePixels() == live
        acc = tb.ReadAccumulation()
    w = acc[..., 3:4]
    with np.errstate(all="ignore"):
        rgb = acc[..., :3] * np.where(w > 0, np.float32(1.0) / w, np.float32(0.0))
    assert same(read_pfm(out), rgb)
