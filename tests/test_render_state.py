"""-m gpu: render states.  A render that is saved, loaded into a NEW context and continued has the bits of the render that was
never interrupted and of the oracle; states of adjacent frame ranges add up to the float32 sum of the oracle's partial sums; the device digest
is the host digest; whatever does not fit is refused with a code; whatever resets the history still does."""
import copy
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from conftest import CORNELL, GOLDEN, ROOT
from test_render_state_host import default_info, np_digest, payload

pytestmark = pytest.mark.gpu
MIX = os.path.join(GOLDEN, "scenes", "mix-glass", "scene.pbrt")
CLI = os.path.join(ROOT, "tracerboy_amd", "tracerboy-hip")
W, H = 70, 50                                                   # ragged against 8, 16 and 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def state(tb):
    return tb.ReadAccumulation(jittered=True)


def same_state(a, b):
    return same(a[0], b[0]) and same(a[1], b[1])


def context(scene=CORNELL, opts=None, **kw):
    from tracerboy_amd import api
    tb = api.TracerBoy(**kw)
    for k, v in (opts or {}).items():
        tb.SetOption(k, v)
    tb.LoadScene(scene)
    return tb


class Oracle:
    """The oracle's sums of frame ranges of one scene, each computed once: part(first, n) on zeroed surfaces, on(first, n, state) continuing a state."""

    def __init__(self, scene, settings, depth=4):
        from tracerboy_amd import api
        self.host = api.HostScene(scene)
        self.s = copy.copy(settings); self.s.MaxBounces = depth
        self.view, self.pf = self.host.view(), self.host.frame_constants(self.s, 0, 0.0)
        self.memo = {}

    def on(self, first, n, st, w=W, h=H):
        out, jit = st[0].copy(), st[1].copy()
        ol.render(self.view, self.pf, w, h, n, first_frame=first, threads=8, jittered=True, out=out, jit=jit)
        return out, jit

    def part(self, first, n, w=W, h=H):
        key = (first, n, w, h)
        if key not in self.memo:
            z = np.zeros((h, w, 4), np.float32)
            self.memo[key] = self.on(first, n, (z, z), w, h)
        return self.memo[key]


@pytest.fixture(scope="module")
def cornell(built, settings):
    return Oracle(CORNELL, settings)


def addends(n_words, seed):
    """float32 words without NaN or infinity whose sums round, cancel, stay denormal and keep or lose the sign of zero."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n_words) * np.exp2(rng.integers(-20, 20, n_words))).astype(np.float32)
    special = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000003, 0x007fffff, 0x00800000, 0x80800001, 0x3f800001], np.uint32).view(np.float32)
    k = min(n_words, special.size)
    a[rng.permutation(n_words)[:k]] = special[rng.permutation(special.size)[:k]]
    return a


# ---- device digest = host digest, and state_add -----------------------------------------------------------------------------------------
# (1024, 513): 525 312 vectors, 1024 over the kernels' grid of 2048 workgroups x 256 lanes = 524 288 -- the digest's remainder loop takes a second
# turn for 1024 lanes, state_add_kernel's paired loop runs for those and leaves a single add to every other lane.  The condition: w * h > 524 288.
@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (17, 1), (64, 1), (65, 1), (70, 50), (1024, 513)])
def test_device_digest_is_the_host_digest_and_add_is_float32_addition(built, settings, tmp_path, w, h):
    from tracerboy_amd import api
    with context() as tb:
        cam = tb.GetCamera()
        def write(name, first, nxt, out, jit):
            info = default_info(first=first, next_frame=nxt, scene_digest=tb.SceneDigest(), settings=settings, camera=cam)
            api.WriteStateFile(str(tmp_path / name), info, out, jit)
            return str(tmp_path / name)
        out, jit = payload(w * h * 4, 21).reshape(h, w, 4), payload(w * h * 4, 22).reshape(h, w, 4)     # NaN payloads, infinities, -0, denormals
        tb.LoadState(write("p.tbs", 2, 5, out, jit))
        assert tb.AccumDigest() == (np_digest(out), np_digest(jit)) == (api.StateDigest(out), api.StateDigest(jit))
        assert same_state(state(tb), (out, jit))
        assert (tb.GetOption("state_first_frame"), tb.GetNumberOfSamplesSinceLastInvalidate()) == (2, 5)
        a = addends(w * h * 4, 31).reshape(h, w, 4), addends(w * h * 4, 32).reshape(h, w, 4)
        b = addends(w * h * 4, 33).reshape(h, w, 4), addends(w * h * 4, 34).reshape(h, w, 4)
        b[0].ravel()[0] = -a[0].ravel()[0]                      # x + (-x) = +0
        tb.LoadState(write("a.tbs", 2, 5, *a))
        append = w % 2 == 1
        tb.LoadState(write("b.tbs", *((5, 9) if append else (0, 2)), *b), add=True)
        want = a[0] + b[0], a[1] + b[1]                         # numpy float32: IEEE additions, denormals kept
        assert same_state(state(tb), want)
        assert tb.AccumDigest() == (np_digest(want[0]), np_digest(want[1]))
        assert (tb.GetOption("state_first_frame"), tb.GetNumberOfSamplesSinceLastInvalidate()) == ((2, 9) if append else (0, 5))


def test_device_digest_in_the_unrolled_loop(built, settings, tmp_path):
    """state_digest_partials keeps four loads in flight while v + 3 * stride < nVec, stride = 524 288 vectors: the condition on the frame is
    w * h > 3 * 524 288 = 1 572 864.  2048 x 769 = 1 574 912 is 2048 over it: the first 2048 lanes take one turn of the unrolled loop, every other
    lane three turns of the remainder loop.  Digest only (one file of 50 MB); the sums of this size are the test above's."""
    from tracerboy_amd import api
    w, h = 2048, 769
    assert w * h > 3 * 2048 * 256
    with context() as tb:
        info = default_info(first=2, next_frame=5, scene_digest=tb.SceneDigest(), settings=settings, camera=tb.GetCamera())
        out, jit = payload(w * h * 4, 41).reshape(h, w, 4), payload(w * h * 4, 42).reshape(h, w, 4)
        api.WriteStateFile(str(tmp_path / "big.tbs"), info, out, jit)
        tb.LoadState(str(tmp_path / "big.tbs"))
        assert tb.AccumDigest() == (np_digest(out), np_digest(jit)) == (api.StateDigest(out), api.StateDigest(jit))
        assert same_state(state(tb), (out, jit))


# ---- resume exactness -------------------------------------------------------------------------------------------------------------------
def resumed_and_uninterrupted(scene, s, w, h, n1, n2, opts, tmp_path):
    path = str(tmp_path / "resume.tbs")
    with context(scene, opts) as a:
        a.Render(w, h, n1, s, 0.0)
        a.SaveState(path)
    with context(scene, opts) as b:                             # a new context: nothing but the file carries the render over
        b.LoadState(path)
        b.Render(w, h, n2, s, 0.0)
        got, frames = state(b), b.GetNumberOfSamplesSinceLastInvalidate()
    with context(scene, opts) as c:
        c.Render(w, h, n1, s, 0.0); c.Render(w, h, n2, s, 0.0)
        straight = state(c)
    return got, frames, straight


@pytest.mark.parametrize("split", [(3, 2), (1, 4)])
@pytest.mark.parametrize("frame_group", [-1, 0, 2])
def test_resumed_render_is_the_uninterrupted_render_and_the_oracle(cornell, tmp_path, frame_group, split):
    got, frames, straight = resumed_and_uninterrupted(CORNELL, cornell.s, W, H, split[0], split[1], {"frame_group": frame_group}, tmp_path)
    assert frames == 5
    assert same_state(got, straight), "resumed differs from the uninterrupted render"
    assert same_state(got, cornell.part(0, 5)), "resumed differs from the oracle's 5 frames"


def test_resumed_render_with_interior_walks(built, settings, tmp_path):
    mix = Oracle(MIX, settings, depth=6)
    got, frames, straight = resumed_and_uninterrupted(MIX, mix.s, 64, 48, 3, 2, {}, tmp_path)
    assert frames == 5 and same_state(got, straight) and same_state(got, mix.part(0, 5, 64, 48))


# ---- resume with adaptive sampling ------------------------------------------------------------------------------------------------------
def skip_test(o, q, thr):
    """DESIGN.md section 10 (tests/test_adaptive_sampling.py): black, or ((|dr| + |dg|) + |db|) / sqrt((c.r + c.g) + c.b) < thr."""
    with np.errstate(all="ignore"):
        c = o[..., :3] / o[..., 3:4]
        j = q[..., :3] / q[..., 3:4]
        black = (c[..., 0] <= 0) & (c[..., 1] <= 0) & (c[..., 2] <= 0)
        err = ((np.abs(j[..., 0] - c[..., 0]) + np.abs(j[..., 1] - c[..., 1])) + np.abs(j[..., 2] - c[..., 2])) / np.sqrt((c[..., 0] + c[..., 1]) + c[..., 2])
        return black, err, black | (err < np.float32(thr))


def checked_threshold(st, share):
    black, err, _ = skip_test(st[0], st[1], 0.0)
    e = np.sort(err[~black & np.isfinite(err)])
    thr = float(np.float32(e[min(len(e) - 1, int(len(e) * share))]))
    live = 1.0 - skip_test(st[0], st[1], thr)[2].mean()
    assert 0.1 <= live <= 0.9, "threshold %g leaves %.1f %% of the pixels live" % (thr, 100 * live)
    return thr


@pytest.mark.parametrize("adaptive_test", [0, 1])
def test_resumed_adaptive_render_is_the_uninterrupted_one(built, settings, tmp_path, adaptive_test):
    MIN, w, h = 16, 64, 48
    opts = {"adaptive": 1, "adaptive_min_frames": MIN, "adaptive_test": adaptive_test}
    s = copy.copy(settings)
    path = str(tmp_path / "adaptive.tbs")
    with context(opts=opts) as a, context(opts=opts) as c:
        a.Render(w, h, MIN + 1, s, 0.0); c.Render(w, h, MIN + 1, s, 0.0)        # the plain call: no pixel can skip yet
        assert a.GetOption("last_adaptive") == 0
        s.ConvergencePercentage = checked_threshold(state(a), 0.5)
        a.Render(w, h, 2, s, 0.0); c.Render(w, h, 2, s, 0.0)
        assert a.GetOption("last_adaptive") == 1 and 0.1 * w * h <= a.LivePixels() <= 0.9 * w * h
        a.SaveState(path)
        c.Render(w, h, 3, s, 0.0)
        straight, live = state(c), c.LivePixels()
    with context(opts=opts) as b:
        b.LoadState(path)
        b.Render(w, h, 3, s, 0.0)
        assert b.GetOption("last_adaptive") == 1
        assert same_state(state(b), straight)
        assert b.LivePixels() == live and 0 < live < w * h
        assert b.GetNumberOfSamplesSinceLastInvalidate() == MIN + 6
    with context(opts={"adaptive": 1, "adaptive_min_frames": MIN + 1, "adaptive_test": adaptive_test}) as d:
        from tracerboy_amd import api
        with pytest.raises(api.TracerBoyError) as e:            # the four result-changing options are part of the state
            d.LoadState(path)
        assert e.value.code == -1 and "adaptive_min_frames" in str(e.value)


# ---- frame ranges and merge -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_parts(cornell, tmp_path_factory):
    """[0, 3) and [3, 5) of cornell-box saved from two contexts."""
    d = tmp_path_factory.mktemp("parts")
    a, b = str(d / "a.tbs"), str(d / "b.tbs")
    with context() as x:
        x.Render(W, H, 3, cornell.s, 0.0); x.SaveState(a)
    with context() as y:
        y.BeginAccumulation(W, H, cornell.s, 0.0, first_frame=3)
        assert (y.GetOption("state_first_frame"), y.GetNumberOfSamplesSinceLastInvalidate()) == (3, 3)
        y.Render(W, H, 2, cornell.s, 0.0)
        assert same_state(state(y), cornell.part(3, 2)), "frames 3, 4 on zeroed surfaces"
        assert (y.GetOption("state_first_frame"), y.GetNumberOfSamplesSinceLastInvalidate()) == (3, 5)
        y.SaveState(b)
    return a, b


def test_begin_at_a_frame_and_merge(cornell, two_parts):
    from tracerboy_amd import api
    a, b = two_parts
    pa, pb = cornell.part(0, 3), cornell.part(3, 2)
    merged = pa[0] + pb[0], pa[1] + pb[1]                       # the float32 sum of the partial sums, not the straight render's bits
    ia, ib = api.StateInfo(a), api.StateInfo(b)
    assert (ia.first_frame, ia.next_frame, ib.first_frame, ib.next_frame) == (0, 3, 3, 5)
    assert (ia.output_digest, ia.jittered_digest) == (np_digest(pa[0]), np_digest(pa[1]))
    assert ia.scene_digest == ib.scene_digest == cornell.host.digest()
    for first, second in ((a, b), (b, a)):                      # append, prepend
        with context() as tb:
            tb.LoadState(first); tb.LoadState(second, add=True)
            got = state(tb)
            assert same_state(got, merged)
            assert np.all(got[0][..., 3] == 5.0)                # box filter: the output's sum of 1.0 is exact (the jittered surface takes a share of the frames)
            assert (tb.GetOption("state_first_frame"), tb.GetNumberOfSamplesSinceLastInvalidate()) == (0, 5)
            tb.Render(W, H, 1, cornell.s, 0.0)                  # frame 5
            assert same_state(state(tb), cornell.on(5, 1, merged)) and tb.GetNumberOfSamplesSinceLastInvalidate() == 6


def test_refusals(cornell, two_parts, tmp_path):
    from tracerboy_amd import api
    a, b = two_parts
    info, out, jit = api.ReadStateFile(b)

    def variant(name, **kw):
        h = copy.copy(info)
        for k, v in kw.items():
            setattr(h, k, v)
        api.WriteStateFile(str(tmp_path / name), h, out, jit)
        return str(tmp_path / name)

    def refused(tb, path, word, code=-1, **kw):
        with pytest.raises(api.TracerBoyError) as e:
            tb.LoadState(path, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    other_settings = copy.copy(info.settings); other_settings.MaxBounces = 3
    other_camera = copy.copy(info.camera); other_camera.Position[0] += 0.25
    with context() as tb:
        with pytest.raises(api.TracerBoyError) as e:            # nothing rendered
            tb.SaveState(str(tmp_path / "none.tbs"))
        assert e.value.code == -1
        refused(tb, b, "TB_STATE_ADD", add=True)                # no state to add to
        refused(tb, str(tmp_path / "missing.tbs"), "open", code=-3)
        tb.LoadState(a)
        held = state(tb)
        refused(tb, a, "overlap", add=True)
        refused(tb, variant("gap.tbs", first_frame=4, next_frame=6), "gap", add=True)
        refused(tb, variant("settings.tbs", settings=other_settings), "settings", add=True)
        refused(tb, variant("seed.tbs", time_seed=1.0), "time_seed", add=True)
        refused(tb, variant("camera.tbs", camera=other_camera), "camera", add=True)
        refused(tb, variant("scene.tbs", scene_digest=info.scene_digest ^ 1), "scene_digest", add=True)
        refused(tb, variant("scene.tbs", scene_digest=info.scene_digest ^ 1), "scene_digest")
        refused(tb, variant("part.tbs", tile_rank=1, tile_world=2), "tile assignment", add=True)
        refused(tb, variant("alpha.tbs", alpha_test=1), "alpha_test")
        refused(tb, variant("seed2.tbs", time_seed=1.0, scene_digest=info.scene_digest ^ 1), "time_seed", add=True, any_scene=True)  # only the scene check
        assert same_state(state(tb), held) and tb.GetNumberOfSamplesSinceLastInvalidate() == 3         # a refusal leaves the state alone
        tb.LoadState(variant("scene.tbs", scene_digest=info.scene_digest ^ 1), add=True, any_scene=True)
        assert tb.GetNumberOfSamplesSinceLastInvalidate() == 5
        # a material edit makes it another scene (and forgets the frames, as it always did)
        m = tb.GetMaterial(0); m.albedo.x = 0.25; tb.SetMaterial(0, m)
        assert tb.SceneDigest() != info.scene_digest and tb.GetNumberOfSamplesSinceLastInvalidate() == 0
        refused(tb, a, "scene_digest")
        refused(tb, a, "scene_digest", add=True)
        tb.LoadState(a, any_scene=True)
        assert same_state(state(tb), held)
        # the real-time chain's surface is no accumulation
        tb.RenderRealTime(W, H, cornell.s, None, 0.0)
        with pytest.raises(api.TracerBoyError) as e:
            tb.SaveState(str(tmp_path / "rt.tbs"))
        assert e.value.code == -1 and "realtime" in str(e.value)
    with context() as tb:                                       # another size
        tb.Render(W + 1, H, 1, cornell.s, 0.0)
        refused(tb, a, "width / height", add=True)


# ---- groups and ranks -------------------------------------------------------------------------------------------------------------------
def owned_mask(w, h, rank, world, tile=64):
    ty, tx = np.meshgrid(np.arange(h) // tile, np.arange(w) // tile, indexing="ij")
    return (ty * ((w + tile - 1) // tile) + tx) % world == rank


def test_groups_and_ranks(cornell, tmp_path):
    w, h = 200, 136
    s = cornell.s
    single, group, part = str(tmp_path / "single.tbs"), str(tmp_path / "group.tbs"), str(tmp_path / "part.tbs")
    o3, o5 = cornell.part(0, 3, w, h), cornell.part(0, 5, w, h)
    with context() as tb:
        tb.Render(w, h, 3, s, 0.0); tb.SaveState(single)
    with context(devices=[0, 0]) as g:                          # a complete state into a group: every member gets the surfaces and its tile map
        g.LoadState(single)
        g.Render(w, h, 2, s, 0.0)
        assert g.GetNumberOfSamplesSinceLastInvalidate() == 5 and same_state(state(g), o5)
        g.SaveState(group)
    from tracerboy_amd import api
    assert api.StateInfo(group).tile_world == 1
    with context() as tb:                                       # and the group's into a single context
        tb.LoadState(group)
        tb.Render(w, h, 1, s, 0.0)
        assert same_state(state(tb), cornell.on(5, 1, o5, w, h))
    mine = owned_mask(w, h, 1, 2)
    with context() as r:                                        # a rank's partial frame
        r.SetTileAssignment(1, 2)
        r.Render(w, h, 3, s, 0.0); r.SaveState(part)
        assert api.StateInfo(part).tile_world == 2
    for assign in (None, (0, 2), (1, 3)):
        with context() as x:
            if assign:
                x.SetTileAssignment(*assign)
            with pytest.raises(api.TracerBoyError) as e:
                x.LoadState(part)
            assert e.value.code == -1 and "tile assignment" in str(e.value)
    with context(devices=[0, 0]) as g:
        with pytest.raises(api.TracerBoyError) as e:
            g.LoadState(part)
        assert e.value.code == -1
    with context() as r:
        r.SetTileAssignment(1, 2)
        r.LoadState(part)
        r.Render(w, h, 2, s, 0.0)
        got = state(r)
        assert r.GetNumberOfSamplesSinceLastInvalidate() == 5
        assert same(got[0][mine], o5[0][mine]) and same(got[1][mine], o5[1][mine]) and not got[0][~mine].any()
    with context() as r:                                        # a complete frame into a rank: only its own tiles go on
        r.SetTileAssignment(1, 2)
        r.LoadState(single)
        r.Render(w, h, 2, s, 0.0)
        got = state(r)
        assert same(got[0][mine], o5[0][mine]) and same(got[0][~mine], o3[0][~mine]) and same(got[1][mine], o5[1][mine])


# ---- history resets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", ["size", "settings", "invalidate", "camera"])
def test_history_resets_after_a_load_return_to_frame_zero(cornell, two_parts, settings, reset):
    with context() as tb:
        tb.LoadState(two_parts[1])                              # frames [3, 5)
        assert tb.GetOption("state_first_frame") == 3
        s, w, h, ref = cornell.s, W, H, cornell
        if reset == "size":
            w, h = 64, 48
        elif reset == "settings":
            ref = Oracle(CORNELL, settings, depth=3); s = ref.s
        elif reset == "invalidate":
            tb.InvalidateHistory()
        else:
            tb.SetCamera(tb.GetCamera())
        tb.Render(w, h, 1, s, 0.0)
        assert (tb.GetOption("state_first_frame"), tb.GetNumberOfSamplesSinceLastInvalidate()) == (0, 1)
        assert same_state(state(tb), ref.part(0, 1, w, h)), "frame 0 after a history reset (%s)" % reset


# ---- device memory ----------------------------------------------------------------------------------------------------------------------
def test_save_load_and_add_give_back_everything(gpu_tb, cornell, two_parts, tmp_path):
    from tracerboy_amd import api
    before = gpu_tb.GetOption("debug_live_device_bytes")
    with context() as tb:
        tb.Render(W, H, 3, cornell.s, 0.0)
        tb.SaveState(str(tmp_path / "m.tbs"))
        tb.LoadState(str(tmp_path / "m.tbs"))
        held = gpu_tb.GetOption("debug_live_device_bytes")
        tb.LoadState(two_parts[1], add=True)
        assert gpu_tb.GetOption("debug_live_device_bytes") == held, "the file's copies on the device outlive the addition"
        tb.AccumDigest()
        with pytest.raises(api.TracerBoyError):
            tb.LoadState(two_parts[1], add=True)
    with context() as tb:
        tb.BeginAccumulation(W, H, cornell.s, 0.0, first_frame=3)
        tb.LoadState(two_parts[1], add=True)                    # onto the empty state [3, 3)
        assert same_state(state(tb), cornell.part(3, 2))
    assert gpu_tb.GetOption("debug_live_device_bytes") == before


# ---- the command-line tool --------------------------------------------------------------------------------------------------------------
def run_cli(*args, status=0):
    r = subprocess.run([CLI, CORNELL, "--width", str(W), "--height", str(H), "--depth", "4", "--blue-noise", "0"] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == status, r.stdout + r.stderr
    return r


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = [int(x) for x in f.readline().split()]
        assert float(f.readline()) < 0                          # little endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1]


def test_cli_resume_is_byte_identical(built, tmp_path):
    a, b, st = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm"), str(tmp_path / "s.tbs")
    run_cli("--spp", 5, "--out", a)
    run_cli("--spp", 3, "--save-state", st, "--out", str(tmp_path / "three.pfm"))
    run_cli("--resume", st, "--spp", 5, "--out", b)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_cli_frame_ranges_merge(built, tmp_path):
    from tracerboy_amd import api
    p, q, out = str(tmp_path / "p.tbs"), str(tmp_path / "q.tbs"), str(tmp_path / "m.pfm")
    run_cli("--frames", "0:3", "--save-state", p, "--out", str(tmp_path / "p.pfm"))
    run_cli("--frames", "3:5", "--save-state", q, "--out", str(tmp_path / "q.pfm"))
    run_cli("--resume", p, "--add", q, "--out", out)
    ip, op, _ = api.ReadStateFile(p); iq, oq, _ = api.ReadStateFile(q)
    assert (ip.first_frame, ip.next_frame, iq.first_frame, iq.next_frame) == (0, 3, 3, 5)
    merged = op + oq
    assert np.all(merged[..., 3] == 5.0)
    want = merged[..., :3] * (np.float32(1.0) / merged[..., 3:4])
    assert same(read_pfm(out), want)


def test_cli_checkpoints_and_refuses_ranks(built, tmp_path):
    from tracerboy_amd import api
    st = str(tmp_path / "c.tbs")
    run_cli("--spp", 5, "--checkpoint-every", 2, "--save-state", st, "--out", str(tmp_path / "c.pfm"))
    info = api.StateInfo(st)
    assert (info.first_frame, info.next_frame) == (0, 5)
    api.ReadStateFile(st)                                       # loadable: digests hold
    assert sorted(os.listdir(tmp_path)) == ["c.pfm", "c.tbs"]
    r = run_cli("--spp", 2, "--ranks", 2, "--save-state", str(tmp_path / "r.tbs"), status=2)
    assert "--ranks" in r.stderr and not os.path.exists(str(tmp_path / "r.tbs"))
