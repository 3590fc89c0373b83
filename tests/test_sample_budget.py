"""Sample budgets: a per-pixel frame index at which the pixel stops receiving samples, the live list's second source.

The invariant every GPU test here checks bit for bit: a pixel's sums are the plain render's at a call boundary -- the last call that started below
its budget -- and exact zeros where no call did.  The plain renders the pictures are composed from are computed once per (scene, size, calls)
and compared with the oracle where the issue asks for it; tests/sample_budget_ref.py holds the NumPy restatement."""
import copy
import ctypes as C

import numpy as np
import pytest

import sample_budget_ref as ref
from conftest import CORNELL
from sample_budget_ref import NEVER
from test_adaptive_sampling import INSTANCES, bits, checked_threshold, same, skips, state

RULE_ADAPTIVE, RULE_ADAPTIVE_GROUPS = 7, 8
TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6
PROC = ("procedural", 0, 3000, 1234)                            # a few thousand triangles: fetched from memory
SCENES = {"cornell": (CORNELL, {}), "from_memory": (PROC, {"scene_in_lds": 0}), "two_level": (INSTANCES, {"flatten_instances": 0})}
_plain = {}


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------
def test_reference_self_checks():
    assert ref.self_check()


def test_null_context_and_declarations(built):
    from tracerboy_amd import api
    L = api.lib()
    b = (C.c_uint32 * 4)()
    assert L.tb_set_sample_budget(None, 2, 2, b) != 0 and L.tb_read_sample_budget(None, b) != 0
    assert L.tb_budget_stop_converged(None, 0.1, 4, None, None) != 0
    for name in ("tb_set_sample_budget", "tb_read_sample_budget", "tb_budget_stop_converged", "tb_run_budget_stop"):
        assert name in L._tb_exports
    for name in ("SetSampleBudget", "SampleBudget", "StopConverged", "RunBudgetStop"):
        assert hasattr(api.TracerBoy, name)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def depth3(settings):
    s = copy.copy(settings); s.MaxBounces = 3
    return s


def context(scene="cornell", opts=None):
    from tracerboy_amd import api
    path, own = SCENES[scene]
    tb = api.TracerBoy(0)
    for k, v in {**own, **(opts or {})}.items():
        tb.SetOption(k, v)
    if isinstance(path, tuple):
        tb.LoadProcedural(*path[1:])
    else:
        tb.LoadScene(path)
    return tb


def plain_states(scene, W, H, calls, s):
    """[(zeros, zeros), the plain render's surfaces after each call] -- computed once, read only."""
    key = (scene, W, H, tuple(calls))
    if key not in _plain:
        states = [(np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32))]
        with context(scene) as a:
            for n in calls:
                a.Render(W, H, n, s, 0.0)
                assert a.GetOption("last_adaptive") == 0 and a.GetOption("last_budgeted") == 0
                states.append(state(a))
        for o, q in states:
            o.setflags(write=False); q.setflags(write=False)
        _plain[key] = states
    return _plain[key]


def differing(got, want):
    return int(((bits(got[0]) != bits(want[0])) | (bits(got[1]) != bits(want[1]))).any(-1).sum())


def budgeted_sequence(scene, W, H, calls, s, budget, opts=None, rule=None, in_lds=None):
    """The calls under the budget; after each: the live count and the prediction.  Returns the final surfaces."""
    states = plain_states(scene, W, H, calls, s)
    with context(scene, opts) as b:
        b.SetSampleBudget(budget)
        assert b.GetOption("budget_set") == 1 and same(b.SampleBudget(), budget)
        start = 0
        for i, n in enumerate(calls):
            b.Render(W, H, n, s, 0.0)
            assert b.GetOption("last_budgeted") == 1 and b.GetOption("last_adaptive") == 1, "call %d" % i
            if rule is not None:
                want_rule = rule if rule == RULE_ADAPTIVE or n > 1 or b.GetOption("scene_in_lds_active") else RULE_ADAPTIVE
                assert b.GetOption("last_plan_rule_pipeline") == want_rule, (i, b.GetOption("last_plan_rule_pipeline"))
            assert b.LivePixels() == int(ref.live(budget, start).sum()), "call %d" % i
            start += n
            want = ref.compose(states[:i + 2], ref.frames_held(budget, calls[:i + 1]))
            got = state(b)
            assert differing(got, want) == 0, "call %d: %d pixels differ from the plain render at their call boundary" % (i, differing(got, want))
        assert b.GetNumberOfSamplesSinceLastInvalidate() == sum(calls)
        if in_lds is not None:
            assert b.GetOption("scene_in_lds_active") == in_lds
        return state(b)


FORMS = {"rule_8": ({}, RULE_ADAPTIVE_GROUPS), "rule_7": ({"frame_group": -1}, RULE_ADAPTIVE)}


# ---- the invariant ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plain_references_equal_the_oracle(settings):
    """The plain renders the pictures below are composed from, whole frame, both surfaces, at 4 and 12 frames."""
    import oracle_lib as ol
    s = depth3(settings)
    W, H = 100, 70
    states = plain_states("cornell", W, H, (4, 4, 4), s)
    with context("cornell") as tb:
        view, pf = tb.HostSceneView(), tb.FrameConstants(W, H, 0, s, 0.0)
        for k, frames in ((1, 4), (3, 12)):
            cpu = ol.render(view, pf, W, H, frames, threads=8, jittered=True)
            assert same(states[k][0], cpu["output"]) and same(states[k][1], cpu["jittered"]), frames


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_pixels_hold_the_plain_render_at_their_call_boundary(settings, form):
    """100 x 70, ragged against the 16 x 16 regions and the 256-entry list blocks, three calls of 4 frames: budget b holds min(12, 4 ceil(b / 4))
    frames on both surfaces, budget 0 exact zeros."""
    opts, rule = FORMS[form]
    W, H = 100, 70
    budget = ref.layout(W, H)
    ref.check_layout(budget, W, H)
    got = budgeted_sequence("cornell", W, H, (4, 4, 4), depth3(settings), budget, opts, rule, in_lds=1)
    assert not bits(got[0])[budget == 0].any() and not bits(got[1])[budget == 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_one_frame_calls_make_budgets_exact(settings, form):
    opts, rule = FORMS[form]
    W, H = 20, 12
    budget = ref.layout(W, H)
    ref.check_layout(budget, W, H, whole_regions=False)
    got = budgeted_sequence("cornell", W, H, (1,) * 10, depth3(settings), budget, opts, rule)
    want_w = np.minimum(budget.astype(np.uint64), 10).astype(np.float32)     # box filter: every sample weighs 1
    assert np.array_equal(got[0][..., 3], want_w)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("scene", ["from_memory", "two_level"])
def test_scenes_fetched_from_memory_and_two_level(settings, scene, form):
    opts, rule = FORMS[form]
    W, H = 52, 36
    budget = ref.layout(W, H, seed=5)
    budgeted_sequence(scene, W, H, (4, 4, 4), depth3(settings), budget, opts, rule, in_lds=0)


@pytest.mark.gpu
def test_aov_call_and_the_aovs_of_pixels_that_are_not_live(settings):
    s = depth3(settings)
    W, H = 40, 24
    budget = ref.layout(W, H, seed=3)
    one = np.array([0, 0, 0, 1], np.float32)
    with context("cornell", {"aov": 1}) as a, context("cornell", {"aov": 1}) as b:
        b.SetSampleBudget(budget)
        S = [(np.zeros((H, W, 4), np.float32),) * 2]
        for i, n in enumerate((4, 4, 4)):
            prev = {k: b.ReadAOV(k) for k in range(2, 8)} if i else None
            a.Render(W, H, n, s, 0.0); b.Render(W, H, n, s, 0.0)
            S.append(state(a))
            assert b.GetOption("last_budgeted") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE
            dead = ~ref.live(budget, 4 * i)
            assert 0 < dead.sum() < dead.size
            A, B = {k: a.ReadAOV(k) for k in range(2, 8)}, {k: b.ReadAOV(k) for k in range(2, 8)}
            # not live in the call: what the list pass leaves for a skipped pixel, every other AOV as the pixel's last live sample left it
            assert same(B[2][dead], np.broadcast_to(one, B[2][dead].shape)) and same(B[5][dead], np.broadcast_to(one, B[5][dead].shape)), "call %d" % i
            if prev:
                for k in (3, 4, 6, 7):
                    assert same(B[k][dead], prev[k][dead]), "call %d, AOV %d" % (i, k)
            for k in range(2, 8):
                assert same(B[k][~dead], A[k][~dead]), "call %d, AOV %d" % (i, k)
            assert differing(state(b), ref.compose(S, ref.frames_held(budget, (4,) * (i + 1)))) == 0


@pytest.mark.gpu
def test_raised_budget_resumes(settings):
    """Budget 4, two calls of 4 frames, raised to never, 4 more frames: frames 0-3 plus frames 8-11, against the oracle's accumulation of exactly
    those frames."""
    import oracle_lib as ol
    s = depth3(settings)
    W, H = 20, 12
    with context("cornell") as b:
        b.SetSampleBudget(np.full((H, W), 4, np.uint32))
        b.Render(W, H, 4, s, 0.0); b.Render(W, H, 4, s, 0.0)
        assert b.LivePixels() == 0
        b.SetSampleBudget(np.full((H, W), NEVER, np.uint32))
        assert b.GetNumberOfSamplesSinceLastInvalidate() == 8
        b.Render(W, H, 4, s, 0.0)
        assert b.LivePixels() == W * H
        got = state(b)
        view, pf = b.HostSceneView(), b.FrameConstants(W, H, 0, s, 0.0)     # (the view points into the context: the oracle runs while it lives)
        out = np.zeros((H, W, 4), np.float32); jit = np.zeros((H, W, 4), np.float32)
        ol.render(view, pf, W, H, 4, first_frame=0, threads=4, jittered=True, out=out, jit=jit)
        ol.render(view, pf, W, H, 4, first_frame=8, threads=4, jittered=True, out=out, jit=jit)
    assert differing(got, (out, jit)) == 0, "%d pixels differ (output %d, jittered %d)" % (
        differing(got, (out, jit)), int((bits(got[0]) != bits(out)).any(-1).sum()), int((bits(got[1]) != bits(jit)).any(-1).sum()))


@pytest.mark.gpu
def test_tile_assignment_merges_to_the_single_context_picture(settings):
    s = depth3(settings)
    W, H = 33, 17
    budget = ref.layout(W, H, seed=2)
    whole = budgeted_sequence("cornell", W, H, (4, 4, 4), s, budget)
    y, x = np.mgrid[0:H, 0:W]
    owner = ((y // 16) * ((W + 15) // 16) + x // 16) % 2
    merged = [np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)]
    for rank in (0, 1):
        with context("cornell") as r:
            r.SetTileAssignment(rank, 2, 16, 16)
            r.SetSampleBudget(budget)
            for i in range(3):
                r.Render(W, H, 4, s, 0.0)
                assert r.LivePixels() == int((ref.live(budget, 4 * i) & (owner == rank)).sum())
            got = state(r)
            assert not bits(got[0])[owner != rank].any() and not bits(got[1])[owner != rank].any()
            for k in range(2):
                merged[k][owner == rank] = got[k][owner == rank]
    assert same(merged[0], whole[0]) and same(merged[1], whole[1])


@pytest.mark.gpu
def test_noise_target_under_a_tile_assignment_counts_what_the_budget_leaves_live(settings):
    """The stop judges the whole surface: a rank's budget holds 0 outside its tiles, and then stopped + live are its owned pixels; with a budget
    that is live everywhere the other ranks' pixels, never sampled, never stop and count as live."""
    s = depth3(settings)
    W, H = 33, 17
    y, x = np.mgrid[0:H, 0:W]
    owned = ((y // 16) * ((W + 15) // 16) + x // 16) % 2 == 0
    with context("cornell") as r:
        r.SetTileAssignment(0, 2, 16, 16)
        r.SetSampleBudget(np.where(owned, NEVER, 0).astype(np.uint32))
        r.Render(W, H, 8, s, 0.0)
        assert r.LivePixels() == int(owned.sum())
        S = state(r)
        stopped, live = r.StopConverged(0.05, 4)
        want, ws, wl = ref.stop(S[0], S[1], np.where(owned, NEVER, 0).astype(np.uint32), 0.05, 4, 8)
        assert (stopped, live) == (ws, wl) and stopped + live == int(owned.sum()) and stopped > 0 and same(r.SampleBudget(), want)
        r.SetSampleBudget(np.full((H, W), NEVER, np.uint32))
        stopped, live = r.StopConverged(0.05, 4)
        assert stopped == ws and live == wl + int((~owned).sum())


@pytest.mark.gpu
def test_adaptive_and_budget_together(settings):
    """A pixel is live iff both predicates say so: frames 0 .. MIN plain on both contexts, a threshold from the data that leaves half of the pixels
    skipping, then a budget that stops some at or below the next start and lets the others run."""
    s = depth3(settings)
    W, H, MIN = 64, 48, 16
    with context("cornell") as a, context("cornell") as b:
        b.SetOption("adaptive", 1); b.SetOption("adaptive_min_frames", MIN); b.SetOption("adaptive_test", 1)
        a.Render(W, H, MIN + 1, s, 0.0); b.Render(W, H, MIN + 1, s, 0.0)
        S0 = state(a)
        assert b.GetOption("last_adaptive") == 0 and differing(state(b), S0) == 0
        thr = checked_threshold(S0, 0.5)
        s.ConvergencePercentage = thr
        budget = ref.layout(W, H, values=(0, MIN + 1, MIN + 2, NEVER), seed=9)
        b.SetSampleBudget(budget)
        a.Render(W, H, 4, s, 0.0); b.Render(W, H, 4, s, 0.0)
        S1 = state(a)
        live = ~skips(S0, thr) & ref.live(budget, MIN + 1)
        for m in (skips(S0, thr) & ref.live(budget, MIN + 1), ~skips(S0, thr) & ~ref.live(budget, MIN + 1), live):
            assert m.sum() > 0.05 * m.size                      # every combination of the two predicates is there
        assert b.GetOption("last_budgeted") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE_GROUPS and b.LivePixels() == int(live.sum())
        want = (np.where(live[..., None], S1[0], S0[0]), np.where(live[..., None], S1[1], S0[1]))
        assert differing(state(b), want) == 0


# ---- hygiene ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_budget_calls_leave_the_render_alone_and_clearing_restores_the_plain_plan(settings):
    s = depth3(settings)
    W, H = 64, 48
    options = ("last_plan_rule_pipeline", "last_plan_frame_group", "last_plan_guided_groups", "last_copy_waves", "last_overlap", "last_adaptive", "last_budgeted")
    with context("cornell") as a, context("cornell") as b:
        a.Render(W, H, 8, s, 0.0); b.Render(W, H, 8, s, 0.0)
        a.RenderGuides(0, 2); b.RenderGuides(0, 2)
        before, guides = b.AccumDigest(), [b.ReadGuide(k) for k in range(3)]
        b.SetSampleBudget(np.full((H, W), NEVER, np.uint32))
        stopped, live = b.StopConverged(0.05, 4)
        assert stopped + live == W * H and 0 < stopped
        assert same(b.SampleBudget(), ref.stop(*state(b), np.full((H, W), NEVER, np.uint32), 0.05, 4, 8)[0])
        assert b.AccumDigest() == before and b.GetNumberOfSamplesSinceLastInvalidate() == 8
        assert all(same(g, b.ReadGuide(k)) for k, g in enumerate(guides))
        b.SetSampleBudget(None)
        assert b.GetOption("budget_set") == 0 and b.AccumDigest() == before and b.GetNumberOfSamplesSinceLastInvalidate() == 8
        a.Render(W, H, 8, s, 0.0); b.Render(W, H, 8, s, 0.0)
        for o in options:
            assert a.GetOption(o) == b.GetOption(o), o
        assert differing(state(a), state(b)) == 0


@pytest.mark.gpu
def test_stop_converged_without_a_budget_makes_one(settings):
    s = depth3(settings)
    W, H = 40, 24
    with context("cornell") as b:
        b.Render(W, H, 8, s, 0.0)
        S = state(b)
        stopped, live = b.StopConverged(0.05, 4)
        want, ws, wl = ref.stop(S[0], S[1], np.full((H, W), NEVER, np.uint32), 0.05, 4, 8)
        assert b.GetOption("budget_set") == 1 and same(b.SampleBudget(), want) and (stopped, live) == (ws, wl) and 0 < stopped < W * H
        assert b.StopConverged(0.05, 4) == (0, wl)              # a second look at the same sums stops nobody else
        b.Render(W, H, 4, s, 0.0)
        assert b.LivePixels() == wl and differing((state(b)[0][want == 8], state(b)[1][want == 8]), (S[0][want == 8], S[1][want == 8])) == 0


@pytest.mark.gpu
def test_context_gives_back_every_device_byte(gpu_tb, settings):
    s = depth3(settings)
    before = gpu_tb.GetOption("debug_live_device_bytes")
    tb = context("cornell")
    try:
        tb.SetSampleBudget(ref.layout(40, 24))
        tb.Render(40, 24, 4, s, 0.0); tb.StopConverged(0.1, 2); tb.Render(40, 24, 4, s, 0.0)
        assert gpu_tb.GetOption("debug_live_device_bytes") > before
    finally:
        tb.close()
    assert gpu_tb.GetOption("debug_live_device_bytes") == before


def refused(call, code, *words):
    from tracerboy_amd import api
    with pytest.raises(api.TracerBoyError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.gpu
def test_refusals_name_their_cause_and_leave_a_context_that_works(settings):
    from tracerboy_amd import api
    s = depth3(settings)
    W, H = 24, 16
    full = np.full((H, W), NEVER, np.uint32)
    with context("cornell") as tb:
        refused(lambda: tb.SampleBudget(), TB_E_INVALID, "no sample budget")
        refused(lambda: tb.StopConverged(0.1), TB_E_INVALID, "nothing rendered")
        refused(lambda: tb.SetSampleBudget(np.zeros((0, 4), np.uint32)), TB_E_INVALID, "dimension is 0")
        L = api.lib()
        assert L.tb_set_sample_budget(tb._ctx, 8192, 4096, full.ctypes.data_as(C.c_void_p)) == TB_E_INVALID   # refused before the array is read
        assert b"2^24" in L.tb_last_error(tb._ctx)
        tb.SetSampleBudget(full)
        refused(lambda: tb.Render(W + 1, H, 1, s, 0.0), TB_E_INVALID, "sample budget is 24 x 16", "25 x 16")
        tb.Render(W, H, 2, s, 0.0)
        assert tb.GetOption("last_budgeted") == 1 and tb.LivePixels() == W * H
        refused(lambda: tb.SetOption("count_rays", 1), TB_E_INVALID, "count_rays", "budget")
        assert tb.GetOption("count_rays") == 0
        tb.SetOption("adaptive", 1)                              # adaptive_test is 0: the per-frame form
        refused(lambda: tb.Render(W, H, 1, s, 0.0), TB_E_INVALID, "adaptive_test")
        tb.SetOption("adaptive_test", 1)
        tb.Render(W, H, 1, s, 0.0)
        assert tb.GetNumberOfSamplesSinceLastInvalidate() == 3
        for bad in (-0.1, float("nan"), float("inf")):
            refused(lambda: tb.StopConverged(bad), TB_E_INVALID, "rel_error")
        assert tb.StopConverged(0.1, 2)[0] >= 0
        tb.SetOption("adaptive", 0)
        tb.RenderRealTime(W, H, s, None, 0.0)                    # real time ignores the budget ...
        assert tb.GetOption("last_budgeted") == 0
        refused(lambda: tb.StopConverged(0.1), TB_E_INVALID, "tb_render_realtime")   # ... and leaves no accumulation to judge
        tb.Render(W, H, 1, s, 0.0)
        assert tb.GetOption("last_budgeted") == 1
    with context("cornell", {"count_rays": 1}) as tb:
        refused(lambda: tb.SetSampleBudget(full), TB_E_INVALID, "count_rays")
        tb.Render(W, H, 1, s, 0.0)
        assert tb.GetOption("budget_set") == 0 and tb.GetOption("last_budgeted") == 0


@pytest.mark.gpu
def test_a_device_group_is_refused():
    from tracerboy_amd import api
    with api.TracerBoy(devices=[0, 0]) as tb:                    # a two-member group on one device
        refused(lambda: tb.SetSampleBudget(np.zeros((4, 4), np.uint32)), TB_E_UNSUPPORTED, "multi-device group")
        refused(lambda: tb.StopConverged(0.1), TB_E_UNSUPPORTED, "multi-device group")
        tb.LoadScene(CORNELL)
        tb.Render(32, 16, 1, None, 0.0)
        assert tb.GetOption("budget_set") == 0 and tb.GetOption("last_budgeted") == 0
