"""The noise target of sample budgets: budget_stop_kernel behind section 12's prepare and prefilter, through the seam
tb_run_budget_stop on synthetic sums, bit for bit against tests/sample_budget_ref.py; and a statistical check on Gaussian samples of known sigma
written through a state file."""
import numpy as np
import pytest

import sample_budget_ref as ref
import still_denoise_ref as dn
from conftest import CORNELL
from sample_budget_ref import NEVER

F32 = np.float32
FRAME = 8
KINDS = 12


def synthetic(w, h, shift, seed=3):
    """Sums whose pixels cycle through the kinds below (pixel index + shift, so that a 1 x 1 surface takes each in turn), and a budget in which
    kind 11 and a sprinkle of others are stopped already."""
    rng = np.random.default_rng(seed + 17 * shift)
    kind = (np.arange(w * h).reshape(h, w) + shift) % KINDS
    o = np.empty((h, w, 4), F32); q = np.empty((h, w, 4), F32)
    o[..., 3] = FRAME
    o[..., :3] = (rng.uniform(0.05, 4.0, (h, w, 1)) * FRAME * rng.uniform(0.9, 1.1, (h, w, 3))).astype(F32)
    q[..., 3] = rng.integers(1, FRAME, (h, w))
    noise = np.where(rng.random((h, w, 1)) < 0.5, rng.uniform(0.98, 1.02, (h, w, 3)), rng.uniform(0.5, 1.5, (h, w, 3)))   # quiet and noisy pixels
    q[..., :3] = (o[..., :3] * (q[..., 3:4] / F32(FRAME)) * noise).astype(F32)
    o[kind == 1] = 0; q[kind == 1] = 0                                          # n = 0: never sampled
    q[kind == 2] = 0                                                            # m = 0
    q[kind == 3] = o[kind == 3]                                                 # m = n
    q[kind == 4, 3] = FRAME + 3                                                 # m > n
    o[kind == 5, :3] = 0                                                        # black
    o[kind == 6, :3] *= F32(-1)                                                 # negative means
    o[kind == 7, 0] = np.nan                                                    # a NaN mean
    o[kind == 8, :3] = F32(3e38) * rng.uniform(0.9, 1.0, (int((kind == 8).sum()), 3)).astype(F32); o[kind == 8, 3] = 2    # sums near FLT_MAX
    q[kind == 8, :3] = F32(1e37); q[kind == 8, 3] = 1
    q[kind == 9] = o[kind == 9] * F32(0.5)                                      # equal halves: variance 0
    o[kind == 10, :3] = F32(3e-41); q[kind == 10, :3] = F32(1e-41); q[kind == 10, 3] = 4    # denormal sums
    budget = np.full((h, w), NEVER, np.uint32)
    budget[kind == 11] = rng.integers(0, FRAME + 1, int((kind == 11).sum()))    # stopped already (budget <= F)
    budget[rng.random((h, w)) < 0.05] = FRAME
    budget[rng.random((h, w)) < 0.05] = FRAME + 1                               # stops later: still live now
    return o, q, budget


def exact_thresholds():
    """(q, rel_error) for a 1 x 1 surface with o = (2, 2, 2, 2) whose threshold is exactly V, one fp32 step above V, one below: searched among
    rel_error's neighbours for a few hundred values of q."""
    o = np.array([[[2, 2, 2, 2]]], F32)
    found = {}
    for k in range(600):
        q = np.array([[[1.3 + 1e-3 * k] * 3 + [1]]], F32)
        V = dn.prefilter(dn.prepare(o, q))[0, 0, 3]
        l = dn.luma(o[..., :3] / o[..., 3:4])[0, 0]
        c = (l * l) + F32(0.01)
        re0 = np.sqrt(np.float64(V) / np.float64(c)).astype(F32)
        cand = (re0.view(np.uint32) + np.arange(-2000, 2000)).astype(np.uint32).view(F32)
        thr = (cand * cand) * c
        for name, t in (("on", V), ("above", np.nextafter(V, F32(np.inf))), ("below", np.nextafter(V, F32(-np.inf)))):
            hit = cand[thr == t]
            if name not in found and len(hit):
                found[name] = (o, q, float(hit[0]), V, t)
        if len(found) == 3:
            break
    return found


def test_exact_thresholds_exist_on_the_cpu():
    found = exact_thresholds()
    assert sorted(found) == ["above", "below", "on"]
    for name, (o, q, re, V, t) in found.items():
        assert ref.threshold_of(o, re)[0, 0] == t
        b, stopped, live = ref.stop(o, q, np.full((1, 1), NEVER, np.uint32), re, 0, FRAME)
        assert stopped == (1 if name == "above" else 0), name    # V < threshold: strict


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (5, 7), (16, 16), (17, 33), (257, 3)], ids=lambda s: "%dx%d" % s)
def test_seam_equals_numpy_bit_for_bit(gpu_tb, size):
    w, h = size
    classes = set()
    for shift in (range(KINDS) if w * h == 1 else (0, 5)):
        o, q, budget = synthetic(w, h, shift)
        for min_frames in (FRAME + 1, FRAME, FRAME - 1, 0):     # F below, at and above min_frames
            for rel_error in (0.0, 0.02, 0.3, 1e3):
                got, stopped, live = gpu_tb.RunBudgetStop(o, q, budget, rel_error, min_frames, FRAME)
                want, ws, wl = ref.stop(o, q, budget, rel_error, min_frames, FRAME)
                assert np.array_equal(got, want), (shift, min_frames, rel_error, int((got != want).sum()))
                assert (stopped, live) == (ws, wl)
                assert np.array_equal(got[budget <= FRAME], budget[budget <= FRAME])      # stopped pixels stay as they are
                if min_frames > FRAME:
                    assert stopped == 0
                classes.add((ws > 0, wl > 0))
    assert (True, True) in classes or w * h == 1                 # some stop and some stay: nothing passes vacuously


@pytest.mark.gpu
def test_seam_on_and_one_step_either_side_of_the_threshold(gpu_tb):
    found = exact_thresholds()
    for name, (o, q, re, V, t) in found.items():
        got, stopped, live = gpu_tb.RunBudgetStop(o, q, np.full((1, 1), NEVER, np.uint32), re, 0, FRAME)
        assert (int(got[0, 0]), stopped, live) == ((FRAME, 1, 0) if name == "above" else (NEVER, 0, 1)), name


@pytest.mark.gpu
def test_seam_refusals(gpu_tb):
    from tracerboy_amd import api
    o = np.ones((2, 2, 4), F32)
    for bad in (-1.0, float("nan")):
        with pytest.raises(api.TracerBoyError) as e:
            gpu_tb.RunBudgetStop(o, o, np.zeros((2, 2), np.uint32), bad, 0, 1)
        assert e.value.code == -1 and "rel_error" in str(e.value)
    assert gpu_tb.RunBudgetStop(o, o, np.zeros((2, 2), np.uint32), 0.1, 0, 1)[1:] == (0, 0)


@pytest.mark.gpu
def test_gaussian_samples_of_known_sigma(built, settings, tmp_path):
    """64 samples per pixel of a grey value ~ N(1, sigma), rel_error 0.05, the standard error of the mean relative to sqrt(luma^2 + 0.01) a
    factor 3 below (sigma 0.134) or above (sigma 1.206) it; 48 x 48 pixels of one class per surface, so that the prefilter mixes no classes.
    The estimate is a 3 x 3-weighted chi-square of about 7 degrees of freedom against a threshold 9 times above / below its mean.
    Measured, NumPy restatement on the CPU, seeds 100-102: below -- 100 % / 100 % / 100 % stop; above -- 0.26 % / 0.48 % / 0.30 % stop.
    The cap is 2 % of either class."""
    from tracerboy_amd import api
    from test_render_state_host import default_info
    e, n, shape = 0.05, 64, (48, 48)
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        for factor, stops in ((1.0 / 3.0, True), (3.0, False)):
            sigma = e * factor * np.sqrt(1.0 + 0.01) * np.sqrt(n)
            for seed in (100, 101, 102):
                o, q = ref.gaussian_sums(np.random.default_rng(seed), shape, 1.0, sigma, n)
                _, ws, wl = ref.stop(o, q, np.full(shape, NEVER, np.uint32), e, n, n)
                wrong_cpu = (wl if stops else ws) / float(shape[0] * shape[1])
                assert wrong_cpu <= 0.02, wrong_cpu             # the restatement alone stays within the cap
                path = str(tmp_path / ("gauss%d_%d.tbs" % (stops, seed)))
                api.WriteStateFile(path, default_info(first=0, next_frame=n, scene_digest=tb.SceneDigest(), settings=settings, camera=tb.GetCamera()), o, q)
                tb.LoadState(path)
                tb.SetSampleBudget(None)
                stopped, live = tb.StopConverged(e, n)
                print("factor %.2f, seed %d: %d stopped, %d live (NumPy: %d, %d)" % (factor, seed, stopped, live, ws, wl))
                assert (stopped, live) == (ws, wl)
                assert (live if stops else stopped) <= 0.02 * shape[0] * shape[1]
                assert tb.GetOption("last_budget_stop_us") > 0
