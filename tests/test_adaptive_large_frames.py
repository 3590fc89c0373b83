"""-m gpu: the adaptive launch's helper kernels at a frame past their one-pass sizes (pt_kernels.hip live_list_count / _scan / _scatter,
accumulate_live_kernel, accumulate_samples_kernel), against the oracle, bit for bit.

live_list_scan is one workgroup of 1024 threads; thread t owns a run of per = ceil(regions / 1024) region counts.  Every other adaptive test has
at most 192 regions (per = 1).  accumulate_live_kernel has one lane per list entry on a grid of at most 2048 x 256 = 524 288 lanes and strides
only past that; accumulate_samples_kernel the same over the pixels.

No warm-up render: the surfaces are made in NumPy and loaded through a render-state file, so which pixel is live is chosen
here, pixel by pixel.  output.w = next_frame = MIN + 1 and rgb = w x a smooth positive colour.  A dead pixel has jittered = 0.5 x output in all four
words (equal quotients: error 0) or rgb = 0 (the black rule); a live pixel has jittered.rgb = 2 x output.rgb x (jittered.w / output.w): an error of
about sqrt(r + g + b), far above the threshold.  The prediction is skips() of tests/test_adaptive_sampling.py on the surfaces, and it is asserted
to agree with the construction.  The reference is the oracle continuing the same surfaces over the whole frame."""
import copy

import numpy as np
import pytest

from conftest import CORNELL
from test_adaptive_sampling import MIN, bits, frozen, same, skips, state
from test_render_state import Oracle
from test_render_state_host import default_info

pytestmark = pytest.mark.gpu
RULE_ADAPTIVE, RULE_ADAPTIVE_GROUPS = 7, 8
THR = 0.01                                                      # fixed: a dead pixel's error is 0 or it is black, a live pixel's is above 0.5
GRID = 2048 * 256                                               # lanes of the two folds' largest grid

# The frame.  Conditions: more than 2048 regions (per >= 3); regions % per != 0 (the last thread's run is short, and threads behind it own nothing);
# W and H no multiples of 16 (ragged regions in the last column and row); W * H > 524 288 + the dead pixels of state A (the live fold strides).
W, H = 1010, 555
BX, BY = (W + 15) // 16, (H + 15) // 16
REGIONS = BX * BY                                               # 64 x 35 = 2240
PER = (REGIONS + 1023) // 1024                                  # 3: 747 threads own runs, the last one 2 regions; 277 threads own nothing
assert REGIONS > 2048 and REGIONS % PER != 0 and W % 16 and H % 16 and W * H > GRID


def lanes():
    """Of every pixel: its region in block_region order, and its place among the region's 256 lanes (wave = the 8x8 tile (w & 1, w >> 1),
    lane = (lane & 7, lane >> 3): the lock-step kernel's mapping)."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    region = (y // 16) * BX + x // 16
    place = (((y % 16) // 8) * 2 + (x % 16) // 8) * 64 + (y % 8) * 8 + x % 8
    return region, place


def surfaces(live, seed):
    """(output, jittered) of frames [0, MIN + 1) in which exactly the pixels of `live` fail the skip test; the dead ones are of either kind."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    n, nj = np.float32(MIN + 1), np.float32(8)
    out = np.empty((H, W, 4), np.float32)
    out[..., 0] = n * (np.float32(0.2) + np.float32(0.6) * x / np.float32(W))
    out[..., 1] = n * (np.float32(0.3) + np.float32(0.5) * y / np.float32(H))
    out[..., 2] = n * (np.float32(0.5) + np.float32(0.25) * np.sin(x / np.float32(37)) * np.cos(y / np.float32(23)))
    out[..., 3] = n
    jit = np.empty_like(out)
    jit[..., :3] = np.float32(2) * out[..., :3] * (nj / n)
    jit[..., 3] = nj
    black = ~live & (rng.random((H, W)) < 0.5)
    out[black, :3] = 0
    jit[black, :3] = 1                                          # c = 0, j > 0: an infinite error -- only the black rule skips it
    equal = ~live & ~black
    jit[equal] = np.float32(0.5) * out[equal]
    return out, jit


def state_a():
    """Nearly all live.  Dead: three runs of PER regions -- regions 0 .. PER - 1 (thread 0's run), a thread's run in the middle, the last PER regions
    of the frame (the end of one thread's run and the short last run) --, 300 single pixels, and all but one pixel of one region: the one at
    wave 3, lane 63.  Condition: more live pixels than the fold's grid has lanes."""
    region, place = lanes()
    live = np.ones((H, W), bool)
    middle = REGIONS // 2 // PER * PER
    for r in list(range(PER)) + list(range(middle, middle + PER)) + list(range(REGIONS - PER, REGIONS)):
        live[region == r] = False
    rng = np.random.default_rng(5)
    live.ravel()[rng.permutation(W * H)[:300]] = False
    lone = 15 * BX + 40                                         # a whole region inside the frame
    live[region == lone] = (place == 3 * 64 + 63)[region == lone]
    return live, surfaces(live, 6)


def state_b():
    """Mixed.  Every region -- the ragged last column and row too -- draws its number of live lanes: 0, 1, 255, 256 with probability 1/8 each,
    otherwise uniform in 2 .. 254; the lanes at random places, so that whole waves of some regions are dead.  Condition: 10 % .. 90 % live."""
    region, place = lanes()
    rng = np.random.default_rng(7)
    pick = rng.integers(0, 8, REGIONS)
    count = np.where(pick < 4, np.array([0, 1, 255, 256])[pick % 4], rng.integers(2, 255, REGIONS))
    rank = np.argsort(np.argsort(rng.random((REGIONS, 256)), axis=1), axis=1)
    live = rank[region, place] < count[region]
    return live, surfaces(live, 8)


class Chain:
    """The oracle's surfaces k frames after a state (frames MIN + 1 ...), one frame at a time, each computed once: after(0) is the state itself."""

    def __init__(self, oracle, st):
        self.oracle, self.states = oracle, [st]

    def after(self, k):
        while len(self.states) <= k:
            self.states.append(self.oracle.on(MIN + len(self.states), 1, self.states[-1], W, H))
        return self.states[k]


@pytest.fixture(scope="module")
def made(built, settings):
    oracle = Oracle(CORNELL, settings)                          # depth 4
    res = {}
    for name, make in (("a", state_a), ("b", state_b)):
        live, st = make()
        res[name] = (live, st, Chain(oracle, st))
    return res


def context(adaptive_test=None):
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    tb.LoadScene(CORNELL)
    if adaptive_test is not None:
        tb.SetOption("adaptive", 1); tb.SetOption("adaptive_min_frames", MIN); tb.SetOption("adaptive_test", adaptive_test)
    return tb


def load(tb, st, settings, path, adaptive_test=None):
    """The header's adaptive, adaptive_min_frames and adaptive_test are the context's options; the payload is the same for every context."""
    from tracerboy_amd import api
    kw = {} if adaptive_test is None else {"adaptive": 1, "adaptive_min_frames": MIN, "adaptive_test": adaptive_test}
    info = default_info(first=0, next_frame=MIN + 1, scene_digest=tb.SceneDigest(), settings=settings, camera=tb.GetCamera(), **kw)
    api.WriteStateFile(str(path), info, st[0], st[1])
    tb.LoadState(str(path))
    assert tb.GetNumberOfSamplesSinceLastInvalidate() == MIN + 1
    assert same(state(tb)[0], st[0]) and same(state(tb)[1], st[1])


def differing(got, want):
    return int(((bits(got[0]) != bits(want[0])) | (bits(got[1]) != bits(want[1]))).any(-1).sum())


def check_construction(name, live, st):
    dead = skips(st, THR)
    assert np.array_equal(~dead, live), "the skip test and the construction disagree on %d pixels" % int((~dead != live).sum())
    n = int(live.sum())
    print("state %s: %d of %d pixels live (%.1f %%)" % (name.upper(), n, W * H, 100.0 * n / (W * H)))
    if name == "a":
        assert n > GRID                                         # accumulate_live_kernel strides
    else:
        assert 0.1 * W * H <= n <= 0.9 * W * H
        region, place = lanes()
        per_wave = np.zeros((REGIONS, 4), np.int64)
        np.add.at(per_wave, (region[live], place[live] // 64), 1)
        assert ((per_wave.sum(1) > 0) & (per_wave.min(1) == 0)).any(), "no region with a live and a wholly dead wave"


@pytest.mark.parametrize("name", ["a", "b"])
def test_calls_on_a_large_frame_are_the_oracle_where_live(made, settings, tmp_path, name):
    """adaptive_test = 1, calls of 3 and 2 frames.  After each: the live count is the skip test's on the surfaces before the call, and both surfaces
    are the surfaces before the call where it skips and the oracle's elsewhere.  A plain context loaded with the same payload gives the oracle's
    bits over the whole frame (accumulate_samples_kernel past one pass of its grid)."""
    live, st, chain = made[name]
    check_construction(name, live, st)
    s = copy.copy(settings); s.ConvergencePercentage = THR
    with context() as a, context(1) as b:
        load(a, st, settings, tmp_path / "plain.tbs")
        load(b, st, settings, tmp_path / "adaptive.tbs", 1)
        done = 0
        for call, n in enumerate((3, 2)):
            before = state(b)
            skip = skips(before, THR)
            # the oracle continuing `before`: where a pixel is live its sums are the plain render's so far (it was live in every call before)
            assert same(before[0][~skip], chain.after(done)[0][~skip]) and same(before[1][~skip], chain.after(done)[1][~skip])
            a.Render(W, H, n, s, 0.0); b.Render(W, H, n, s, 0.0)
            done += n
            ref = chain.after(done)
            assert differing(state(a), ref) == 0, "call %d: the plain context differs from the oracle" % call
            assert b.GetOption("last_adaptive") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE_GROUPS
            assert b.LivePixels() == int((~skip).sum()), "call %d" % call
            want = np.where(skip[..., None], before[0], ref[0]), np.where(skip[..., None], before[1], ref[1])
            got = state(b)
            assert differing(got, want) == 0, "call %d (%d frames): %d pixels differ from the prediction" % (call, n, differing(got, want))
        assert b.GetNumberOfSamplesSinceLastInvalidate() == MIN + 6


def test_per_frame_mode_on_a_large_frame(made, settings, tmp_path):
    """adaptive_test = 0, state B, one call of 2 frames: the plain render frozen where the skip test first held (frozen())."""
    live, st, chain = made["b"]
    s = copy.copy(settings); s.ConvergencePercentage = THR
    with context(0) as b:
        load(b, st, settings, tmp_path / "per_frame.tbs", 0)
        b.Render(W, H, 2, s, 0.0)
        assert b.GetOption("last_adaptive") == 1 and b.GetOption("last_plan_rule_pipeline") == RULE_ADAPTIVE
        assert b.LivePixels() == int((~skips(st, THR)).sum()) == int(live.sum())
        po, pq, _ = frozen([chain.after(0), chain.after(1), chain.after(2)], THR)
        got = state(b)
        assert differing(got, (po, pq)) == 0, "%d pixels differ from the prediction" % differing(got, (po, pq))
