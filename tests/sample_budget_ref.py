"""NumPy restatement of sample budgets: which pixels a budgeted call lists, what a pixel holds after a sequence of calls,
the budgets the tests lay out, and the noise target (dn_kernels.hip budget_stop_kernel behind section 12's prepare and prefilter) in float32,
operation for operation.  Imported by tests/test_sample_budget*.py; self_check() is run by the CPU tests."""
import numpy as np

import still_denoise_ref as dn

F32 = np.float32
NEVER = 0xffffffff
VALUES = (0, 1, 4, 5, 8, NEVER)


def live(budget, first_frame):
    """The pixels a call that starts at global frame first_frame lists: first_frame < budget."""
    return np.uint64(first_frame) < np.asarray(budget, np.uint64)


def frames_held(budget, calls):
    """Per pixel, which of the call boundaries its sums are the plain render's of: the index k into the boundaries (0, n0, n0 + n1, ...) -- valid for a
    budget that does not change between the calls (a pixel that is dead at one start is dead at every later one)."""
    b = np.asarray(budget, np.uint64)
    k = np.zeros(b.shape, np.int64)
    start = 0
    for i, n in enumerate(calls):
        k = np.where(np.uint64(start) < b, i + 1, k)
        start += n
    return k


def compose(states, k):
    """states[j] = a plain render's (output, jittered) at boundary j, states[0] = zeros; the budgeted picture: states[k[p]] at pixel p."""
    o = np.zeros_like(states[-1][0]); q = np.zeros_like(states[-1][1])
    for j, (so, sq) in enumerate(states):
        m = k == j
        o[m] = so[m]; q[m] = sq[m]
    return o, q


def lanes(width, height):
    """Per pixel: its 16x16 region (row-major), its 8x8 tile (row-major over the frame's tiles), and whether region / tile lie wholly in the frame."""
    y, x = np.mgrid[0:height, 0:width]
    rx = (width + 15) // 16; tx = (width + 7) // 8
    region = (y // 16) * rx + x // 16
    tile = (y // 8) * tx + x // 8
    region_whole = ((x // 16) * 16 + 16 <= width) & ((y // 16) * 16 + 16 <= height)
    tile_whole = ((x // 8) * 8 + 8 <= width) & ((y // 8) * 8 + 8 <= height)
    return region, tile, region_whole, tile_whole


def layout(width, height, values=VALUES, seed=11):
    """A budget in which single lanes (every pixel draws its value), whole waves (every third 8x8 tile that lies wholly in the frame) and whole
    regions (every fourth 16x16 region that does, from the second on) carry the values in turn."""
    rng = np.random.default_rng(seed)
    v = np.asarray(values, np.uint32)
    b = v[rng.integers(0, len(v), (height, width))]
    region, tile, region_whole, tile_whole = lanes(width, height)
    for i, t in enumerate(np.unique(tile[tile_whole & (tile % 3 == 0)])):
        b[tile == t] = v[i % len(v)]
    for i, r in enumerate(np.unique(region[region_whole & (region % 4 == 1)])):
        b[region == r] = v[i % len(v)]
    return np.ascontiguousarray(b, np.uint32)


def carries_every_value(budget, mask, values=VALUES):
    return all((budget[mask] == np.uint32(v)).any() for v in values)


def check_layout(budget, width, height, values=VALUES, whole_regions=True):
    """What the tests rely on: every value on single lanes of the ragged last column and row, on a whole wave, and (where the frame has room) on a
    whole region."""
    region, tile, region_whole, tile_whole = lanes(width, height)
    y, x = np.mgrid[0:height, 0:width]
    if width % 16:
        assert carries_every_value(budget, x >= width // 16 * 16, values)
    if height % 16:
        assert carries_every_value(budget, y >= height // 16 * 16, values)
    if whole_regions:
        for v in values:
            assert any((budget[tile == t] == np.uint32(v)).all() for t in np.unique(tile[tile_whole])), v
            assert any((budget[region == r] == np.uint32(v)).all() for r in np.unique(region[region_whole])), v
    mixed = [r for r in np.unique(region) if len(np.unique(budget[region == r])) == len(values)]
    assert mixed, "no region holds every value on single lanes"


def stop(output, jittered, budget, rel_error, min_frames, frame):
    """tb_budget_stop_converged / tb_run_budget_stop: (the budget afterwards, pixels stopped, pixels live afterwards)."""
    o, q = np.asarray(output, F32), np.asarray(jittered, F32)
    b = np.array(budget, np.uint32)
    V = dn.prefilter(dn.prepare(o, q))[..., 3]
    re = F32(rel_error)
    with np.errstate(all="ignore"):
        n, m = o[..., 3], q[..., 3]
        r = n - m
        c = o[..., :3] / n[..., None]
        l = dn.luma(c)
        threshold = (re * re) * ((l * l) + F32(0.01))
        black = (c[..., 0] <= 0) & (c[..., 1] <= 0) & (c[..., 2] <= 0)
        stops = (b > np.uint32(frame)) & (np.uint64(frame) >= np.uint64(min_frames)) & (n > 0) & (black | ((m > 0) & (r > 0) & (V < threshold)))
    b[stops] = np.uint32(frame)
    return b, int(stops.sum()), int((b > np.uint32(frame)).sum())


def threshold_of(output, rel_error):
    """rel_error^2 (luma(mean)^2 + 0.01) per pixel, as the kernel forms it."""
    o = np.asarray(output, F32); re = F32(rel_error)
    with np.errstate(all="ignore"):
        l = dn.luma(o[..., :3] / o[..., 3:4])
        return (re * re) * ((l * l) + F32(0.01))


def gaussian_sums(rng, shape, mean, sigma, n):
    """Sums of n samples per pixel of a grey value ~ N(mean, sigma), each sample in the second half with probability 1/2 (at least one in each):
    (output, jittered) as the accumulation holds them."""
    h, w = shape
    s = rng.normal(mean, sigma, (n, h, w))
    coin = rng.random((n, h, w)) < 0.5
    coin[0] = True; coin[1] = False
    o = np.empty((h, w, 4), F32); q = np.empty((h, w, 4), F32)
    o[..., :3] = s.sum(0)[..., None]; o[..., 3] = n
    q[..., :3] = (s * coin).sum(0)[..., None]; q[..., 3] = coin.sum(0)
    return o, q


def self_check():
    # live / frames_held / compose on a hand-made case: three calls of 4 frames
    b = np.array([[0, 1, 4, 5, 8, NEVER]], np.uint32)
    assert live(b, 0).tolist() == [[False, True, True, True, True, True]] and live(b, 4).tolist() == [[False, False, False, True, True, True]]
    k = frames_held(b, (4, 4, 4))
    assert k.tolist() == [[0, 1, 1, 2, 2, 3]]                 # min(12, 4 ceil(b / 4)) frames
    assert [min(12, 4 * -(-int(v) // 4)) for v in b[0]] == [4 * int(j) for j in k[0]]
    assert frames_held(b, (1,) * 9).tolist() == [[0, 1, 4, 5, 8, 9]]    # one-frame calls: budgets are exact
    states = [(np.full((1, 6, 4), j, F32), np.full((1, 6, 4), 10 + j, F32)) for j in range(4)]
    o, q = compose(states, k)
    assert o[0, :, 0].tolist() == [0, 1, 1, 2, 2, 3] and q[0, :, 0].tolist() == [10, 11, 11, 12, 12, 13]
    # the layouts of the tests
    check_layout(layout(100, 70), 100, 70)
    check_layout(layout(20, 12), 20, 12, whole_regions=False)
    # stop: black stops, a noisy pixel does not, a quiet one does, n = 0 / m = 0 / m = n never by variance, F < min_frames never, stopped stay
    o = np.zeros((1, 8, 4), F32); q = np.zeros((1, 8, 4), F32)
    o[0, 0] = (0, 0, 0, 4); q[0, 0] = (0, 0, 0, 2)            # black
    o[0, 1] = (8, 8, 8, 4); q[0, 1] = (8, 8, 8, 2)            # halves 4 and 0: noisy
    o[0, 2] = (8, 8, 8, 4); q[0, 2] = (4, 4, 4, 2)            # equal halves: variance 0
    o[0, 3] = (0, 0, 0, 0)                                    # never sampled
    o[0, 4] = (8, 8, 8, 4); q[0, 4] = (0, 0, 0, 0)            # m = 0
    o[0, 5] = (8, 8, 8, 4); q[0, 5] = (8, 8, 8, 4)            # m = n
    o[0, 6] = (8, 8, 8, 4); q[0, 6] = (4, 4, 4, 2)            # already stopped
    o[0, 7] = (np.nan, 1, 1, 4); q[0, 7] = (1, 1, 1, 2)       # NaN mean
    bud = np.full((1, 8), NEVER, np.uint32); bud[0, 6] = 3
    # (the prefilter spreads pixel 1's variance over its neighbours: judge pixel 2 on a surface of its own)
    nb, stopped, alive = stop(o, q, bud, 0.1, 4, 4)
    assert nb[0, 0] == 4 and nb[0, 1] == NEVER and nb[0, 3] == NEVER and nb[0, 6] == 3 and nb[0, 7] == NEVER
    assert stopped == int((nb != bud).sum()) and alive == int((nb > 4).sum())
    nb2, s2, a2 = stop(o[:, 2:3], q[:, 2:3], bud[:, 2:3], 0.1, 4, 4)
    assert nb2[0, 0] == 4 and (s2, a2) == (1, 0)
    for lone in (4, 5):
        assert stop(o[:, lone:lone + 1], q[:, lone:lone + 1], bud[:, lone:lone + 1], 0.1, 4, 4)[1] == 0
    assert stop(o, q, bud, 0.1, 5, 4)[1] == 0                  # F below min_frames
    assert stop(o, q, bud, 0.0, 4, 4)[1] == 1                  # rel_error 0: V < 0 never holds, black alone stops
    return True
