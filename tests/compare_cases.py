"""The inputs of the image-quality metrics' tests (tests/test_compare_ref.py, tests/test_compare_kernels.py): sizes, patterns and the cases made of
them.  A case is (test image, reference image, keyword arguments of metrics_ref.compare); case(name, w, h) builds it, restated(name, w, h) is its
restatement, computed once per process."""
import functools

import numpy as np

import metrics_ref as ref

F32 = np.float32
TILE = 32      # cmp_ssim: windows per workgroup and axis (CMP_SSIM_TILE)
# 1 x 1; a frame smaller than a window; two with one axis too short for a window; one window; a few windows; ragged against the tile in both
# directions, one- and two-tile-wide strips; one tile exactly, one tile plus one and two tiles minus one in either axis; many workgroups with a
# count of partial records that is no power of two (pointwise 900, SSIM 20 x 11); and two frames past cmp_pointwise's grid cap of 2048 x 256
# lanes (CMP_MAX_POINTWISE_GROUPS), pointwise only: at 1024 x 600 some lanes take a second trip of the loop, at 1920 x 1080 the first 500 736
# lanes run the four-trip body and the rest three single trips
SIZES = [(1, 1), (3, 2), (10, 40), (40, 10), (11, 11), (12, 13), (75, 33), (19, 257), (257, 19),
         (TILE + 10, TILE + 10), (TILE + 11, TILE + 10), (TILE + 10, TILE + 11), (2 * TILE + 9, TILE + 11), (TILE + 11, 2 * TILE + 9), (2 * TILE + 9, 2 * TILE + 9),
         (640, 360), (1024, 600), (1920, 1080)]
PAST_THE_GRID = ((1024, 600), (1920, 1080))
SIZE_IDS = ["%dx%d" % s for s in SIZES]
PLAIN = ["random", "constant", "flat_bright", "identical", "step", "ramp", "checker", "outside", "denormal", "huge", "nan_alpha", "sums", "peak", "no_ssim"]
NONFINITE = ["nonfinite%d" % k for k in range(6)]       # k: the channel of (A.r, A.g, A.b, R.r, R.g, R.b) that is planted
ALL_EXCLUDED = "all_excluded"
LARGE = ["random", "identical", "outside", "sums", "nonfinite1", "nonfinite4"]      # at 640 x 360 the restatement costs a third of a second per case
POINTWISE_ONLY = ["no_ssim", "sums_no_ssim"]      # past the grid cap: the SSIM restatement would take seconds there, and cmp_ssim has no such loop


def names(w, h):
    """the cases run at a size.  Planted pixels need room: a frame of one pixel, or one whose few windows all hold the interior pixel, would be
    left without an included pixel or without a window, which only the named all-excluded case may be"""
    if (w, h) == (640, 360):
        return LARGE
    if (w, h) in PAST_THE_GRID:
        return POINTWISE_ONLY
    planted = NONFINITE if (w, h) not in ((1, 1), (11, 11), (12, 13)) else []
    return PLAIN + planted + ([ALL_EXCLUDED] if (w, h) in ((1, 1), (12, 13), (75, 33)) else [])


def planted_positions(w, h):
    """(x, y): a corner, a pixel on the edge between two tiles' windows, the interior"""
    return [(0, 0), (min(TILE, w - 1), min(TILE, h - 1)), (w // 2, h // 2)]


def case(name, w, h):
    rng = np.random.default_rng(100003 * w + 17 * h + sum(name.encode()))
    ys, xs = np.mgrid[0:h, 0:w]
    test = np.ones((h, w, 4), F32); refi = np.ones((h, w, 4), F32)
    kw = {}
    noise = (rng.random((h, w, 3)) * 0.1 - 0.05).astype(F32)
    if name in ("random", "nan_alpha", "huge", "peak", "no_ssim", ALL_EXCLUDED) or name.startswith("nonfinite"):
        test[..., :3] = rng.random((h, w, 3)); refi[..., :3] = rng.random((h, w, 3))
    elif name == "constant":
        # A dark flat field, on purpose.  The variances of a flat field cancel to rounding error, up to 135 * 2^-24 * (a^2 + r^2) each way beside
        # C2 = 9e-4 (metrics_ref.ssim_windows), so fp32 SSIM agrees with an fp64 evaluation to 1e-5 -- what tests/test_compare_ref.py asks of
        # every case here -- only where 2 * 135 * 2^-24 * (a^2 + r^2) / 9e-4 <= 1e-5, that is a^2 + r^2 <= 5.6e-4.  1/64 against 3/256: 3.8e-4.
        # (Bright flat fields: test_flat_images_give_the_closed_form, and DESIGN.md section 18 for what they lose.)
        test[..., :3] = 1.0 / 64.0; refi[..., :3] = 3.0 / 256.0
    elif name == "flat_bright":   # where fp32 SSIM is least exact: on the device bit for bit the restatement all the same
        test[..., :3] = 0.37; refi[..., :3] = 0.52
    elif name == "identical":
        test[..., :3] = rng.random((h, w, 3)); refi[:] = test
    elif name == "step":
        refi[..., :3] = (xs >= (w + 1) // 2)[..., None]; test[..., :3] = refi[..., :3] * F32(0.9) + noise
    elif name == "ramp":
        refi[..., :3] = (xs / max(w - 1, 1))[..., None] * np.array([1.0, 0.5, 0.25]); test[..., :3] = refi[..., :3] + noise
    elif name == "checker":
        refi[..., :3] = ((xs + ys) & 1)[..., None]; test[..., :3] = ((xs + ys + (xs > w // 2)) & 1)[..., None]
    elif name == "outside":       # below 0 and above peak
        test[..., :3] = rng.random((h, w, 3)) * 3.0 - 1.0; refi[..., :3] = rng.random((h, w, 3)) * 3.0 - 1.0
    elif name == "denormal":      # denormals and -0 against zeros, denormals and small normals
        test[..., :3] = rng.choice(np.array([1e-40, -1e-40, 1.4e-45, -0.0, 0.0, 1.2e-38], F32), (h, w, 3))
        refi[..., :3] = rng.choice(np.array([0.0, -0.0, 3e-41, 1e-20], F32), (h, w, 3))
    elif name in ("sums", "sums_no_ssim"):          # an accumulation: (rgb * n, n); without a sample: the last pixel and, where windows are left over, half a column
        n = rng.integers(1, 4, (h, w)).astype(F32)
        if w * h > 1 and (w, h) != (11, 11):      # (the one window of 11 x 11 holds every pixel)
            n[h - 1, w - 1] = 0
        if w >= 19 or w < 11 or h < 11:
            n[:h // 2, 0] = 0
        if name == "sums_no_ssim":          # no window to keep: unsampled pixels all over the frame, about one in five hundred
            n[rng.random((h, w)) < 0.002] = 0
        test[..., :3] = rng.random((h, w, 3)).astype(F32) * n[..., None]; test[..., 3] = n
        refi[..., :3] = rng.random((h, w, 3))
        kw["flags"] = ref.TB_COMPARE_SUMS | (ref.TB_COMPARE_SSIM if name == "sums" else 0)
    if name == "huge":            # finite, far outside the clamp: the fp64 squares do not overflow
        for i, (x, y) in enumerate(planted_positions(w, h)):
            test[y, x, i % 3] = 1e30; refi[y, x, (i + 1) % 3] = -1e30
        test[h - 1, w - 1, :3] = -1e30; refi[h - 1, w - 1, :3] = 1e30
    if name == "nan_alpha":
        test[::2, ::3, 3] = np.nan; refi[1::2, ::2, 3] = np.nan
    if name == "peak":
        test[..., :3] *= 3; refi[..., :3] *= 3; kw.update(peak=2.5, rel_epsilon=0.5)
    if name == "no_ssim":
        kw["flags"] = 0
    if name.startswith("nonfinite"):
        k = int(name[len("nonfinite"):])
        values = [np.nan, np.inf, -np.inf]
        for i, (x, y) in enumerate(planted_positions(w, h)):
            (test if k < 3 else refi)[y, x, k % 3] = values[(k + i) % 3]
    if name == ALL_EXCLUDED:
        test[..., 1] = np.nan
    return test, refi, kw


@functools.lru_cache(maxsize=None)
def restated(name, w, h):
    test, refi, kw = case(name, w, h)
    return test, refi, kw, ref.compare(test, refi, **kw)
