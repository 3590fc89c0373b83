"""The staged form of nn_convk (tb_run_conv with form = 1) against the plain form, bit for bit.

Both forms accumulate tap-major, then k-block, one accumulator per block of 16 output channels, and give the matrix core the same fragments: the
staged one only fetches them from an LDS image of its 32 x 8 tile and halo.  So there is no tolerance here.  Sizes: every width 1 ... 35 at heights
1, 2, 3, 4, 5, 7, 8, 9, 16, 17 -- tile interiors, edges and remainders, pictures smaller than a tile and than the filter.  A source read upsampled
needs even sizes; the odd ones are covered by the other configurations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = range(1, 36)
HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def filters(rng, c_out, c_in, k):
    return (rng.standard_normal((c_out, c_in, k, k)) * np.sqrt(2.0 / (k * k * c_in))).astype(np.float16), (rng.standard_normal(c_out) * 0.1).astype(np.float16)


def both_forms(tb, a, w, b, **kw):
    plain, staged = tb.RunConv(a, w, b, form=0, **kw), tb.RunConv(a, w, b, form=1, **kw)
    return plain, staged


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("config", ["3-to-32", "64-to-32-upsampled", "20-and-7-to-48", "5-upsampled-and-3-to-64"])
def test_staged_equals_plain_at_every_size(gpu_tb, k, config):
    rng = np.random.default_rng(k + len(config))
    c_a, c_b, c_out, up = {"3-to-32": (3, 0, 32, False), "64-to-32-upsampled": (64, 0, 32, True), "20-and-7-to-48": (20, 7, 48, False),
                           "5-upsampled-and-3-to-64": (5, 3, 64, True)}[config]
    w, b = filters(rng, c_out, c_a + c_b, k)
    big_a, big_b = (rng.random((17, 35, c_a)) - 0.25).astype(np.float16), (rng.random((17, 35, max(c_b, 1))) - 0.25).astype(np.float16)
    checked = 0
    for height in HEIGHTS:
        for width in WIDTHS:
            if up and (width | height) & 1:
                continue
            a = np.ascontiguousarray(big_a[:height // 2, :width // 2] if up else big_a[:height, :width])
            in_b = np.ascontiguousarray(big_b[:height, :width, :c_b]) if c_b else None
            relu = bool((width + height) & 1) or up                   # both ways
            plain, staged = both_forms(gpu_tb, a, w, b if width % 3 else None, in_b=in_b, upsample_a=up, relu=relu)
            assert plain.shape == (height, width, c_out)
            assert np.array_equal(bits(plain), bits(staged)), (config, k, width, height)
            checked += 1
    assert checked == (len([h for h in HEIGHTS if not h & 1]) * 17 if up else 350)
    assert float(np.abs(plain.astype(np.float32)).max()) > 0.05       # the layer is not dead


@pytest.mark.parametrize("k", [3, 5])
def test_a_nan_spreads_over_its_neighbourhood_alone_across_tile_seams(gpu_tb, k):
    """a NaN in the last column and row of the first 32 x 8 tile: its K x K neighbourhood lies in four tiles"""
    rng = np.random.default_rng(50 + k)
    x = rng.random((12, 40, 35)).astype(np.float16); w, b = filters(rng, 32, 35, k)
    r = (k - 1) // 2
    poisoned = x.copy(); poisoned[7, 31, 33] = np.nan
    plain, staged = both_forms(gpu_tb, poisoned, w, b)
    clean_plain, clean = both_forms(gpu_tb, x, w, b)                  # afterwards, on the same sizes
    mask = np.zeros(staged.shape[:2], bool); mask[7 - r:8 + r, 31 - r:32 + r] = True
    assert np.isnan(staged[mask]).all() and not np.isnan(staged[~mask]).any() and int(mask.sum()) == k * k
    assert np.array_equal(np.isnan(plain), np.isnan(staged))
    assert np.array_equal(bits(staged[~mask]), bits(clean[~mask])) and np.array_equal(bits(clean), bits(clean_plain))
    assert np.array_equal(bits(plain[~mask]), bits(staged[~mask]))
