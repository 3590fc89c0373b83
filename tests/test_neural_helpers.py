"""The four helper kernels around the layers of the neural still denoiser (nn_kernels.hip: nn_pack_input, nn_unpack_output, nn_resolve_aux,
nn_to_rgba8) through their hooks tb_run_nn_pack / _unpack / _resolve_aux / _to_rgba8, bit for bit against NumPy
(tests/neural_ref.py, tests/still_guides_ref.py), a NaN for a NaN.

Sizes (width, height): 1 x 1, 5 x 7, 16 x 16, 17 x 33, 257 x 3 -- ragged against the 256-lane workgroups, against the four lanes a pixel has in the
pack, and against the extension to multiples of 16 in both directions; 16 x 16 is the one size that needs no extension.

Values are planted from the last pixel backwards, so the last pixel of the last row (the end of a ragged row) always holds one; where a picture has
fewer pixels than there are values, as many pictures are run as it takes to plant every value.

What a binary16 rounding can get wrong, and the float32 values that show it (PLANTED; the CPU test below pins the halves NumPy gives for them):
  * ties between two binary16 neighbours, the even one below (1 + 2^-11 -> 1) and above (1 + 3 * 2^-11 -> 1 + 2^-9), both signs: a truncating or
    round-half-up conversion misses one of them;
  * 65519.996 (the float32 below 65520) -> 65504 and 65520 -> infinity, both signs: 65520 is the tie between 65504 and 2^16;
  * 2^-24 -> the smallest denormal, 2^-25 -> 0 (a tie, zero is even), the float32 above 2^-25 -> the smallest denormal;
  * 3 * 2^-24 and 2^-15 (denormal halves), a float32 denormal (-> 0), -0, both infinities, NaN.

About nn_resolve_aux's "length that is a float32 denormal": the length is a square root, and the square root of the smallest positive float32,
2^-149, is 2^-74.5 -- no length is ever a denormal.  What can happen is that the SUM OF SQUARES is one (a vector of length 1e-20: l is normal, and a
kernel that flushed the denormal would give zeros instead of a unit vector), or that it underflows to 0 (length 1e-30: zeros, although the sum is
not zero), or that a component itself is a denormal.  All three are here."""
import ctypes as C

import numpy as np
import pytest

import neural_ref as nr
import still_guides_ref as guides_ref

F32, F16 = np.float32, np.float16
TB_E_INVALID = -1
SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (257, 3)]
IDS = ["%dx%d" % s for s in SIZES]

TIE_DOWN, TIE_UP = F32(1 + 2.0 ** -11), F32(1 + 3 * 2.0 ** -11)
LAST_FINITE = np.nextafter(F32(65520), F32(0))
PLANTED = np.array([TIE_DOWN, TIE_UP, -TIE_DOWN, -TIE_UP, LAST_FINITE, 65520.0, -LAST_FINITE, -65520.0, 2.0 ** -24, 2.0 ** -25,
                    np.nextafter(F32(2.0 ** -25), F32(1)), 3 * 2.0 ** -24, 2.0 ** -15, 1e-40, -0.0, np.inf, -np.inf, np.nan], F32)
# the binary16 bit patterns of PLANTED, round to nearest even (the NaN is checked as a NaN)
PLANTED_HALVES = [0x3C00, 0x3C02, 0xBC00, 0xBC02, 0x7BFF, 0x7C00, 0xFBFF, 0xFC00, 0x0001, 0x0000, 0x0001, 0x0003, 0x0200, 0x0000, 0x8000, 0x7C00, 0xFC00, None]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """bit-equal, a NaN for a NaN (a host and a device NaN may differ in sign and payload), as tests/test_still_denoise.py::same"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def assert_same(got, want, what):
    if same(got, want):
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))) if got.dtype.kind == "f" else got != want
    at = tuple(np.argwhere(bad)[0])
    raise AssertionError("%s: %d elements differ, the first at %s: got %r, want %r" % (what, int(bad.sum()), at, got[at], want[at]))


def random_surface(rng, w, h):
    """(H, W, 4) float32, both signs, magnitudes from binary16's denormals to 3e4"""
    return (rng.standard_normal((h, w, 4)) * 10.0 ** rng.uniform(-7, 4, (h, w, 4))).astype(F32)


def starts(pixels, values):
    """the first planted value of as many pictures as it takes to plant every value"""
    return range(0, len(values), min(pixels, len(values)))


def plant(surface, values, channel, start):
    """a copy with `values`, cyclically from `start`, in `channel` of the last pixels, the last pixel first"""
    a = surface.copy()
    flat = a.reshape(-1, a.shape[-1])
    k = np.arange(min(len(flat), len(values)))
    flat[len(flat) - 1 - k, channel] = values[(start + k) % len(values)]
    return a


# ---- the references themselves: no library code --------------------------------------------------------------------------------------
def test_selfcheck_of_the_references_on_the_planted_values():
    """pack_input, rgba8_of and unorm_color on literal values: a NumPy that rounds otherwise moves these, not the GPU tests' ground"""
    surface = np.zeros((1, len(PLANTED), 4), F32); surface[0, :, 1] = PLANTED
    h = nr.pack_input(surface)[0, :, 1]
    for value, half, want in zip(PLANTED, h, PLANTED_HALVES):
        assert (np.isnan(half) if want is None else int(half.view(np.uint16)) == want), (value, hex(int(half.view(np.uint16))), want)
    x = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1.0, 1.5, 0.5] + [float.fromhex(v) for v in ("0x1.010100p-9", "0x1.0100fep-9", "0x1.fefefep-1", "0x1.fefefcp-1")], F32)
    picture = np.zeros((1, len(x), 4), F32); picture[0, :, 0] = x; picture[0, :, 3] = np.nan
    got = nr.rgba8_of(picture)
    # 0.5 * 255 + 0.5 = 128 exactly.  0x1.010100p-9 * 255 = 0.49999997, and + 0.5 is a tie that goes to the even 1.0 (two float32 below fl(0.5 / 255));
    # its lower neighbour gives 0.99999994.  0x1.fefefep-1 * 255 rounds to 254.5 and gives 255, its lower neighbour 254.49998 and 254.
    assert got[0, :, 0].tolist() == [0, 255, 0, 0, 0, 0, 255, 255, 128, 1, 0, 255, 254] and (got[..., 1:3] == 0).all() and (got[..., 3] == 255).all()
    back = nr.unorm_color(got)
    assert back.dtype == F32 and back[0, 8, 0] == F32(128) / F32(255) and back[0, 1, 0] == 1.0 and (back[..., 3] == 1).all()
    assert int(F16(back[0, 8, 0]).view(np.uint16)) == 0x3804         # 128 / 255 = 0.50196: one rounding to binary16


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
def pack_ref(color, albedo=None, normal=None, unorm_color=False):
    """nr.pack_input + nr.extend16, zero-padded to 32 channels; with unorm_color the colour is uint8 / 255 of the 8-bit store"""
    if unorm_color:
        color = nr.unorm_color(nr.rgba8_of(color))
    x = nr.extend16(nr.pack_input(color, albedo, normal))
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, 0), (0, 32 - x.shape[2]))))


def assert_packed(got, want, w, h, channels, what):
    assert_same(got, want, what)
    assert got.shape == (h + -h % 16, w + -w % 16, 32)
    assert not bits(got[..., channels:]).any(), what + ": a channel past the input's holds something"
    assert not bits(got[h:]).any() and not bits(got[:, w:]).any(), what + ": the extension holds something"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_pack_random_values(gpu_tb, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    color, albedo, normal = (random_surface(rng, w, h) for _ in range(3))
    want = pack_ref(color, albedo, normal)
    assert np.isfinite(want.astype(F32)).all() and (want[:h, :w, :9] < 0).any() and (want[:h, :w, :9] > 0).any()
    assert_packed(gpu_tb.RunNnPack(color, albedo, normal), want, w, h, 9, "9 inputs")
    # no guides: channels 3-31 are zero although the colour's alpha is not
    assert_packed(gpu_tb.RunNnPack(color), pack_ref(color), w, h, 3, "3 inputs")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_pack_planted_values_in_every_channel(gpu_tb, w, h):
    rng = np.random.default_rng(w * 1000 + h + 1)
    base = [random_surface(rng, w, h) for _ in range(3)]
    seen = set()
    nan_seen = False
    for channel in range(9):
        for start in starts(w * h, PLANTED):
            planes = list(base)
            planes[channel // 3] = plant(base[channel // 3], PLANTED, channel % 3, start)
            want = pack_ref(*planes)
            seen |= set(bits(want[:h, :w, channel]).ravel().tolist())
            nan_seen |= bool(np.isnan(want[:h, :w, channel]).any())
            assert_packed(gpu_tb.RunNnPack(*planes), want, w, h, 9, "channel %d, from value %d" % (channel, start))
            if channel < 3:
                assert_packed(gpu_tb.RunNnPack(planes[0]), pack_ref(planes[0]), w, h, 3, "3 inputs, channel %d, from value %d" % (channel, start))
    # every class is in what the GPU was held to: both tie directions and signs, the last finite value and infinity of both signs, denormal halves, -0
    assert nan_seen and {p for p in PLANTED_HALVES if p is not None} <= seen, sorted(hex(p) for p in PLANTED_HALVES if p is not None and p not in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_pack_through_the_unorm_store(gpu_tb, w, h):
    """the stage's form: the colour is k / 255 of the 8-bit store (NaN -> 0, clamped), albedo and normals go in as they are"""
    rng = np.random.default_rng(w * 1000 + h + 2)
    albedo, normal = random_surface(rng, w, h), random_surface(rng, w, h)
    color = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(F32)
    values = to8_values()
    levels = set()
    for channel in range(3):
        for start in starts(w * h, values):
            c = plant(color, values, channel, start)
            want = pack_ref(c, albedo, normal, unorm_color=True)
            lv = want[:h, :w, :3].astype(F32)
            assert np.isfinite(lv).all() and lv.min() >= 0 and lv.max() <= 1
            levels |= set(nr.rgba8_of(c)[..., channel].ravel().tolist())
            assert_packed(gpu_tb.RunNnPack(c, albedo, normal, unorm_color=True), want, w, h, 9, "channel %d, from value %d" % (channel, start))
        assert_same(gpu_tb.RunNnPack(plant(color, values, channel, 0), unorm_color=True), pack_ref(plant(color, values, channel, 0), unorm_color=True), "3 inputs")
    assert {0, 255} <= levels and len(levels) > 12
    # the flag reaches the colour only: guides outside [0, 1] and non-finite ones are not clamped
    normal = plant(normal, PLANTED, 2, 0)
    want = pack_ref(color, albedo, normal, unorm_color=True)
    assert (want[:h, :w, 3:9].astype(F32) < 0).any()
    assert_packed(gpu_tb.RunNnPack(color, albedo, normal, unorm_color=True), want, w, h, 9, "guides are not clamped")


# ---- unpack ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_unpack_crops_channels_0_to_2(gpu_tb, w, h):
    rng = np.random.default_rng(w * 1000 + h + 3)
    H0, W0 = h + -h % 16, w + -w % 16
    special = np.array([0x7C00, 0xFC00, 0x7E00, 0x0001, 0x83FF, 0x8000, 0x7BFF], np.uint16).view(F16)    # inf, -inf, NaN, denormals, -0, 65504
    tensor = rng.standard_normal((H0, W0, 32)).astype(F16)                                                  # every channel, and the extension
    assert len(np.unique(bits(tensor))) > min(tensor.size, 8192) // 8                                      # no two neighbours alike, for all practical purposes
    seen = np.zeros((h, w, 3), F32)[:0].reshape(0)
    for start in starts(w * h, special):
        t = tensor.copy()
        for channel in range(3):
            t[:h, :w] = plant(np.ascontiguousarray(t[:h, :w]), special, channel, start + channel)
        want = np.ones((h, w, 4), F32); want[..., :3] = t[:h, :w, :3].astype(F32)
        seen = np.concatenate([seen, want[..., :3].ravel()])
        assert_same(gpu_tb.RunNnUnpack(t, w, h), want, "from value %d" % start)
    assert np.isposinf(seen).any() and np.isneginf(seen).any() and np.isnan(seen).any() and ((seen != 0) & (np.abs(seen) < 2.0 ** -14)).any()


# ---- resolve aux -----------------------------------------------------------------------------------------------------------------------
def guide_sums(rng, w, h, offset):
    """synthetic albedo and normal guide sums that reach every branch of nn_resolve_aux, and the class of each pixel"""
    n = w * h
    A = np.empty((n, 4), F32); N = np.empty((n, 4), F32)
    i = np.arange(n) + offset
    A[:, :3] = rng.uniform(0, 1, (n, 3)) * np.array([1, 3, 2.0 ** 24])[i % 3, None]
    A[:, 3] = np.array([1, 3, 2.0 ** 24], F32)[i % 3]                                   # frames 1, 3 and 2^24
    v = rng.standard_normal((n, 3)).astype(F32)
    kind = i % 9
    N[:, :3] = v
    N[:, 3] = 0                                                                          # kind 0: nothing hit, garbage in .xyz
    one = kind == 1; N[one, :3] = v[one] * F32(2.5) + F32(0.25); N[one, 3] = 1           # one hit: divided by 1, not brought to length 1
    for k, hits in ((2, 2), (3, 3), (4, 7)):                                             # several hits: the mean's direction
        m = kind == k; N[m, :3] = v[m] * F32(hits) * F32(0.8); N[m, 3] = hits
    N[kind == 5] = (0, 0, 0, 2)                                                          # two normals that cancel exactly
    m = kind == 6; N[m, :3] = v[m] * F32(1e-20); N[m, 3] = 2                             # the sum of squares is a float32 denormal
    m = kind == 7; N[m, :3] = v[m] * F32(1e-30); N[m, 3] = 2                             # the sum of squares underflows to 0
    m = kind == 8; N[m, :3] = (1e-40, -3e-41, 0.5); N[m, 3] = 1                          # denormal components, one hit
    return A.reshape(h, w, 4), N.reshape(h, w, 4), kind.reshape(h, w)


def resolve_ref(A, N):
    albedo = np.ones(A.shape, F32)
    with np.errstate(all="ignore"):
        albedo[..., :3] = A[..., :3] / A[..., 3:4]
    normal, _ = guides_ref.resolve(N, np.zeros_like(N))
    return albedo, normal.astype(F32)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_resolve_aux_on_every_branch(gpu_tb, w, h):
    rng = np.random.default_rng(w * 1000 + h + 4)
    reached = set()
    for offset in range(0, 9, min(w * h, 9)):
        A, N, kind = guide_sums(rng, w, h, offset)
        albedo, normal = resolve_ref(A, N)
        length = np.sqrt((normal[..., :3].astype(np.float64) ** 2).sum(-1))
        # each branch does on the reference what its case is there for
        for k in np.unique(kind):
            m = kind == k
            if k in (0, 5, 7):
                assert not normal[m][:, :3].any()
            if k == 1:
                assert (np.abs(length[m] - 1) > 0.05).any() and same(normal[m][:, :3], N[m][:, :3])
            if k in (2, 3, 4, 6):                                # (a denormal sum of squares has some 13 bits: its root is that coarse)
                assert (np.abs(length[m] - 1) < (1e-2 if k == 6 else 1e-6)).all()
            if k == 6:
                q = (N[m][:, :3] / F32(2)) ** 2
                assert ((q.sum(-1) > 0) & (q.sum(-1) < np.finfo(F32).tiny)).all()
            if k == 8:
                assert same(normal[m][:, :3], N[m][:, :3]) and (np.abs(normal[m][:, 0]) < np.finfo(F32).tiny).all() and normal[m][:, 0].all()
            reached.add(int(k))
        assert (normal[..., 3] == 1).all() and (albedo[..., 3] == 1).all() and np.isfinite(albedo).all()
        got_albedo, got_normal = gpu_tb.RunNnResolveAux(A, N)
        assert_same(got_albedo, albedo, "albedo")
        assert_same(got_normal, normal, "normals")
    assert reached == set(range(9))


# ---- to 8-bit --------------------------------------------------------------------------------------------------------------------------
def to8_values():
    """the special values, and for a dozen k the two neighbouring float32 between which x * 255 + 0.5 crosses k + 1"""
    v = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1.0, np.nextafter(F32(1), F32(2)), 1.5]
    for k in (0, 1, 2, 7, 63, 100, 126, 127, 128, 200, 253, 254):
        lo = F32((k + 0.5) / 255)
        level = lambda x: int(F32(F32(x) * F32(255)) + F32(0.5))
        while level(lo) > k:
            lo = np.nextafter(lo, F32(0))
        while level(np.nextafter(lo, F32(2))) == k:
            lo = np.nextafter(lo, F32(2))
        v += [lo, np.nextafter(lo, F32(2))]
    return np.array(v, F32)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_to_rgba8_on_edges_and_crossings(gpu_tb, w, h):
    rng = np.random.default_rng(w * 1000 + h + 5)
    values = to8_values()
    picture = rng.uniform(-0.5, 1.5, (h, w, 4)).astype(F32)
    for channel in range(3):
        for start in starts(w * h, values):
            p = plant(picture, values, channel, start)
            assert_same(gpu_tb.RunNnToRgba8(p), nr.rgba8_of(p), "channel %d, from value %d" % (channel, start))
    # on the reference: the specials, and each crossing is one: k below, k + 1 above
    p = np.zeros((1, len(values), 4), F32); p[0, :, 2] = values
    want = nr.rgba8_of(p)[0, :, 2].tolist()
    assert want[:9] == [0, 255, 0, 0, 0, 0, 255, 255, 255]
    assert want[9:] == [k + d for k in (0, 1, 2, 7, 63, 100, 126, 127, 128, 200, 253, 254) for d in (0, 1)]
    assert_same(gpu_tb.RunNnToRgba8(p), nr.rgba8_of(p), "the values in a row")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hooks_refuse_bad_arguments(gpu_tb):
    L, ctx = gpu_tb._L, gpu_tb._ctx
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    f = [np.zeros((4, 4, 4), F32) for _ in range(4)]
    t = np.zeros((16, 16, 32), F16)
    b = np.zeros((4, 4, 4), np.uint8)
    big = (1 << 13, (1 << 11) + 1)                           # 2^24 + 2^13 pixels; refused before anything is read

    def refused(rc, word):
        assert rc == TB_E_INVALID, rc
        message = L.tb_last_error(ctx).decode()
        assert word in message, message

    pack = lambda w, h, pw, ph, color, albedo, normal, out: L.tb_run_nn_pack(ctx, w, h, pw, ph, 0, *[None if a is None else ptr(a) for a in (color, albedo, normal, out)])
    assert pack(4, 4, 16, 16, f[0], f[1], f[2], t) == 0 and pack(4, 4, 16, 16, f[0], None, None, t) == 0
    refused(pack(4, 4, 16, 16, None, f[1], f[2], t), "null")
    refused(pack(4, 4, 16, 16, f[0], f[1], f[2], None), "null")
    refused(pack(4, 4, 16, 16, f[0], f[1], None, t), "together")
    refused(pack(4, 4, 16, 16, f[0], None, f[2], t), "together")
    refused(pack(0, 4, 16, 16, f[0], None, None, t), "0")
    refused(pack(4, 0, 16, 16, f[0], None, None, t), "0")
    refused(pack(*big, *big, f[0], None, None, t), "2^24")
    refused(pack(4096, 4096, 4096, 4112, f[0], None, None, t), "2^24")       # the picture fits, its extension does not
    refused(pack(4, 4, 3, 16, f[0], None, None, t), "smaller")
    refused(pack(4, 4, 16, 3, f[0], None, None, t), "smaller")

    unpack = lambda w, h, pw, ph, tensor, out: L.tb_run_nn_unpack(ctx, w, h, pw, ph, *[None if a is None else ptr(a) for a in (tensor, out)])
    assert unpack(4, 4, 16, 16, t, f[0]) == 0
    refused(unpack(4, 4, 16, 16, None, f[0]), "null")
    refused(unpack(4, 4, 16, 16, t, None), "null")
    refused(unpack(0, 4, 16, 16, t, f[0]), "0")
    refused(unpack(4, 0, 16, 16, t, f[0]), "0")
    refused(unpack(*big, *big, t, f[0]), "2^24")
    refused(unpack(4096, 4096, 4112, 4096, t, f[0]), "2^24")
    refused(unpack(4, 4, 3, 16, t, f[0]), "smaller")
    refused(unpack(4, 4, 16, 3, t, f[0]), "smaller")

    resolve = lambda w, h, *arrays: L.tb_run_nn_resolve_aux(ctx, w, h, *[None if a is None else ptr(a) for a in arrays])
    assert resolve(4, 4, *f) == 0
    for i in range(4):
        refused(resolve(4, 4, *[None if j == i else a for j, a in enumerate(f)]), "null")
    refused(resolve(0, 4, *f), "0")
    refused(resolve(4, 0, *f), "0")
    refused(resolve(*big, *f), "2^24")

    to8 = lambda w, h, picture, out: L.tb_run_nn_to_rgba8(ctx, w, h, *[None if a is None else ptr(a) for a in (picture, out)])
    assert to8(4, 4, f[0], b) == 0
    refused(to8(4, 4, None, b), "null")
    refused(to8(4, 4, f[0], None), "null")
    refused(to8(0, 4, f[0], b), "0")
    refused(to8(4, 0, f[0], b), "0")
    refused(to8(*big, f[0], b), "2^24")
    assert gpu_tb.RunNnToRgba8(np.ones((2, 3, 4), F32)).tolist() == [[[255] * 4] * 3] * 2      # the context works afterwards


def test_new_entry_points_exist(built):
    """the four hooks: declared in the header, exported, bound in ctypes, wrapped"""
    import os
    import re
    from conftest import ROOT
    from tracerboy_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracerboy_hip.h")).read(), flags=re.S)
    raw, bound = C.CDLL(api.LIB_PATH), api.lib()
    for name in ("tb_run_nn_pack", "tb_run_nn_unpack", "tb_run_nn_resolve_aux", "tb_run_nn_to_rgba8"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in bound._tb_exports and getattr(bound, name).argtypes is not None, name
    assert all(callable(getattr(api.TracerBoy, n)) for n in ("RunNnPack", "RunNnUnpack", "RunNnResolveAux", "RunNnToRgba8"))
