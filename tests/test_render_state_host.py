"""Render-state files without a GPU: the digest of include/tb_state.h against a numpy restatement, the file format's
round trip, every malformed file an error code and a message, the scene digest, and the existing kernels' listings unchanged."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, GOLDEN

TEAPOT = os.path.join(GOLDEN, "scenes", "Teapot", "scene.pbrt")
HEADER = 256
M64 = (1 << 64) - 1


def np_digest(a):
    """sum over i of fmix64((i << 32) | w[i]) mod 2^64, w = the bytes as 32-bit words."""
    w = np.ascontiguousarray(a).view(np.uint32).ravel().astype(np.uint64)
    with np.errstate(over="ignore"):
        k = (np.arange(w.size, dtype=np.uint64) << np.uint64(32)) | w
        k ^= k >> np.uint64(33); k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33); k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
        return int(k.sum(dtype=np.uint64)) & M64


def payload(n_words, seed):
    """float32 words with the values a digest must tell apart: -0, denormals, +-inf, two NaNs with different payloads, ordinary sums."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0x3d000000, 0x44000000, n_words, dtype=np.uint32)      # ordinary positive floats
    special = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00001, 0x7fc12345, 0x00000000], np.uint32)
    k = min(n_words, special.size)
    if k:
        u[rng.permutation(n_words)[:k]] = special[:k]
    return u.view(np.float32)


def default_info(first=0, next_frame=3, scene_digest=0, **kw):
    from tracerboy_amd import _ctypes_abi as abi, api
    h = abi.tb_state_info()
    h.first_frame, h.next_frame, h.time_seed = first, next_frame, 0.0
    h.settings = api.GetDefaultOutputSettings()
    h.tile_rank, h.tile_world, h.tile_w, h.tile_h = 0, 1, 64, 64
    h.adaptive_min_frames = 1024
    h.scene_digest = scene_digest
    for k, v in kw.items():
        setattr(h, k, v)
    return h


@pytest.mark.parametrize("n", [0, 1, 4, 255, 256, 257])
def test_digest_known_answers(built, n):
    from tracerboy_amd import api
    a = payload(n, 11 + n)
    assert api.StateDigest(a) == np_digest(a)
    if n == 0:
        assert api.StateDigest(a) == 0
    if n == 1:                                                  # the one term, in Python integers
        k = int(a.view(np.uint32)[0])                           # index 0: (0 << 32) | w
        k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M64; k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M64; k ^= k >> 33
        assert api.StateDigest(a) == k


def test_digest_of_a_surface_sees_bits_and_places(built):
    from tracerboy_amd import api
    a = payload(70 * 50 * 4, 5).reshape(50, 70, 4)
    d = api.StateDigest(a)
    assert d == np_digest(a)
    u = a.view(np.uint32).ravel()
    i, j = [int(x) for x in np.flatnonzero(u != u[0])[:2]]     # two unequal words trade places
    assert u[i] != u[j]
    b = u.copy(); b[i], b[j] = u[j], u[i]
    assert api.StateDigest(b.view(np.float32)) != d
    z = u.copy(); z[int(np.flatnonzero(u == 0x80000000)[0])] = 0   # -0 is not +0
    assert api.StateDigest(z.view(np.float32)) != d
    p = u.copy(); p[int(np.flatnonzero(u == 0x7fc00001)[0])] = 0x7fc00002   # another NaN payload
    assert api.StateDigest(p.view(np.float32)) != d


@pytest.mark.parametrize("W,H", [(1, 1), (70, 50)])
def test_file_round_trip(built, tmp_path, W, H):
    from tracerboy_amd import api
    out = payload(W * H * 4, 1).reshape(H, W, 4); jit = payload(W * H * 4, 2).reshape(H, W, 4)
    h = default_info(first=7, next_frame=12, scene_digest=0x0123456789abcdef, time_seed=2.5, tile_rank=1, tile_world=3, tile_w=32, tile_h=16,
                     alpha_test=1, adaptive=1, adaptive_test=1, adaptive_min_frames=(1 << 33) + 5)
    h.settings.MaxBounces = 9; h.settings.ConvergencePercentage = 0.125; h.settings.EnableBlueNoise = 0
    h.camera.Position[:] = [1.0, 2.0, 3.0]; h.camera.Up[:] = [0.0, 1.0, 0.0]; h.camera.LensHeight = 2.0; h.camera.FocalDistance = 7.0
    path = str(tmp_path / "s.tbs")
    api.WriteStateFile(path, h, out, jit)
    assert os.path.getsize(path) == HEADER + 2 * W * H * 16
    assert sorted(os.listdir(tmp_path)) == ["s.tbs"]            # written beside and renamed: nothing else is left
    info = api.StateInfo(path)
    got, gout, gjit = api.ReadStateFile(path)
    for g in (info, got):
        assert (g.version, g.width, g.height, g.first_frame, g.next_frame, g.time_seed) == (1, W, H, 7, 12, 2.5)
        assert bytes(g.settings) == bytes(h.settings) and bytes(g.camera) == bytes(h.camera)
        assert (g.tile_rank, g.tile_world, g.tile_w, g.tile_h) == (1, 3, 32, 16)
        assert (g.alpha_test, g.adaptive, g.adaptive_test, g.adaptive_min_frames) == (1, 1, 1, (1 << 33) + 5)
        assert g.scene_digest == 0x0123456789abcdef
        assert (g.output_digest, g.jittered_digest) == (np_digest(out), np_digest(jit))
    assert np.array_equal(gout.view(np.uint32), out.view(np.uint32)) and np.array_equal(gjit.view(np.uint32), jit.view(np.uint32))
    raw = open(path, "rb").read()
    assert raw[:8] == b"TBSTATE1" and raw[HEADER:HEADER + W * H * 16] == out.tobytes() and raw[HEADER + W * H * 16:] == jit.tobytes()


def test_malformed_files_are_codes_and_messages(built, tmp_path, monkeypatch):
    from tracerboy_amd import _ctypes_abi as abi, api
    monkeypatch.chdir(tmp_path)
    W, H = 5, 3
    out = payload(W * H * 4, 3).reshape(H, W, 4); jit = payload(W * H * 4, 4).reshape(H, W, 4)
    api.WriteStateFile("good.tbs", default_info(), out, jit)
    good = open("good.tbs", "rb").read()
    api.ReadStateFile("good.tbs")

    def refused(name, data, code, word, info_too=True):
        open(name, "wb").write(data)
        for reader in ([api.StateInfo] if info_too else []) + [api.ReadStateFile]:
            with pytest.raises(api.TracerBoyError) as e:
                reader(name)
            assert e.value.code == code and word in str(e.value), (name, str(e.value))

    with pytest.raises(api.TracerBoyError) as e:
        api.StateInfo("missing.tbs")
    assert e.value.code == -3
    refused("magic.tbs", b"TBSTATEX" + good[8:], -4, "magic")
    refused("version.tbs", good[:8] + (2).to_bytes(4, "little") + good[12:], -4, "version")
    refused("cut1.tbs", good[:-1], -4, "truncated")
    refused("cut_header.tbs", good[:HEADER], -4, "truncated")
    refused("cut_in_header.tbs", good[:100], -4, "truncated")
    refused("longer.tbs", good + b"\0", -4, "too long")
    flipped = bytearray(good); flipped[HEADER + 17] ^= 0x10
    refused("flip_output.tbs", bytes(flipped), -4, "output_digest", info_too=False)
    flipped = bytearray(good); flipped[-1] ^= 0x80
    refused("flip_jittered.tbs", bytes(flipped), -4, "jittered_digest", info_too=False)
    api.StateInfo("flip_jittered.tbs")                          # the header alone is fine
    # sizes: a product that overflows 32 and 64 bits, a side past 16384, a zero side -- refused on the header, before anything is sized
    off_w = 8 + abi.tb_state_info.width.offset
    for w, h in [(0xffffffff, 0xffffffff), (0x10000, 0x10000), (16385, 1), (1, 16385), (0, 3)]:
        bad = good[:off_w] + w.to_bytes(4, "little") + h.to_bytes(4, "little") + good[off_w + 8:]
        refused("size.tbs", bad, -4, "width / height")
    off_tw = 8 + abi.tb_state_info.tile_world.offset
    refused("tiles.tbs", good[:off_tw] + (0).to_bytes(4, "little") + good[off_tw + 4:], -4, "tile assignment")
    off_first = 8 + abi.tb_state_info.first_frame.offset
    refused("range.tbs", good[:off_first] + (9).to_bytes(4, "little") + good[off_first + 4:], -4, "first_frame")
    # the writer refuses what the reader would
    with pytest.raises(api.TracerBoyError) as e:
        api.WriteStateFile("bad.tbs", default_info(first=4, next_frame=3), out, jit)
    assert e.value.code == -1 and not os.path.exists("bad.tbs")
    with pytest.raises(api.TracerBoyError) as e:
        api.WriteStateFile(os.path.join("no_such_dir", "s.tbs"), default_info(), out, jit)
    assert e.value.code == -3


def test_host_scene_digest(built):
    from tracerboy_amd import api
    a, b = api.HostScene(CORNELL), api.HostScene(CORNELL)
    assert a.digest() == b.digest() != 0
    assert api.HostScene(CORNELL, bvh_builder=1).digest() != a.digest()
    assert api.HostScene(TEAPOT).digest() != a.digest()


def _listing_hash(src):
    """sha256 of the device listing of one kernel unit, compiled with the build's own flags from the repository root with relative paths (so that
    no path of the checkout reaches the text); the assembler's .file / .ident lines left out."""
    from tracerboy_amd import build as B
    common = [f for f in B.COMMON if not f.startswith("-I")] + ["-I" + os.path.relpath(os.path.join(B.REPO, "include"), B.REPO)]
    cmd = [B.HIPCC] + common + B.device_flags(src) + ["--cuda-device-only", "-S", os.path.relpath(os.path.join(B.CSRC, src), B.REPO), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=B.REPO)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if not l.lstrip().startswith((".file", ".ident"))]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _compiler_version():
    from tracerboy_amd import build as B
    out = subprocess.run([B.HIPCC, "--version"], capture_output=True, text=True).stdout
    return "\n".join(l.strip() for l in out.splitlines() if "version" in l)


def test_existing_kernels_unchanged(built):
    """The render path's device code is what it was before render states: the listing of pt_variant_matte.hip hashes to the value recorded from
    the parent commit's build (tests/golden/state_kernel_listings.json holds all units' hashes and the compiler they were taken with)."""
    rec = json.load(open(os.path.join(GOLDEN, "state_kernel_listings.json")))
    if rec["compiler"] != _compiler_version():
        pytest.skip("the parent build's listings were recorded with another compiler (%s): no listing to compare with" % rec["compiler"].splitlines()[0])
    src = "kernels/pt_variant_matte.hip"
    assert _listing_hash(src) == rec["parent_listing_sha256"][src]
