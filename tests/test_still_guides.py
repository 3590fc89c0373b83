"""The guide pass of a denoised still: first hits traced again by a kernel of their own, summed over frames, and the denoise
chains that read the sums (option "denoise_guides" = 1: normals and positions; 2: 1 + albedo demodulation).

CPU part (-m "not gpu"): the entry points exist; identities of the NumPy restatement (tests/still_guides_ref.py); the claim of mode 2 on the
oracle -- relMSE(mode 2) <= relMSE(section 12's chain) on material-maps, no margin.
GPU part (-m gpu): every comparison is on bits -- the guide surfaces against the restatement fed with the oracle's per-frame AOVs, the chains
against the restatement fed with the device's own surfaces, mode 1 against section 12 itself; the render is left alone; states; refusals; the
command-line tool."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import still_denoise_ref as ref
import still_guides_ref as gref
from conftest import CORNELL, GOLDEN, ROOT
from test_still_denoise import CLI, assert_stages, bits, denoiser, same

F32 = np.float32
TB_E_INVALID, TB_E_UNSUPPORTED = -1, -6
SCENES = {name: os.path.join(GOLDEN, "scenes", name, "scene.pbrt") for name in ("cornell-box", "material-maps", "mix-glass", "instances", "Teapot")}
W, H = 100, 70                                                  # ragged against the 16 x 16 regions and the 256-pixel workgroups


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_exist(built):
    """tb_render_guides, tb_read_guide and option denoise_guides: declared, exported, bound in ctypes, wrapped."""
    from tracerboy_amd import _ctypes_abi as abi, api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracerboy_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(api.LIB_PATH)
    bound = api.lib()
    for name in ("tb_render_guides", "tb_read_guide"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert getattr(bound, name).argtypes is not None, name
    assert b"denoise_guides\0" in open(api.LIB_PATH, "rb").read() and b"last_guides_us\0" in open(api.LIB_PATH, "rb").read()
    assert callable(api.TracerBoy.RenderGuides) and callable(api.TracerBoy.ReadGuide)
    assert (abi.TB_GUIDE_ALBEDO, abi.TB_GUIDE_NORMAL, abi.TB_GUIDE_POSITION) == (0, 1, 2)


@pytest.fixture(scope="module")
def s4(built, settings):
    s = copy.copy(settings); s.MaxBounces = 4; s.EnableBlueNoise = 0
    return s


def test_restatement_identities(built, cornell_host, s4):
    """One frame: the resolved guides are that frame's oracle AOVs.  A constant effective albedo of 1: mode 2's stages are mode 1's.  No filter
    pass: stage 3 is ((o / n) / d) * d."""
    w, h = 64, 48
    view, pf = cornell_host.view(), cornell_host.frame_constants(s4, 0, 0.0)
    frames = [gref.oracle_frame(view, pf, w, h, f) for f in (5, 6)]
    low = ol.render(view, pf, w, h, 2, first_frame=5, threads=8, jittered=True)
    o, q = low["output"], low["jittered"]
    for normal, albedo, position in frames:
        A, N, P = gref.guide_sums([(normal, albedo, position)])
        normals, positions = gref.resolve(N, P)
        hit = normal[..., :3].any(-1)
        assert hit.any() and not hit.all()
        assert same(normals, normal)
        assert same(positions[hit], position[hit]) and not positions[~hit].any()
        assert same(A[..., :3], np.where(albedo[..., :3].any(-1)[..., None], albedo[..., :3], F32(1))) and np.all(A[..., 3] == 1)
    A, N, P = gref.guide_sums(frames)
    assert np.all(A[..., 3] == 2) and set(np.unique(N[..., 3])) <= {0.0, 1.0, 2.0}
    flat = np.full_like(A, 2)                                    # effective albedo 1 in both frames
    assert np.all(gref.demod(flat) == 1)
    one, two = gref.chain(o, q, flat, N, P, 7, denoiser(3), 1), gref.chain(o, q, flat, N, P, 7, denoiser(3), 2)
    assert all(same(a, b) for a, b in zip(one, two))
    none = gref.chain(o, q, A, N, P, 7, denoiser(0), 2)
    d = gref.demod(A)
    assert none[2] is None
    assert same(none[3][..., :3], ((o[..., :3] / o[..., 3:4]) / d) * d) and np.all(none[3][..., 3] == 1)


def test_demodulation_does_not_lose_to_section_12_on_an_albedo_texture(built, s4):
    """The claim of mode 2.  material-maps (albedo texture) 128 x 96, 16 spp, MaxBounces 4, blue noise off, time seed 0, default filter settings,
    guides over K = 16 frames; truth: the oracle's frames [4096, 5120).  relMSE(mode 2) <= relMSE(section 12's chain on the same 16 frames), no
    margin.  cornell-box (no albedo detail) and mode 1 at K = 1 / 8 / 16 are reported, and finite; the values measured are in DESIGN.md
    section 13."""
    from tracerboy_amd import api
    w, h, spp = 128, 96, 16
    dn = api.GetDefaultDenoiserSettings()
    for name in ("material-maps", "cornell-box"):
        host = api.HostScene(SCENES[name])
        view, pf = host.view(), host.frame_constants(s4, 0, 0.0)
        low = ol.render(view, pf, w, h, spp, first_frame=0, threads=8, jittered=True, aovs=True)
        truth = ol.render(view, pf, w, h, 1024, first_frame=4096, threads=8)["output"]
        truth = truth[..., :3] / truth[..., 3:4]
        frames = [gref.oracle_frame(view, pf, w, h, f) for f in range(spp)]
        positions = low["worldpos1"] if (spp - 1) % 2 else low["worldpos0"]
        base = ref.chain(low["output"], low["jittered"], low["normals"], positions, spp, dn)
        twelve = ref.rel_mse(base[3], truth)
        print("%s: relMSE raw %.6f, section 12 %.6f" % (name, ref.rel_mse(base[0], truth), twelve))
        for k in (1, 8, 16):
            A, N, P = gref.guide_sums(frames[spp - k:])
            one = gref.chain(low["output"], low["jittered"], A, N, P, spp, dn, 1)[3]
            print("%s: mode 1, K = %d: relMSE %.6f" % (name, k, ref.rel_mse(one, truth)))
            assert np.all(np.isfinite(one))
        two = gref.chain(low["output"], low["jittered"], A, N, P, spp, dn, 2)[3]
        demodulated = ref.rel_mse(two, truth)
        print("%s: mode 2, K = 16: relMSE %.6f" % (name, demodulated))
        assert np.all(np.isfinite(two))
        if name == "material-maps":
            assert demodulated <= twelve


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s3(built, settings):
    s = copy.copy(settings); s.MaxBounces = 3; s.EnableBlueNoise = 0
    return s


def context(scene, **opts):
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    for k, v in opts.items():
        tb.SetOption(k, v)
    tb.LoadScene(scene)
    return tb


@pytest.fixture(scope="module")
def aov_tb(built):
    tb = context(CORNELL, aov=1)
    yield tb
    tb.close()


@pytest.fixture(scope="module")
def plain_tb(built):
    """option "aov" off: the render at full speed"""
    tb = context(CORNELL)
    yield tb
    tb.close()


def guides(tb):
    return [tb.ReadGuide(k) for k in range(3)]


def read_stages(tb):
    return [tb.ReadDenoiseStage(k) for k in range(4)]


@pytest.fixture(scope="module")
def section12(aov_tb, s3):
    """context A of the equivalence: option "aov" on, frames [0, 4), tb_denoise as section 12 has it -- the four stages"""
    aov_tb.InvalidateHistory()
    aov_tb.Render(W, H, 4, s3, 0.0)
    aov_tb.SetOption("denoise_guides", 0)
    aov_tb.Denoise(denoiser(5), read=False)
    return read_stages(aov_tb)


@pytest.mark.gpu
def test_gpu_one_frame_equals_the_aovs(aov_tb, s3):
    tb = aov_tb
    tb.InvalidateHistory()
    tb.Render(W, H, 3, s3, 0.0)
    tb.RenderGuides(2, 1)
    albedo, normal, position = guides(tb)
    n, p, a = tb.ReadAOV(2), tb.ReadAOV(3 + 2 % 2), tb.ReadAOV(5)
    hit = n[..., :3].any(-1)
    print("pixels that hit: %d of %d; without an albedo: %d" % (int(hit.sum()), W * H, int((~a[..., :3].any(-1)).sum())))
    assert hit.any() and not hit.all() and not a[..., :3].any(-1).all()
    assert same(normal[..., :3], n[..., :3]) and same(normal[..., 3], hit.astype(F32))
    assert same(position[hit], p[hit]) and not position[~hit].any()
    assert same(albedo[..., :3], np.where(a[..., :3].any(-1)[..., None], a[..., :3], F32(1))) and np.all(albedo[..., 3] == 1)
    assert tb.GetOption("last_guides_us") > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_gpu_sums_equal_the_oracle(built, s3, name):
    """Frames [2, 7) -- five frames, odd and even, not from 0 -- at 100 x 70, and frame 2 alone at 20 x 12 (one partial row of regions): the three
    guide surfaces against the restatement fed with the oracle's per-frame AOVs.  instances: the two-level walk.  Teapot (no camera ray misses at its
    own camera: the other scenes have the pixels no frame hits) also with part of the stack in global memory."""
    tb = context(SCENES[name], **({"flatten_instances": 0} if name == "instances" else {}))
    try:
        view = tb.HostSceneView()
        for w, h, first, n in ((W, H, 2, 5), (20, 12, 2, 1)):
            tb.BeginAccumulation(w, h, s3, 0.0, first_frame=0)   # a size, settings and a time seed; nothing is rendered
            tb.RenderGuides(first, n)
            pf = tb.FrameConstants(w, h, 0, s3, 0.0)
            want = gref.guide_sums([gref.oracle_frame(view, pf, w, h, f) for f in range(first, first + n)])
            got = guides(tb)
            print("%s %d x %d: pixels no frame hit %d, some but not all %d" % (name, w, h, int((want[1][..., 3] == 0).sum()),
                                                                             int(((want[1][..., 3] > 0) & (want[1][..., 3] < n)).sum())))
            for k, what in enumerate(("albedo", "normal", "position")):
                bad = (bits(got[k]) != bits(want[k])).any(-1)
                assert not bad.any(), "%s %d x %d: guide %s differs in %d pixels, first at %s: %s, restatement %s" % (
                    name, w, h, what, int(bad.sum()), np.argwhere(bad)[0], got[k][tuple(np.argwhere(bad)[0])], want[k][tuple(np.argwhere(bad)[0])])
            assert tb.GetNumberOfSamplesSinceLastInvalidate() == 0 and tb.GetOption("last_guides_stack_overflow") == 0
        if name == "Teapot":                                     # a tree 28 deep with 20 entries of the stack in LDS: the split-stack form of the kernel
            tb.SetOption("stack_lds_cap", 20)
            tb.RenderGuides(first, n)
            assert tb.GetOption("last_guides_stack_overflow") == 8
            assert all(same(a, b) for a, b in zip(guides(tb), got))
    finally:
        tb.close()


@pytest.mark.gpu
def test_gpu_guides_leave_the_render_alone(aov_tb, s3):
    tb = aov_tb
    tb.InvalidateHistory()
    tb.Render(W, H, 3, s3, 0.0)
    digest, aovs = tb.AccumDigest(), [tb.ReadAOV(k) for k in range(2, 8)]
    tb.RenderGuides(1, 2)
    assert tb.AccumDigest() == digest and tb.GetNumberOfSamplesSinceLastInvalidate() == 3
    assert all(same(a, tb.ReadAOV(k)) for a, k in zip(aovs, range(2, 8)))
    tb.Render(W, H, 4, s3, 0.0)
    interrupted = tb.AccumDigest(), tb.ReadAccumulation(jittered=True)
    tb.InvalidateHistory()
    tb.Render(W, H, 3, s3, 0.0)
    tb.Render(W, H, 4, s3, 0.0)
    straight = tb.ReadAccumulation(jittered=True)
    assert tb.AccumDigest() == interrupted[0]
    assert same(straight[0], interrupted[1][0]) and same(straight[1], interrupted[1][1])


@pytest.mark.gpu
def test_gpu_mode_1_reproduces_section_12(section12, plain_tb, s3):
    """B: option "aov" off, the same four frames, the guides of frame 3 alone, mode 1: all four stages are A's."""
    tb = plain_tb
    tb.InvalidateHistory()
    tb.Render(W, H, 4, s3, 0.0)
    assert tb.GetOption("last_variant") != 4                     # not the full feature set: the render ran without AOVs
    tb.RenderGuides(3, 1)
    tb.SetOption("denoise_guides", 1)
    try:
        final = tb.Denoise(denoiser(5))
    finally:
        tb.SetOption("denoise_guides", 0)
    assert_stages(tb, section12, "mode 1 against section 12")
    assert same(final, section12[3])


def assert_mode(tb, mode, dn, what):
    """tb_denoise in `mode` against the restatement fed with the device's own surfaces and guides"""
    frames = tb.GetNumberOfSamplesSinceLastInvalidate()
    o, q = tb.ReadAccumulation(jittered=True)
    A, N, P = guides(tb)
    tb.SetOption("denoise_guides", mode)
    try:
        final = tb.Denoise(dn)
    finally:
        tb.SetOption("denoise_guides", 0)
    want = gref.chain(o, q, A, N, P, frames, dn, mode)
    assert_stages(tb, want, what)
    assert same(final, want[3]) and np.all(final[..., 3] == 1.0)
    return A, N, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["material-maps", "Teapot"])
def test_gpu_mode_2_equals_the_restatement(built, s3, name):
    tb = context(SCENES[name])
    try:
        tb.Render(W, H, 6, s3, 0.0)
        tb.RenderGuides(2, 4)
        A, N, want = assert_mode(tb, 2, denoiser(5), name + " mode 2")
        assert_mode(tb, 1, denoiser(5), name + " mode 1")
        print("%s: mean effective albedo %.4f ... %.4f" % (name, float((A[..., :3] / A[..., 3:4]).min()), float((A[..., :3] / A[..., 3:4]).max())))
        assert np.all(np.isfinite(want[3]))
    finally:
        tb.close()


@pytest.mark.gpu
def test_gpu_mode_2_on_a_zero_channel_and_on_no_hit_at_all(built, s3):
    """cornell-box with the green of every albedo set to 0: d is held at 0.01 there.  Then the camera taken out of the box and turned away: no frame hits anywhere, the
    effective albedo is 1, every pixel keeps its mean."""
    tb = context(CORNELL)
    try:
        i = 0
        while tb.IsMaterialIDValid(i):
            m = tb.GetMaterial(i); m.albedo.y = 0.0; tb.SetMaterial(i, m); i += 1
        tb.Render(W, H, 4, s3, 0.0)
        tb.RenderGuides(0, 4)
        A, N, want = assert_mode(tb, 2, denoiser(5), "zero channel")
        lit = A[..., 0] != A[..., 3]
        assert lit.any() and np.all(A[..., 1][lit & (N[..., 3] == 4)] < 4)    # green sums only the frames that count as 1
        assert (gref.demod(A)[..., 1] == F32(0.01)).any()
        cam = tb.GetCamera()
        for k in range(3):                                       # a hundred view vectors back from the box, facing the other way
            d = cam.LookAt[k] - cam.Position[k]
            cam.Position[k] -= 100.0 * d
            cam.LookAt[k] = cam.Position[k] - d
        tb.SetCamera(cam)
        tb.Render(W, H, 4, s3, 0.0)
        tb.RenderGuides(0, 4)
        A, N, want = assert_mode(tb, 2, denoiser(5), "no hit")
        assert not N.any() and np.all(A == 4)
        assert same(want[3][..., :3], want[0][..., :3])
    finally:
        tb.close()


@pytest.mark.gpu
def test_gpu_guides_after_a_state(section12, plain_tb, s3, tmp_path):
    """Saved at frame 4, loaded into a fresh context, nothing rendered: section 12 refuses as it did, the guide pass + mode 1 gives section 12's
    result of the straight render."""
    from tracerboy_amd import api
    plain_tb.InvalidateHistory()
    plain_tb.Render(W, H, 4, s3, 0.0)
    path = str(tmp_path / "four.tbs")
    plain_tb.SaveState(path)
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.LoadState(path)
        with pytest.raises(api.TracerBoyError) as e:
            tb.Denoise(denoiser(5))
        assert e.value.code == TB_E_INVALID and "tb_state_load" in str(e.value)
        tb.SetOption("denoise_guides", 1)
        with pytest.raises(api.TracerBoyError) as e:
            tb.Denoise(denoiser(5))
        assert e.value.code == TB_E_INVALID and "tb_render_guides" in str(e.value)
        tb.RenderGuides(3, 1)
        final = tb.Denoise(denoiser(5))
        assert_stages(tb, section12, "after tb_state_load")
        assert same(final, section12[3])
        assert tb.GetNumberOfSamplesSinceLastInvalidate() == 4


@pytest.mark.gpu
def test_gpu_guide_refusals_and_invalidation(built, s3, tmp_path):
    from tracerboy_amd import api

    def refused(call, code, word):
        with pytest.raises(api.TracerBoyError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    with api.TracerBoy(0) as tb:
        tb.width, tb.height = 32, 24
        refused(lambda: tb.RenderGuides(0, 1), TB_E_INVALID, "no scene")
        tb.LoadScene(CORNELL)
        refused(lambda: tb.RenderGuides(0, 1), TB_E_INVALID, "no size")
        refused(lambda: tb.SetOption("denoise_guides", 3), TB_E_INVALID, "denoise_guides")
        tb.Render(32, 24, 2, s3, 0.0)
        refused(lambda: tb.RenderGuides(0, 0), TB_E_INVALID, "n_frames")
        refused(lambda: tb.RenderGuides(0, 257), TB_E_INVALID, "n_frames")
        refused(lambda: tb.ReadGuide(0), TB_E_INVALID, "tb_render_guides")
        refused(lambda: tb.ReadGuide(3), TB_E_INVALID, "which")
        tb.RenderGuides(1000, 256)                               # any range, the longest pass
        assert np.all(tb.ReadGuide(0)[..., 3] == 256)
        for output_type, word in ((9, "heat map"), (7, "live pixels")):
            s = copy.copy(s3); s.OutputType = output_type
            tb.Render(32, 24, 1, s, 0.0)
            refused(lambda: tb.RenderGuides(0, 1), TB_E_INVALID, word)
        tb.RenderRealTime(32, 24, s3, None, 0.0)
        refused(lambda: tb.RenderGuides(0, 1), TB_E_INVALID, "tb_render_realtime")
        # validity
        tb.Render(32, 24, 2, s3, 0.0)
        tb.RenderGuides(0, 2)
        tb.SetOption("denoise_guides", 1)
        tb.Denoise(read=False)
        tb.Render(32, 24, 4, s3, 0.0)                            # four more frames: still valid
        tb.Denoise(read=False); tb.ReadGuide(1)
        cam = tb.GetCamera()
        tb.SetCamera(cam)                                        # resets the history
        tb.Render(32, 24, 2, s3, 0.0)
        refused(lambda: tb.Denoise(), TB_E_INVALID, "tb_render_guides")
        refused(lambda: tb.ReadGuide(1), TB_E_INVALID, "tb_render_guides")
        tb.RenderGuides(0, 2)
        tb.Denoise(read=False)
        tb.Render(48, 24, 2, s3, 0.0)                            # a resize
        refused(lambda: tb.Denoise(), TB_E_INVALID, "tb_render_guides")
        tb.RenderGuides(0, 2)
        assert tb.ReadGuide(2).shape == (24, 48, 4)
        tb.SetOption("denoise_guides", 0)
        tb.SetTileAssignment(0, 2)
        tb.Render(128, 64, 1, s3, 0.0)
        refused(lambda: tb.RenderGuides(0, 1), TB_E_UNSUPPORTED, "tile assignment")
    with api.TracerBoy(devices=[0, 0]) as g:                     # a two-member group on one device
        g.LoadScene(CORNELL)
        g.Render(64, 64, 1, s3, 0.0)
        refused(lambda: g.RenderGuides(0, 1), TB_E_UNSUPPORTED, "group")


@pytest.mark.gpu
def test_cli_denoise_guides(section12, tmp_path):
    from test_render_state import read_pfm
    out, state = str(tmp_path / "f.pfm"), str(tmp_path / "s.tbs")
    common = [CLI, CORNELL, "--width", str(W), "--height", str(H), "--depth", "3", "--blue-noise", "0"]
    r = subprocess.run(common + ["--spp", "4", "--denoise-guides", "1", "--save-state", state, "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "guides: first hits of frames [3, 4)" in r.stdout, r.stdout + r.stderr
    assert same(read_pfm(out), section12[3][..., :3])
    resumed = str(tmp_path / "r.pfm")                            # no frame left to render
    r = subprocess.run([CLI, CORNELL, "--resume", state, "--denoise", "--denoise-guides", "2", "--denoise-demodulate", "--out", resumed],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "guides: first hits of frames [2, 4)" in r.stdout and os.path.exists(resumed), r.stdout + r.stderr
    r = subprocess.run(common + ["--spp", "2", "--denoise-demodulate", "--out", str(tmp_path / "d.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--denoise-guides" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(common + ["--spp", "2", "--ranks", "2", "--denoise-guides", "1", "--out", str(tmp_path / "n.pfm")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--denoise" in r.stderr and not os.path.exists(str(tmp_path / "n.pfm")), r.stdout + r.stderr
