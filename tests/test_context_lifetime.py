"""-m gpu: a context gives back every device byte it took.  Option "debug_live_device_bytes" reads the library's own count of the device
memory it holds (added where it allocates, taken back where DevBuf frees; every context of the process together).  It is exact and does not
depend on other processes, which hipMemGetInfo on a shared device would.  Each test makes a fresh context beside the session's, runs one path
through it, destroys it and asks for the count it found -- to the byte."""
import copy
import os

import pytest

from conftest import CORNELL, GOLDEN

pytestmark = pytest.mark.gpu
TEAPOT = os.path.join(GOLDEN, "scenes", "Teapot", "scene.pbrt")


def live(tb):
    return tb.GetOption("debug_live_device_bytes")


def _fresh_context_round_trip(gpu_tb, exercise, devices=None):
    """The count before a fresh context (or group, over `devices`) is made, the most it held while alive, and the count after it is destroyed."""
    from tracerboy_amd import api
    before = live(gpu_tb)
    tb = api.TracerBoy(0) if devices is None else api.TracerBoy(devices=devices)
    try:
        exercise(tb)
        held = live(gpu_tb) - before
    finally:
        tb.close()
    return before, held, live(gpu_tb)


def _assert_given_back(gpu_tb, exercise, what, devices=None):
    before, held, after = _fresh_context_round_trip(gpu_tb, exercise, devices)
    assert held > 0, "%s: the counter saw no allocation (%d B)" % (what, held)
    assert after == before, "%s: %d B of device memory outlive the context (it held %d B)" % (what, after - before, held)


def test_counter_is_exact_and_shared_by_contexts(gpu_tb, settings):
    """The count is the same read through any live context, grows by the bytes a load uploads and falls back when the context goes."""
    from tracerboy_amd import api
    base = live(gpu_tb)
    with api.TracerBoy(0) as tb:
        assert live(tb) == base                                 # a context without a scene or a render holds no device memory
        tb.LoadScene(CORNELL)
        loaded = live(tb)
        assert loaded > base and live(gpu_tb) == loaded
        tb.Render(24, 16, 1, settings, 0.0)
        assert live(tb) >= loaded + 24 * 16 * 16 * 2            # at least the two accumulation surfaces
    assert live(gpu_tb) == base


def test_costly_first_frame_groups_give_back_everything(gpu_tb, settings):
    """(a) glass blobs fetched from memory, two frame-group calls: the second runs on the region order the first one's counts built
    (regionCost: 2^20 counts; regionOrder: one table per side stream) -- and all of it goes with the context."""
    s = copy.copy(settings); s.MaxBounces = 6

    def exercise(tb):
        tb.LoadProcedural(1, 20000, 5)
        tb.SetOption("frame_group", 2)
        for _ in range(2):
            tb.InvalidateHistory(); tb.Render(328, 200, 6, s, 0.0)
            assert tb.GetOption("last_plan_costly_first") == 1
        for _ in range(3):                                      # both side streams' order tables
            tb.InvalidateHistory(); tb.Render(328, 200, 6, s, 0.0, sync=False)
        tb.Sync()
        assert tb.GetOption("debug_region_cost_ptr") != 0
    _assert_given_back(gpu_tb, exercise, "costly regions first")


def test_aovs_post_process_and_realtime_give_back_everything(gpu_tb, settings):
    """(b) cornell with AOVs, the output stage and the real-time chain (TAA, denoiser and composite ping-pong surfaces)."""
    from tracerboy_amd import api
    s = copy.copy(settings); s.MaxBounces = 3

    def exercise(tb):
        tb.LoadScene(CORNELL)
        tb.SetOption("aov", 1)
        tb.Render(72, 40, 3, s, 0.0)
        tb.PostProcess(api.GetDefaultPostProcessSettings())
        tb.PostProcess(api.GetDefaultPostProcessSettings(), outputType=3)
        dn = api.GetDefaultDenoiserSettings(); dn.WaveletIterations = 2
        for _ in range(2):
            tb.RenderRealTime(72, 40, s, dn, 0.0)
        tb.PostProcess(api.GetDefaultPostProcessSettings())
    _assert_given_back(gpu_tb, exercise, "AOVs + post process + real-time chain")


@pytest.mark.parametrize("pipeline", ["split", "wavefront", "pooled"])
def test_other_pipelines_give_back_everything(gpu_tb, settings, pipeline):
    """(c) the split-role kernel (pipeline 4: profile buffer, mapped abort word), the wavefront pipeline (pipeline 2: SoA queues, hit and
    sample buffers) and the pooled kernel (pipeline 3), with the options their own tests use."""
    s = copy.copy(settings); s.MaxBounces = 5
    W, H = 120, 72

    def exercise(tb):
        if pipeline == "split":
            tb.LoadScene(CORNELL)
            tb.SetOption("pipeline", 4); tb.SetOption("split_profile", 1)
        elif pipeline == "wavefront":
            tb.LoadProcedural(1, 30000, 7)                      # glass: the SSS walk as queue entries of its own
            tb.SetOption("pipeline", 2); tb.SetOption("wavefront_paths", W * H * 2); tb.SetOption("wavefront_refill", 24)
        else:
            tb.LoadScene(CORNELL)
            tb.SetOption("pipeline", 3); tb.SetOption("pooled_samples", W * H * 3)
        tb.Render(W, H, 4, s, 0.0)
        assert tb.GetOption("last_pipeline") == {"split": 4, "wavefront": 2, "pooled": 3}[pipeline]
    _assert_given_back(gpu_tb, exercise, pipeline)


def test_tile_assignment_and_device_pack_give_back_everything(gpu_tb, settings):
    """(d) a rank's own tiles rendered and packed into a torch buffer on the device (the N > 1 step's path); the torch buffer is torch's."""
    import torch
    W, H = 200, 120

    def exercise(tb):
        tb.LoadScene(CORNELL)
        tb.SetTileAssignment(1, 3, 32, 16)
        tb.Render(W, H, 2, settings, 0.0)
        buf = torch.zeros((tb.OwnedPixels(W, H), 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        tb.PackOwnedTo(buf.data_ptr())
        assert float(buf[:, 3].max()) == 2.0
    _assert_given_back(gpu_tb, exercise, "tile assignment + PackOwnedTo")


def test_group_on_one_device_gives_back_everything(gpu_tb, settings):
    """(f) a group of two members on one device, 4 x 2 tiles of 64 x 64 so that both own tiles: the packed and gathered tiles, the events
    between the members (the second asynchronous call waits for the first one's un-permute) and the peer's whole context."""
    W, H = 200, 120

    def exercise(tb):
        assert tb._L.tb_group_size(tb._ctx) == 2
        tb.LoadScene(CORNELL)
        tb.Render(W, H, 2, settings, 0.0)
        tb.Render(W, H, 2, settings, 0.0, sync=False); tb.Render(W, H, 2, settings, 0.0, sync=False); tb.Sync()
        assert tb.GetNumberOfSamplesSinceLastInvalidate() == 6
    _assert_given_back(gpu_tb, exercise, "group of two on one device", devices=[0, 0])


def test_prepass_records_and_split_stack_give_back_everything(gpu_tb, settings):
    """(g) cornell fetched from memory in frame groups: sample buffers and slot logs, the pre-pass's hit records, the first-bounce pass's
    larger ones, then the split stack's overflow columns (forced as tests/test_primary_prepass.py forces them)."""
    s = copy.copy(settings); s.MaxBounces = 5
    W, H = 120, 72

    def render(tb):
        tb.InvalidateHistory(); tb.Render(W, H, 4, s, 0.0)

    def exercise(tb):
        tb.SetOption("scene_in_lds", 0); tb.SetOption("frame_group", 2)
        tb.LoadScene(CORNELL)
        tb.SetOption("primary_prepass", 1); render(tb)
        assert tb.GetOption("scene_in_lds_active") == 0 and tb.GetOption("last_primary_prepass") == 0     # the default policy: not for a call this small
        tb.SetOption("primary_prepass", 2); render(tb)
        assert tb.GetOption("last_primary_prepass") == 1 and tb.GetOption("last_first_bounce") == 0
        tb.SetOption("first_bounce", 1); render(tb)
        assert tb.GetOption("last_primary_prepass") == 1 and tb.GetOption("last_first_bounce") == 1
        tb.SetOption("stack_lds_cap", 4); tb.SetOption("stack_overflow_max", 64); render(tb)
        assert tb.GetOption("last_primary_prepass") == 1 and tb.GetOption("last_plan_stack_overflow") > 0
    _assert_given_back(gpu_tb, exercise, "pre-pass records + split stack")


def test_layout_c_gives_back_everything(gpu_tb, settings):
    """(h) the compact nodes, built at the first render that asks for them, lie among the scene's buffers."""
    def exercise(tb):
        tb.SetOption("scene_in_lds", 0); tb.SetOption("node_layout", 1)
        tb.LoadScene(CORNELL)
        tb.Render(64, 48, 4, settings, 0.0)                     # frame groups of a scene fetched from memory: the kernels that walk layout C
        assert tb.GetOption("last_node_layout") == 1
    _assert_given_back(gpu_tb, exercise, "layout C")


def test_batch_entry_points_hold_nothing_after_they_return(gpu_tb):
    """(i) TraceClosest and DeviceMath work in buffers of their own: gone when the call returns, while the context lives."""
    import numpy as np
    rng = np.random.default_rng(3)
    n = 1000

    def exercise(tb):
        tb.LoadScene(CORNELL)
        loaded = live(gpu_tb)
        d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
        info = tb.SceneInfo()
        centre = (np.float32(info.sceneMin[:]) + np.float32(info.sceneMax[:])) / 2
        hits = tb.TraceClosest(np.tile(centre, (n, 1)), d)
        assert (hits["t"] > 0).any() and live(gpu_tb) == loaded
        x = rng.uniform(0.5, 2.0, n).astype(np.float32)
        assert np.array_equal(tb.DeviceMath(11, x, x), np.ones(n, np.float32)) and live(gpu_tb) == loaded      # 11: a / b
    _assert_given_back(gpu_tb, exercise, "TraceClosest + DeviceMath")


def test_failed_load_gives_back_everything(gpu_tb, settings, tmp_path):
    """(e) a context whose LoadScene failed: first on a fresh context, then after a scene had been loaded and rendered."""
    from tracerboy_amd import api
    empty = tmp_path / "empty.pbrt"
    empty.write_text('LookAt 0 1 5  0 1 0  0 1 0\nCamera "perspective" "float fov" [45]\nWorldBegin\nWorldEnd\n')

    def fail_first(tb):
        with pytest.raises(api.TracerBoyError):
            tb.LoadScene(str(empty))
    before, held, after = _fresh_context_round_trip(gpu_tb, fail_first)
    assert after == before, "a context whose only load failed: %d B outlive it" % (after - before)

    def fail_later(tb):
        tb.LoadScene(TEAPOT)
        tb.Render(48, 32, 2, settings, 0.0)
        with pytest.raises(api.TracerBoyError):
            tb.LoadScene(str(empty))
        with pytest.raises(api.TracerBoyError):
            tb.LoadScene(os.path.join(str(tmp_path), "missing.pbrt"))
    _assert_given_back(gpu_tb, fail_later, "failed load after a render")


def test_reloads_do_not_accumulate(gpu_tb, settings):
    """Load A, render, load B, load A, render: the context holds what it held after the first render of A -- a load gives back the scene
    it replaces (the costly-first counts and tables stay, sized for the frame, and are reused)."""
    from tracerboy_amd import api
    s = copy.copy(settings); s.MaxBounces = 6
    base = live(gpu_tb)
    with api.TracerBoy(0) as tb:
        tb.SetOption("frame_group", 2)
        def render_a():
            tb.LoadProcedural(1, 20000, 5)
            for _ in range(2):
                tb.InvalidateHistory(); tb.Render(328, 200, 6, s, 0.0)
            assert tb.GetOption("last_plan_costly_first") == 1
            return live(tb)
        first = render_a()
        tb.LoadScene(CORNELL)
        tb.LoadScene(TEAPOT)
        second = render_a()
        assert second == first, "reload: %+d B against the first render of the same scene" % (second - first)
    assert live(gpu_tb) == base
