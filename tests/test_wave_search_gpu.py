"""The tree of builder 1's wave stage as it searches now -- every legal place priced, docs/experiments/r13.md -- on the GPU: cornell-box through the
six-wave copy at two small sizes with park_min 1, 2 and 64, `output` and `jittered` bit for bit the oracle's over the same host scene (the oracle
is rendered once per size: park_min changes the schedule, never a sample), and one counting launch whose box and triangle counts are the oracle's
on that tree."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import CORNELL

SIZES = [(40, 24, 4), (64, 48, 8)]
PARK_MINS = [1, 2, 64]
_REF = {}
_LOADED = {}


@pytest.fixture(scope="module")
def tb(built):
    """a context of this module's own: park_min is read when a scene is loaded"""
    from tracerboy_amd import api
    ctx = api.TracerBoy(0)
    ctx.SetOption("bvh_builder", 1); ctx.SetOption("wave_tree", 1)
    yield ctx
    ctx.close()
    _LOADED.clear(); _REF.clear()


def _settings():
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 8
    return s


def _load(tb, park_min):
    if _LOADED.get("now") != park_min:
        tb.SetOption("park_min", park_min)
        tb.LoadScene(CORNELL)
        _LOADED["now"] = park_min
    assert tb.GetOption("scene_in_lds_active") == 1


def _oracle(tb, W, H, F):
    """the oracle's surfaces over the context's own host scene, once per size"""
    if (W, H, F) not in _REF:
        _REF[(W, H, F)] = ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, _settings(), 0.0), W, H, F, threads=8, jittered=True)
    return _REF[(W, H, F)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,F", SIZES)
@pytest.mark.parametrize("park_min", PARK_MINS)
def test_the_searched_tree_renders_the_oracles_bits_at_every_park_min(tb, park_min, W, H, F):
    _load(tb, park_min)
    tb.InvalidateHistory(); tb.Render(W, H, F, _settings(), 0.0); tb.Sync()
    assert tb.GetOption("last_copy_waves") == 6 and tb.GetOption("last_pipeline") == 0
    out, jit = tb.ReadAccumulation(jittered=True)
    ref = _oracle(tb, W, H, F)
    assert np.array_equal(out.view(np.uint32), ref["output"].view(np.uint32))
    assert np.array_equal(jit.view(np.uint32), ref["jittered"].view(np.uint32))


@pytest.mark.gpu
def test_a_counting_launch_counts_what_the_oracle_counts_on_the_searched_tree(tb):
    W, H, _ = SIZES[0]; s = _settings()
    _load(tb, 2)
    try:
        tb.SetOption("count_rays", 1); tb.InvalidateHistory(); tb.Render(W, H, 1, s, 0.0)
        got = tb.ReadbackStats().rays
    finally:
        tb.SetOption("count_rays", 0)
    one = ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, s, 0.0), W, H, 1, threads=8, stats=True)["stats"]
    print("one %dx%d frame on the searched tree: %d box tests, %d triangle tests" % (W, H, int(got.boxesTested), int(got.trianglesTested)))
    assert int(got.boxesTested) == int(one.boxesTested) and int(got.trianglesTested) == int(one.trianglesTested)
    assert int(got.boxesTested) > 0 and int(got.trianglesTested) > 0
