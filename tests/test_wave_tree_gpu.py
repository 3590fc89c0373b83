"""Builder 1's wave stage (option wave_tree; csrc/host/bvh_build.cpp optimizeForWaves, docs/experiments/r11.md) on the GPU: cornell-box through the
six-wave copy on the tree the stage leaves, bit for bit the oracle's on the same tree; the same picture with the stage off and on (a ray's closest hit
does not depend on the tree; at these sizes the oracle's own two pictures are the same bits, checked on the CPU before the sizes were committed);
and a counting launch whose box counts differ between the two trees and equal the oracle's on each."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import CORNELL

SIZES = [(40, 24, 4), (64, 48, 8)]
_SEEN = {}


def _settings():
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 8
    return s


def _both_trees(tb, W, H, F):
    """GPU surfaces, oracle surfaces and box counts of both trees at one size, computed once"""
    key = (W, H, F)
    if key in _SEEN:
        return _SEEN[key]
    s = _settings(); res = {}
    try:
        tb.SetOption("bvh_builder", 1)
        for wave_tree in (0, 1):
            tb.SetOption("wave_tree", wave_tree)
            tb.LoadScene(CORNELL)
            assert tb.GetOption("scene_in_lds_active") == 1
            tb.InvalidateHistory(); tb.Render(W, H, F, s, 0.0); tb.Sync()
            assert tb.GetOption("last_copy_waves") == 6 and tb.GetOption("last_pipeline") == 0
            out, jit = tb.ReadAccumulation(jittered=True)
            tb.SetOption("count_rays", 1); tb.InvalidateHistory(); tb.Render(W, H, 1, s, 0.0)
            boxes = int(tb.ReadbackStats().rays.boxesTested); tb.SetOption("count_rays", 0)
            pf = tb.FrameConstants(W, H, 0, s, 0.0)
            ref = ol.render(tb.HostSceneView(), pf, W, H, F, threads=8, jittered=True)
            one = ol.render(tb.HostSceneView(), pf, W, H, 1, threads=8, stats=True)
            res[wave_tree] = dict(out=out, jit=jit, boxes=boxes, ref=ref, ref_boxes=int(one["stats"].boxesTested), depth=tb.SceneInfo().bvhMaxDepth)
    finally:
        tb.SetOption("count_rays", 0); tb.SetOption("wave_tree", -1); tb.SetOption("bvh_builder", 0)
    _SEEN[key] = res
    return res


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,F", SIZES)
def test_the_wave_tree_renders_the_oracles_bits_through_the_six_wave_copy(gpu_tb, W, H, F):
    r = _both_trees(gpu_tb, W, H, F)[1]
    assert np.array_equal(_bits(r["out"]), _bits(r["ref"]["output"])) and np.array_equal(_bits(r["jit"]), _bits(r["ref"]["jittered"]))


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,F", SIZES)
def test_the_picture_is_the_same_with_the_stage_off_and_on(gpu_tb, W, H, F):
    r = _both_trees(gpu_tb, W, H, F)
    assert np.array_equal(_bits(r[0]["ref"]["output"]), _bits(r[1]["ref"]["output"]))      # the reference alone is tie-free at this size
    assert np.array_equal(_bits(r[0]["out"]), _bits(r[1]["out"])) and np.array_equal(_bits(r[0]["jit"]), _bits(r[1]["jit"]))


@pytest.mark.gpu
def test_a_counting_launch_sees_the_other_tree(gpu_tb):
    r = _both_trees(gpu_tb, *SIZES[0])
    print("box tests of one frame, stage off / on:", r[0]["boxes"], r[1]["boxes"], "depth", r[0]["depth"], r[1]["depth"])
    assert r[0]["boxes"] != r[1]["boxes"]
    assert r[0]["boxes"] == r[0]["ref_boxes"] and r[1]["boxes"] == r[1]["ref_boxes"]
