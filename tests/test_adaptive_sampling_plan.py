"""CPU: the launch plan of an adaptive call (tb_plan_input::adaptive, launch_plan.h) -- the base copy's one-pixel-per-lane
form whatever the options ask for, no frame groups, no pre-pass, no overlapping launches; two-level scenes in the full feature set.  With the
field off every plan is what it was before the field existed."""
import pytest

from tracerboy_amd import api

ENV, SPEC, TEX, SSS = 1, 2, 4, 8
W_MATTE, W_ENV, W_SSS = (api.VariantWavesHi(n) for n in ("matte", "env", "sss"))
MATTE = dict(variant_features=0, variant_waves_hi=W_MATTE, variant_has_wavefront=1, variant_has_pooled=1, variant_has_split=1)
ENVV = dict(variant_features=ENV, variant_waves_hi=W_ENV, variant_has_wavefront=1, variant_has_pooled=1, variant_has_split=1)
SSSV = dict(variant_features=ENV | SPEC | TEX | SSS, variant_waves_hi=W_SSS, variant_has_wavefront=1, variant_has_split=1)
HD = dict(width=1920, height=1080, owned_regions=120 * 68, max_bounces=8)
UHD = dict(width=3840, height=2160, owned_regions=240 * 135, max_bounces=6)
# the shapes of tests/test_launch_plan.py: C2 cornell-box (scene in LDS), C3 the 870 k scene, C4 the van-class 4K glass scene
SHAPES = {
    "c2": {**MATTE, **HD, **dict(frames=64, scene_in_lds=1, lds_blob_bytes=17 * 1024, stack_depth=11, has_lights=1)},
    "c3": {**ENVV, **HD, **dict(frames=128, stack_depth=26, max_bounces=6)},
    "c4": {**SSSV, **UHD, **dict(frames=256, stack_depth=36, has_lights=1, interior_walk_triangle_share=0.2)},
}
RULE_ADAPTIVE, COPY_NONE, COPY_FULL_FOR_INSTANCES, PRE_NO_KERNEL = 7, 10, 15, 20
FIELDS = [f for f, _ in api.abi.tb_launch_plan._fields_]


def plan(d, **kw):
    x = dict(d); x.update(kw)
    return api.PlanLaunch(**x)


def as_dict(p):
    return {f: getattr(p, f) for f in FIELDS}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("pipeline", [0, 1, 2, 3, 4])
def test_adaptive_plan_is_the_base_copy_one_pixel_per_lane(shape, pipeline):
    p = plan(SHAPES[shape], pipeline=pipeline, adaptive=1)
    assert (p.pipeline, p.groups, p.rule_pipeline) == (0, 0, RULE_ADAPTIVE)
    assert (p.prepass, p.rule_prepass, p.overlap_launches) == (0, PRE_NO_KERNEL, 0)
    assert (p.high_occupancy_copy, p.full_variant, p.rule_copy, p.stack_overflow_entries) == (0, 0, COPY_NONE, 0)
    assert p.stack_lds_entries == SHAPES[shape]["stack_depth"] and p.compact_nodes == 0
    assert (p.frame_group, p.batch_frames, p.guided_groups, p.costly_first) == (0, 0, 0, 0)
    # whatever else the options ask for
    q = plan(SHAPES[shape], pipeline=pipeline, adaptive=1, frame_group=8, primary_prepass=2, overlap_launches=2, node_layout=1, has_compact_nodes=1)
    assert as_dict(q) == as_dict(p)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_adaptive_two_level_scene_runs_the_full_feature_set(shape):
    p = plan(SHAPES[shape], two_level=1, adaptive=1)
    assert (p.pipeline, p.groups, p.rule_pipeline, p.full_variant, p.high_occupancy_copy, p.rule_copy) == (0, 0, RULE_ADAPTIVE, 1, 0,
                                                                                                          COPY_FULL_FOR_INSTANCES)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("pipeline", [0, 1, 2, 3, 4])
def test_adaptive_off_leaves_every_plan_as_it_was(shape, pipeline):
    for extra in ({}, dict(two_level=1), dict(frames=1), dict(aov=1)):
        kw = {**SHAPES[shape], "pipeline": pipeline, **extra}
        assert as_dict(plan(kw, adaptive=0)) == as_dict(api.PlanLaunch(**kw))
    assert as_dict(plan(SHAPES[shape], pipeline=pipeline)) != as_dict(plan(SHAPES[shape], pipeline=pipeline, adaptive=1))
