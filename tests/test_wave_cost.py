"""What a 64-lane wave pays for a tree (tracerboy_amd/csrc/host/wave_cost.h) and builder 1's wave stage that optimises for it (bvh_build.cpp
optimizeForWaves, option wave_tree; docs/experiments/r11.md).  CPU only.

The single-ray walk visits what the oracle visits; the lock-step replay gives the trip counts worked out by hand below; the stage is deterministic,
leaves a valid tree inside both depth limits, never returns a tree it prices above the one it was given, stays within its load-time bound, and
touches nothing but the trees of LDS-resident scenes.  tests/wave/wave_driver.cpp runs the same code under ASan + UBSan as a host program."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from conftest import CORNELL

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "wave", "_build")

# sha256 of the layout-A image of cornell-box under builder 1 as the commit before the wave stage built it
CORNELL_TREE_BEFORE = "f6cb38cad9ec49e68ea7fa6be994b2967a290cf594b16c61c6b069bf41702ba7"
PROCEDURAL = (0, 300, 1)      # a few hundred triangles: over the LDS budget
STAGE_BOUND_MS = 1000.0       # the stated load-time bound for a 36-triangle scene on one core (0.6 s measured)


@pytest.fixture(scope="module")
def cornell(built):
    from tracerboy_amd import api
    return {wt: api.HostScene(CORNELL, bvh_builder=1, wave_tree=wt) for wt in (0, 1)}


@pytest.fixture(scope="module")
def procedural(built):
    from tracerboy_amd import api
    return {wt: api.HostScene(procedural=PROCEDURAL, bvh_builder=1, wave_tree=wt) for wt in (0, 1)}


@pytest.mark.parametrize("which", ["cornell_off", "cornell_on", "procedural"])
def test_the_walk_visits_what_the_oracle_visits(cornell, procedural, which):
    hs = {"cornell_off": cornell[0], "cornell_on": cornell[1], "procedural": procedural[1]}[which]
    o, d, t = hs.wave_rays(waves=48)     # 3 072 model rays: bounce rays and, where the scene has lights, feelers
    assert len(o) == 48 * 64 and np.all(t == np.float32(999999.0))
    inner, leaf, steps = hs.wave_walk(o, d, want_steps=True)
    ref = ol.trace_closest(hs.view(), o, d)
    assert np.array_equal(inner * 2, ref["boxes"]) and np.array_equal(leaf, ref["tris"])
    assert [s.count("I") for s in steps] == list(inner) and [s.count("L") for s in steps] == list(leaf)
    assert inner.sum() > len(o) and leaf.sum() > len(o) // 4          # the rays do walk the tree
    if which != "procedural":
        assert 0 < (inner + leaf == 0).sum() < len(o) // 2             # some leave on the outer side of a wall and miss the root box


def _trips(steps, park_min):
    from tracerboy_amd import api
    w = api.wave_replay(steps, park_min)
    return (w.inner_trips, w.leaf_trips, w.idle_passes, w.inner_active, w.leaf_active)


def test_replay_of_hand_written_walks():
    """The schedule: inner = lanes at an inner node; do { if (inner) do { they step } while (popc(inner) >= park_min); busy = inner | lanes at a leaf;
    those take the leaf step } while (busy).  A pass whose leaf step nobody takes counts as idle."""
    # one lane, park_min 2: a lone lane leaves the inner loop after every step -- trip, idle pass, trip, leaf pass, the idle pass that ends the walk
    assert _trips(["IIL"], 2) == (2, 1, 2, 2, 1)
    # ... and park_min 1 keeps it in the loop: two trips, the leaf pass, the last pass
    assert _trips(["IIL"], 1) == (2, 1, 1, 2, 1)
    # two lanes of different length: trip (both), leaf pass (B), trip (A), leaf pass (A), last pass
    assert _trips(["IIL", "IL"], 2) == (2, 2, 1, 3, 2)
    # the threshold matters: at 2 the two long lanes go on together and all three share ONE leaf pass ...
    assert _trips(["IIIL", "IIIL", "IL"], 2) == (3, 1, 1, 7, 3)
    # ... at 3 the loop is left when the short lane reaches its leaf: leaf pass (C), trip, idle pass, trip, leaf pass (A, B), last pass
    assert _trips(["IIIL", "IIIL", "IL"], 3) == (3, 2, 2, 7, 3)
    # a walk that is only the idle pass: no lane has a step
    assert _trips(["", ""], 2) == (0, 0, 1, 0, 0)
    assert _trips([], 2) == (0, 0, 1, 0, 0)
    # leaf steps only (a root that is a leaf); and a string of anything else is refused
    assert _trips(["L"] * 64, 2) == (0, 1, 1, 0, 64)
    from tracerboy_amd import api
    with pytest.raises(api.TracerBoyError):
        api.wave_replay(["IXL"], 2)


def test_cost_is_trips_times_the_listed_instruction_counts(cornell):
    from tracerboy_amd import api
    st = cornell[1].wave_stage()
    assert (st.inner_insts, st.leaf_insts) == (63, 88)
    w = api.wave_replay(["IIIL", "IIIL", "IL"], 3)
    assert w.cost == 3 * 63 + 2 * 88


def test_the_stage_is_deterministic_and_off_means_the_tree_of_before(cornell):
    from tracerboy_amd import api
    again = api.HostScene(CORNELL, bvh_builder=1, wave_tree=1)
    assert np.array_equal(again.bvh_bytes(), cornell[1].bvh_bytes())
    assert hashlib.sha256(cornell[0].bvh_bytes().tobytes()).hexdigest() == CORNELL_TREE_BEFORE
    assert not np.array_equal(cornell[0].bvh_bytes(), cornell[1].bvh_bytes())
    assert cornell[0].wave_stage().ran == 0 and cornell[1].wave_stage().ran == 1
    # the other builders have no such stage
    assert np.array_equal(api.HostScene(CORNELL, bvh_builder=0, wave_tree=1).bvh_bytes(), api.HostScene(CORNELL, bvh_builder=0).bvh_bytes())


def _shading_bytes(hs):
    v = hs.view()
    r16 = lambda b: (b + 15) // 16 * 16   # noqa: E731
    return r16(v.numHitGroups * 16) + r16(v.numIndices * 4) + r16(v.numVertexFloats * 4) + r16(v.numMaterials * 96) + r16(v.numLights * 112)


def _six_wave_copy_fits(stack_depth, image_bytes):
    share = (160 * 1024 // 6) // 512 * 512
    return (stack_depth * 1024 + image_bytes + 128 + 511) // 512 * 512 <= share


def test_the_tree_stays_valid_and_inside_both_depth_limits(cornell):
    on, off = cornell[1], cornell[0]
    rc, depth = ol.validate_bvh(on.bvh_bytes(), on.triangles())
    assert rc == 0 and depth == on.info().bvhMaxDepth
    st = on.wave_stage()
    assert depth <= st.depth_limit <= 31                       # the step the area passes keep (31 levels: five workgroups per CU)
    _, info = on.lds_image()
    _, before = off.lds_image()
    assert info.bytes == before.bytes and info.stack_depth == max(depth, 2)
    assert _six_wave_copy_fits(before.stack_depth, before.bytes) and _six_wave_copy_fits(info.stack_depth, info.bytes)
    assert info.bytes + _shading_bytes(on) + info.stack_depth * 1024 <= 40 * 1024          # LDS-resident under the default budget
    # the limit itself is the deepest tree for which all of that still holds
    assert _six_wave_copy_fits(st.depth_limit, info.bytes) and info.bytes + _shading_bytes(on) + st.depth_limit * 1024 <= 40 * 1024
    assert not (_six_wave_copy_fits(st.depth_limit + 1, info.bytes) and info.bytes + _shading_bytes(on) + (st.depth_limit + 1) * 1024 <= 40 * 1024
                and st.depth_limit + 1 <= 31)


def test_the_stage_never_prices_its_result_above_its_start_and_keeps_its_time_bound(cornell):
    st = cornell[1].wave_stage()
    print("wave stage: %d rays, %d moves, %d trees priced, %.0f ms, cost %.0f -> %.0f" % (st.rays, st.moves, st.evaluations, st.milliseconds,
                                                                                          st.before.cost, st.after.cost))
    assert st.after.cost <= st.before.cost and st.moves > 0 and st.after.cost < st.before.cost
    # the prices are those of the images that were built: the same rays over the tree read back from each scene
    assert cornell[0].wave_cost().cost == st.before.cost and cornell[1].wave_cost().cost == st.after.cost
    assert (cornell[1].wave_cost().inner_trips, cornell[1].wave_cost().leaf_trips) == (st.after.inner_trips, st.after.leaf_trips)
    # rays the search never saw agree on the direction
    for seed in (0x1234, 0xbeef):
        assert cornell[1].wave_cost(seed=seed, waves=64).cost < cornell[0].wave_cost(seed=seed, waves=64).cost
    assert st.rays == 24 * 64 and st.park_min == 2
    assert st.milliseconds < 4 * STAGE_BOUND_MS      # loose: a loaded machine must not fail it


def test_a_scene_over_the_lds_budget_is_left_alone(procedural):
    assert np.array_equal(procedural[0].bvh_bytes(), procedural[1].bvh_bytes())
    assert procedural[1].wave_stage().ran == 0
    _, info = procedural[1].lds_image()
    assert info.bytes + info.stack_depth * 1024 > 40 * 1024


def test_wave_cost_and_the_stage_under_sanitizers():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "wave"), "OUT=" + BUILD], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    p = subprocess.run([os.path.join(BUILD, "wave_driver")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:] + p.stderr)[-4000:]
    answers = dict((w[0], w[1:]) for w in (line.split() for line in p.stdout.splitlines()))
    print(answers)
    assert answers["replay_one_lane"] == ["2", "1", "2"] and answers["replay_threshold"] == ["3", "2", "2"] and answers["replay_idle"] == ["0", "0", "1"]
    assert answers["stage"][0] == "ran" and float(answers["stage"][2]) <= float(answers["stage"][1])
    assert answers["walk_matches_brute_force"] == ["1"]
