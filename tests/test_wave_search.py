"""The search of builder 1's wave stage (tracerboy_amd/csrc/host/bvh_build.cpp optimizeForWaves, docs/experiments/r13.md): every legal place of a cut
subtree is priced, not the three that rank first by induced area.  CPU only.

`places=3` is the stage as it was, byte for byte; the default's tree is the same bytes for every number of workers; it is priced no higher than the
three-place tree on the stage's own rays, on the validation rays and on two held-out seeds; the validation price does not rise; the tree stays valid
and inside the depth limit; one worker stays inside the load-time bound of tests/test_wave_cost.py; and on the hand-made 38-triangle room of
tests/wave_search/search_driver.cpp the full search reaches a price the three-place filter does not.  That program also runs the search under
ASan + UBSan and under TSan, with every shortcut's price checked against a plain walk of all rays."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from conftest import CORNELL

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "wave_search", "_build")

# sha256 of the layout-A image of cornell-box under builder 1 with the wave stage of the commit before this search (three places by area)
CORNELL_TREE_THREE_PLACES = "26105ccdc57f97ed2e028c3379d48ad03cfc9f8db6ba874d5d6a12f1d3c1f6ec"
STAGE_BOUND_MS = 4000.0       # tests/test_wave_cost.py's assertion, which must hold with one worker


def _sha(hs):
    return hashlib.sha256(hs.bvh_bytes().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def searched(built):
    """cornell-box: the default search with 1, 2 and 16 workers, and the three-place search; each (scene, stage report)"""
    from tracerboy_amd import api
    out = {}
    for key, kw in (("t1", dict(threads=1)), ("t2", dict(threads=2)), ("t16", dict(threads=16)), ("three", dict(places=3, threads=1))):
        hs = api.HostScene(CORNELL, bvh_builder=1, wave_tree=0)
        out[key] = (hs, hs.wave_search(**kw))
    out["default"] = (api.HostScene(CORNELL, bvh_builder=1, wave_tree=1), None)
    return out


def test_three_places_is_the_stage_as_it_was(searched):
    hs, st = searched["three"]
    assert _sha(hs) == CORNELL_TREE_THREE_PLACES
    assert (st.places, st.moves, st.evaluations, st.before.cost, st.after.cost) == (3, 4, 409, 53172.0, 49079.0)
    assert st.screen_waves == 0 and st.validation_rejects == 0


def test_the_tree_is_the_same_bytes_for_every_number_of_workers(searched):
    one = searched["t1"][0].bvh_bytes()
    for key in ("t2", "t16", "default"):
        assert np.array_equal(searched[key][0].bvh_bytes(), one), key
    assert searched["t1"][1].threads == 1 and searched["t2"][1].threads == 2 and searched["t16"][1].threads == 16
    assert 1 <= searched["default"][0].wave_stage().threads <= 16
    assert searched["t1"][1].after.cost == searched["t16"][1].after.cost == searched["default"][0].wave_stage().after.cost


def test_every_place_is_priced_no_higher_than_three_places_on_seen_and_unseen_rays(searched):
    (full, st), (three, st3) = searched["t1"], searched["three"]
    print("stage rays %.0f vs %.0f, validation %.0f vs %.0f" % (st.after.cost, st3.after.cost, st.validation_after, st3.validation_after))
    assert st.places == 0 and st.before.cost == st3.before.cost
    assert st.after.cost <= st3.after.cost and st.after.cost < st.before.cost
    assert full.wave_cost().cost == st.after.cost                        # the price is that of the image that was built
    assert st.validation_after <= st3.validation_after
    for seed in (0x1234, 0xbeef):
        a, b = full.wave_cost(seed=seed, waves=64).cost, three.wave_cost(seed=seed, waves=64).cost
        print("seed %#x at 64 waves: %.0f vs %.0f" % (seed, a, b))
        assert a <= b


def test_the_validation_price_does_not_rise(searched):
    st = searched["t1"][1]
    assert 0 < st.validation_after <= st.validation_before
    assert st.validation_before == searched["three"][1].validation_before      # the same rays over the same start tree


def test_depth_stays_within_the_limit_and_the_tree_is_valid(searched):
    hs, st = searched["t1"]
    rc, depth = ol.validate_bvh(hs.bvh_bytes(), hs.triangles())
    assert rc == 0 and depth == hs.info().bvhMaxDepth and depth <= st.depth_limit


def test_one_worker_stays_inside_the_load_time_bound(searched):
    st = searched["t1"][1]
    print("one worker: %.0f ms; %d passes, %d moves, %d places screened on %d waves, %d priced on all, %d abandoned, %d rays checked, %d walked again, "
          "%d winners refused, %d cuts skipped" % (st.milliseconds, st.passes, st.moves, st.places_screened, st.screen_waves, st.places_priced, st.abandoned,
                                                   st.rays_checked, st.rays_rewalked, st.validation_rejects, st.cuts_skipped))
    assert st.milliseconds < STAGE_BOUND_MS
    assert st.passes < 12                                                      # the search ended because a pass moved nothing, not at the cap


def test_the_room_has_a_move_the_three_place_filter_cannot_reach_under_sanitizers():
    """tests/wave_search/search_driver.cpp, once with ASan + UBSan and once with TSan (four workers), every price checked against a plain walk"""
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "wave_search"), "OUT=" + BUILD], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # the plain program at the stage's own size; the sanitizer builds, many times slower, on 9 waves (one more than the screen's 8), ASan + UBSan
    # with every price checked against a plain walk of all rays
    for exe, args in (("search_plain", ["4"]), ("search_asan", ["4", "verify", "9"]), ("search_tsan", ["4", "plain", "9"])):
        p = subprocess.run([os.path.join(BUILD, exe)] + args, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, (exe, (p.stdout[-2000:] + p.stderr)[-4000:])
        answers = dict((w[0], w[1:]) for w in (line.split() for line in p.stdout.splitlines()))
        print(exe, answers)
        assert answers["same_tree"] == ["1"] and answers["priced_right"] == ["1"]
        assert answers["threaded"][:3] == answers["serial"][:3] and answers["threaded"][-1] == "4"
        assert float(answers["serial"][8]) <= float(answers["serial"][7])      # the validation price did not rise
        if exe == "search_plain":
            # the full search ends below what the three-place search reaches: there are moves here that the filter never prices
            assert float(answers["serial"][1]) < float(answers["by_area"][1]) < float(answers["by_area"][0])
