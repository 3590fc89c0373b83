"""The two trials of a render call (tracerboy_amd/csrc/host/launch_trials.h) on the CPU, with made-up times.

What a call launches where no rule decides -- the primary-visibility pre-pass, overlapping consecutive calls on the two side streams -- is
tried and measured by two state machines that renderImpl feeds with what it read from its events.  tests/trials/trials_driver.cpp stands in
for renderImpl; the sequences below are the ones the header promises."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "trials", "_build")


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "trials"), "OUT=" + BUILD], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    exe = os.path.join(BUILD, "trials_driver")

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
        return [l.split()[1:] for l in p.stdout.splitlines()]
    return run


def _prepass(driver, steps, key=7):
    """steps: the time of the first launch of the call before, per call (0 = not known); every call is the context's next render.
    -> [with?], (nWith, nWithout) after the last call"""
    out = driver(["prepass %d %d %g" % (key, stamp, ms) for stamp, ms in enumerate(steps)])
    return [int(o[0]) for o in out], (int(out[-1][1]), int(out[-1][2]))


def test_prepass_trial_decides_for(driver):
    # first call without and untimed; then with / without alternately until two samples a side: with 8 and 7 ms, without 10 and 9 ms
    withs, n = _prepass(driver, [0, 0, 8, 10, 7, 9, 0, 0])
    assert withs == [0, 1, 0, 1, 0, 1, 1, 1] and n == (2, 2)


def test_prepass_trial_decides_against_below_one_percent(driver):
    # the faster of two samples a side: 9.95 ms with against 10 ms without is no gain of 1 % (0.99 x 10 = 9.9) ...
    withs, _ = _prepass(driver, [0, 0, 12, 11, 9.95, 10, 0, 0])
    assert withs == [0, 1, 0, 1, 0, 0, 0, 0]
    # ... 9.8 ms is
    withs, _ = _prepass(driver, [0, 0, 12, 11, 9.8, 10, 0, 0])
    assert withs[5:] == [1, 1, 1]


def test_prepass_trial_repeats_a_step_whose_sample_was_lost(driver):
    # call 2 does not know yet how long call 1 (with) took: with again; call 4 does not know call 3 (without): without again
    withs, n = _prepass(driver, [0, 0, 0, 8, 0, 10, 7, 9, 0])
    assert withs == [0, 1, 1, 0, 0, 1, 0, 1, 1] and n == (2, 2)          # decided at call 7: 7 ms with against 9 ms without


def test_prepass_trial_ignores_a_sample_another_render_recorded(driver):
    # between call 1 (with, stamp 1 -> its events are render 2's) and the next call of the kind, another render used the events: stamp 3, not 2
    out = driver(["prepass 7 0 0", "prepass 7 1 0", "prepass 7 3 8"])
    assert [o[0] for o in out] == ["0", "1", "1"] and out[-1][1:] == ["0", "0"]


def test_prepass_trial_starts_over_for_a_new_key(driver):
    lines = ["prepass 7 %d %g" % (i, ms) for i, ms in enumerate([0, 0, 8, 10, 7, 9, 0])] + ["prepass 9 7 5", "prepass 9 8 0", "prepass 9 9 4"]
    out = driver(lines)
    assert out[6] == ["1", "2", "2"]                       # decided for key 7
    assert out[7] == ["0", "0", "0"]                       # key 9: first call without, untimed, nothing carried over (the 5 ms are key 7's)
    assert out[8] == ["1", "0", "0"] and out[9] == ["0", "1", "0"]


def _burst(first, count, key, step, t0, lag=2):
    """`count` calls enqueued back to back from call number `first`, ending `step` ms apart from t0; when a call is enqueued the calls up to
    `lag` before it have ended.  The first call of a burst finds the device idle."""
    lines = []
    for k in range(count):
        i = first + k
        lines.append("end %d %g" % (i, t0 + step * (k + 1)))
        lines.append("call %d %d %d" % (key, 1 if k else 0, i - lag))
    return lines


def _overlap(driver, lines):
    return [(int(o[0]), int(o[1]), int(o[2]), int(o[3]), float(o[4]), float(o[5])) for o in driver(lines)]


def _steady(per_call_overlapped, per_call_in_turn, calls=14):
    """one long burst: overlapped calls end `per_call_overlapped` ms apart, calls taking turns `per_call_in_turn` ms apart"""
    lines, t = [], 0.0
    # the trial leaves phase 0 before call 5 (spans of calls 2 and 3 known); calls 0-4 run overlapped, the rest one at a time until it decides
    for i in range(calls):
        t += per_call_overlapped if i < 5 else per_call_in_turn
        lines += ["end %d %g" % (i, t), "call 3 %d %d" % (1 if i else 0, i - 2)]
    return lines


def test_overlap_trial_keeps_overlapping(driver):
    out = _overlap(driver, _steady(10, 12))
    assert [o[0] for o in out[:5]] == [1] * 5 and [o[1] for o in out[:5]] == [0] * 5          # phase 0: overlapped
    assert out[5][:3] == (0, 1, 2)                                                             # two spans known: one at a time
    # call 5 is not settled (the call before it ran overlapped): the spans of calls 7 and 8 count, known before calls 9 and 10
    assert [o[1] for o in out[5:10]] == [1] * 5 and [o[0] for o in out[5:10]] == [0] * 5
    assert out[10][:4] == (1, 2, 2, 2) and out[10][4:] == (10.0, 12.0)                         # half of two calls' interval each
    assert all(o[:2] == (1, 2) for o in out[10:])


def test_overlap_trial_taking_turns_has_to_win_by_two_percent(driver):
    assert _overlap(driver, _steady(10, 9.9))[-1][:2] == (1, 2)       # 10 < 1.02 x 9.9: stays overlapped
    assert _overlap(driver, _steady(10, 9.7))[-1][:2] == (0, 2)       # 10 > 1.02 x 9.7: one at a time


def test_overlap_trial_does_not_count_the_last_call_of_a_burst(driver):
    # two bursts of four with the device idle in between: call 3 is the last of its burst (call 4 found the device idle) -- of calls 2 and 3
    # only call 2's span counts; call 4 is not device-bound, so neither calls 4 nor 5 (whose predecessor it is) give one
    out = _overlap(driver, _burst(0, 4, 3, 10, 0) + _burst(4, 4, 3, 10, 1000) + _burst(8, 1, 3, 10, 2000, lag=1))
    assert [o[2] for o in out] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert out[-1][:2] == (0, 1)                                      # call 6's span was the second: phase 1 from call 8 on


def test_overlap_trial_of_a_caller_that_waits_stays_in_phase_0(driver):
    lines = []
    for i in range(24):
        lines += ["end %d %g" % (i, 10.0 * (i + 1)), "call 3 0 %d" % (i - 1)]              # every call finds the device idle
    out = _overlap(driver, lines)
    assert all(o[:4] == (1, 0, 0, 0) for o in out)


def test_overlap_trial_starts_over_for_a_new_key_and_skips_other_kinds(driver):
    lines = _steady(10, 12, calls=8)
    lines += ["plain 5 1"]                                             # a call outside the trial: its record is nobody's span
    t = 1000.0
    for i in range(9, 15):
        t += 10
        lines += ["end %d %g" % (i, t), "call 4 1 %d" % (i - 2)]
    out = _overlap(driver, lines)
    assert out[7][:2] == (0, 1)                                        # kind 3 was in phase 1
    assert out[8][:4] == (1, 0, 0, 0)                                  # kind 4 starts in phase 0 with nothing known
    # call 9 follows a call of another kind (not settled): calls 11 and 12 are the first whose spans count, known before calls 13 and 14
    assert [o[2] for o in out[8:]] == [0, 0, 0, 0, 1, 2]
