/* launch_trials.h -- the two things about a render call no rule of launch_plan.h could decide and the context therefore TRIES: the
 * primary-visibility pre-pass and overlapping consecutive launches on the two side streams.  Both are state machines over times the caller
 * measured: nothing here includes a HIP header or asks the device anything (renderImpl, context_render.cpp, queries the events and hands
 * the results in), so tests/trials/ drives them on the CPU with made-up times (tests/test_launch_trials.py). */
#pragma once
#include <stdint.h>
#include <algorithm>

namespace tbhost {

/* The scenes the pre-pass policy cannot tell apart: of the first calls of one kind (same scene, frame, frames per call, depth: `key`) the
 * first runs without (it also pays for buffers and scratch, untimed), then with / without alternately until each side has two timed samples
 * -- the first launch of a call, with the events the context records anyway -- and the faster way is kept from then on. */
struct PrepassTrial { uint64_t key = 0; int calls = 0, pending = 0 /* 1 with, 2 without */, nWith = 0, nWithout = 0; float msWith = 0, msWithout = 0;
    bool keep = false; uint64_t stamp = 0; };

/* is the time of the first launch of the call before this one a sample of the trial?  (`stamp` counts the renders that have recorded the
 * two events: only if no other render has recorded them since) */
inline bool PrepassSampleWanted(const PrepassTrial& t, uint64_t key, uint64_t stamp) { return t.key == key && t.pending && t.stamp == stamp; }

/* One call of kind `key`: run it with the pre-pass?  sampleMs: the time PrepassSampleWanted asked for; <= 0 when it is not known -- the
 * caller renders asynchronously and the launch has not finished (nobody waits for it) -- and that step of the trial is repeated. */
inline bool PrepassTrialStep(PrepassTrial& t, uint64_t key, uint64_t stamp, float sampleMs)
{
    if (t.key != key) { t = PrepassTrial(); t.key = key; }
    if (t.pending) {
        if (t.stamp == stamp && sampleMs > 0) { float& best = t.pending == 1 ? t.msWith : t.msWithout; best = best > 0 ? std::min(best, sampleMs) : sampleMs;
            (t.pending == 1 ? t.nWith : t.nWithout)++; }
        else t.calls = t.pending == 1 ? 1 : 2; /* repeat the step whose sample was lost */
        if (t.nWith >= 2 && t.nWithout >= 2) t.keep = t.msWith < 0.99f * t.msWithout; /* the faster of two samples per side */
        t.pending = 0;
    }
    if (t.calls == 0) { t.calls = 1; return false; }
    if (t.nWith >= 2 && t.nWithout >= 2) return t.keep;
    const bool with = t.calls == 1;
    t.pending = with ? 1 : 2; t.stamp = stamp + 1; t.calls = with ? 2 : 1;
    return with;
}

/* Do back-to-back calls gain from running on the two side streams at once?  The end of every render is marked by an event of a ring of
 * eight (tb_context::evCallEnd); the interval between two ends, when the later call was enqueued before the earlier one had finished (the
 * device was never idle between them), is what a call costs in that mode.  Calls of one kind run overlapped until two device-bound spans are
 * known (phase 0), then one at a time until two more are (phase 1), then the faster way (phase 2).  A caller that waits for every call never
 * produces a device-bound interval and stays overlapped (for it the two ways are the same). */
struct OverlapTrial { uint64_t key = 0; int phase = 0; int n[2] = {0, 0}; float best[2] = {0, 0} /* [0] overlapped, [1] one at a time */; bool keep = true; };
/* call i of the context, at [i & 7]: its kind, its mode (0 overlapped, 1 one at a time, -1 not part of a trial), was the device still busy
 * with the call before it when it was enqueued, is that call of the same kind and mode (a settled pipeline); used: no span is to be read of it */
struct CallRec { uint64_t key = 0; int mode = -1; bool deviceBound = false, settled = false, used = true; };

/* Before call number `callCount`, of kind `key`: overlap it?  ended(i): has call i finished (its end event and that of call i - 2 exist);
 * spanMs(i): milliseconds between the ends of calls i - 2 and i, <= 0 when unknown.  A span is TWO calls long, halved: overlapped launches
 * finish in pairs (two are in flight at once: the ends of consecutive calls are alternately 2 ms and 86 ms apart on the van-class 4K
 * scene).  It counts when calls i - 1 and i were device-bound and settled and call i is not the last of a burst (the call after it was
 * enqueued while it ran): the last launch has the chip to itself.  Every record is looked at once. */
template <class Ended, class SpanMs>
inline bool OverlapTrialStep(OverlapTrial& t, CallRec (&ring)[8], uint64_t callCount, uint64_t key, Ended ended, SpanMs spanMs)
{
    if (t.key != key) { t = OverlapTrial(); t.key = key; }
    for (uint64_t i = callCount >= 5 ? callCount - 5 : 2; i + 1 < callCount; i++) {
        CallRec& r = ring[i & 7u]; const CallRec& q = ring[(i - 1) & 7u]; const CallRec& nx = ring[(i + 1) & 7u];
        if (r.used || r.key != key || !ended(i)) continue;
        r.used = true;
        float ms = 0;
        if (r.deviceBound && r.settled && q.deviceBound && q.settled && q.key == key && q.mode == r.mode && (r.mode == 0 || r.mode == 1) &&
            nx.deviceBound && nx.key == key && nx.mode == r.mode && (ms = spanMs(i)) > 0) {
            ms *= 0.5f; t.best[r.mode] = t.n[r.mode] ? std::min(t.best[r.mode], ms) : ms; t.n[r.mode]++;
        }
    }
    if (t.phase == 0 && t.n[0] >= 2) t.phase = 1;
    /* taking turns has to win by 2 %: short bursts flatter it (their last launch runs alone) */
    if (t.phase == 1 && t.n[1] >= 2) { t.phase = 2; t.keep = t.best[0] < 1.02f * t.best[1]; }
    return t.phase == 0 ? true : (t.phase == 1 ? false : t.keep);
}

/* the record of call number `callCount`: trial = it is part of the overlap trial, previousStillRunning = the call before it had not finished
 * when this one was enqueued */
inline void RecordCall(CallRec (&ring)[8], uint64_t callCount, uint64_t key, bool trial, bool overlap, bool previousStillRunning)
{
    CallRec& r = ring[callCount & 7u]; const CallRec& prev = ring[(callCount - 1) & 7u];
    r.key = key; r.mode = trial ? (overlap ? 0 : 1) : -1; r.used = !trial;
    r.deviceBound = callCount > 0 && previousStillRunning;
    r.settled = callCount > 0 && prev.key == key && prev.mode == r.mode;
}

} // namespace tbhost
