/* trials_driver.cpp -- launch_trials.h driven from standard input, in renderImpl's place (tests/test_launch_trials.py writes the lines):
 *   prepass KEY STAMP MS     one call of kind KEY when the context has recorded STAMP renders; MS: the first launch of the call before it
 *                            took that long, 0 = it has not finished.  -> "prepass WITH nWith nWithout"
 *   end I MS                 call I of the context ended at time MS
 *   call KEY BUSY DONE       the next call, of kind KEY; BUSY: the call before it had not finished; DONE: calls up to that number have
 *                            -> "call OVERLAP phase n[0] n[1] best[0] best[1]"
 *   plain KEY BUSY           the next call, of a kind that is not tried (its record only) */
#include "launch_trials.h"
#include <cstdio>
#include <cstring>
#include <map>
using namespace tbhost;

int main()
{
    PrepassTrial pre; OverlapTrial over; CallRec ring[8]; uint64_t callCount = 0;
    std::map<uint64_t, float> ends;
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "prepass")) {
            unsigned long long key, stamp; float ms;
            if (scanf("%llu %llu %f", &key, &stamp, &ms) != 3) return 2;
            if (!PrepassSampleWanted(pre, key, stamp)) ms = 0;
            const bool with = PrepassTrialStep(pre, key, stamp, ms);
            printf("prepass %d %d %d\n", with ? 1 : 0, pre.nWith, pre.nWithout);
        } else if (!strcmp(cmd, "end")) {
            unsigned long long i; float ms;
            if (scanf("%llu %f", &i, &ms) != 2) return 2;
            ends[i] = ms;
        } else if (!strcmp(cmd, "call") || !strcmp(cmd, "plain")) {
            const bool trial = cmd[0] == 'c';
            unsigned long long key; int busy; long long done = -1;
            if (scanf("%llu %d", &key, &busy) != 2 || (trial && scanf("%lld", &done) != 1)) return 2;
            bool overlap = true;
            if (trial) overlap = OverlapTrialStep(over, ring, callCount, key,
                [&](uint64_t i) { return (long long)i <= done && ends.count(i) && ends.count(i - 2); },
                [&](uint64_t i) { return ends[i] - ends[i - 2]; });
            RecordCall(ring, callCount, key, trial, overlap, busy != 0);
            callCount++;
            if (trial) printf("call %d %d %d %d %.4f %.4f\n", overlap ? 1 : 0, over.phase, over.n[0], over.n[1], over.best[0], over.best[1]);
        } else return 2;
    }
    return 0;
}
