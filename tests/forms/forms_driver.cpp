/* forms_driver.cpp -- pt_pick_form (pt_copies.h) over every copy and every shape of a launch, in the launchers' place
 * (tests/test_launch_forms.py reads the lines):
 *   copy NAME SET FEATURES ROLE WAVES STASH COUNTING STREAMING PREPASS_IN_BASE NFORMS      one per row of the table; NFORMS: pt_forms_of
 *   pick NAME  mode groups list counting sceneLds twoLevel layoutC split overflowFits hits first shrinking  ->  OK
 *        stream sceneLds count groups hybrid nodeC twoLevel primary first guided adaptive pre              one per copy and shape */
#include "pt_copies.h"
#include <cstdio>

int main()
{
    for (int k = 0; k < kNumPtCopies; k++) {
        const PtCopy& c = kPtCopies[k];
        printf("copy %s %s %u %d %u %u %d %d %d %d\n", c.name, c.set, c.features, c.role, c.waves, c.stash, c.counting, c.streaming, c.prepassInBase,
            pt_forms_of(c).n);
        for (uint32_t i = 0; i < PT_SHAPES; i++) {
            const PtShape s = pt_shape_of(i);
            const PtPick p = pt_pick_form(c, s);
            const PtForm& f = p.form;
            printf("pick %s %d %d %d %d %d %d %d %d %d %d %d %d -> %d %d %d %d %d %d %d %d %d %d %d %d %d\n", c.name, s.mode, s.groups, s.list, s.counting,
                s.sceneLds, s.twoLevel, s.layoutC, s.split, s.overflowFits, s.hits, s.first, s.shrinking, p.ok, f.stream, f.sceneLds, f.count, f.groups,
                f.hybrid, f.nodeC, f.twoLevel, f.primary, f.first, f.guided, f.adaptive, f.pre);
        }
    }
    return 0;
}
