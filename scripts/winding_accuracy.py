"""The CPU measurements behind the constants of the winding numbers; needs no GPU.

    python scripts/winding_accuracy.py

1. The motivating count: on tetra4 and star40 (tests/winding_cases.py), the off-surface points of the seeds 70, 71, 72 at which
   HostScene.nearest(signed=True) -- the side of the nearest triangle -- disagrees with winding64 > 0.5, and at which the host walk at the default
   beta does.
2. The tolerance of the exact form (winding_cases.W_EXACT_TOL): the worst |w - winding64| of the host brute force and of the host walk at beta = inf
   under the builders 0, 1, 3, over every case but zero32, the same seeds, every off-surface point.
3. The tolerances of the dipole form (W_BETA_TOL): the same for the host walk at beta = 2, 3 and 4.
Each tolerance is the next power of two above 2 x the worst."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import adversarial_cases as ac  # noqa: E402
import mesh_cases as mc         # noqa: E402
import winding_cases as wc      # noqa: E402
from tracerboy_amd import api   # noqa: E402

BUILDERS = (0, 1, 3)


def tolerance(worst):
    return 2.0 ** (math.floor(math.log2(2.0 * worst)) + 1)


def main():
    exact = (0.0, None); dipole = {2.0: (0.0, None), 3.0: (0.0, None), 4.0: (0.0, None)}
    for name in wc.ACCURACY_NAMES:
        tri = wc.triangles(name)
        p, i = ac.soup(tri)
        scenes = {b: api.HostScene.from_meshes([api.Mesh(p, i)], mc.MATERIALS(), bvh_builder=b) for b in BUILDERS}
        wrong_nearest = wrong_walk = total = 0
        for seed in wc.SEEDS:
            pos, kinds, off, w64 = wc.truth(name, seed)
            pts = api.make_query_points(pos[off])
            want = w64[off]
            forms = [("brute", scenes[0].winding(pts))] + [("walk inf, builder %d" % b, scenes[b].winding(pts, beta=np.inf, walk=True)) for b in BUILDERS]
            for what, w in forms:
                e = float(np.abs(w.astype(np.float64) - want).max())
                if e > exact[0]:
                    exact = (e, (name, seed, what))
            for beta in dipole:
                for b in BUILDERS:
                    e = float(np.abs(scenes[b].winding(pts, beta=beta, walk=True).astype(np.float64) - want).max())
                    if e > dipole[beta][0]:
                        dipole[beta] = (e, (name, seed, "builder %d" % b))
            if name in ("tetra4", "star40"):
                inside = want > 0.5
                wrong_nearest += int(((scenes[0].nearest(pts, signed=True)["Distance"] < 0) != inside).sum())
                wrong_walk += int((api.winding_inside(scenes[0].winding(pts, walk=True)) != inside).sum())
                total += len(want)
        if total:
            print("%-10s the nearest triangle's side is wrong at %d of %d off-surface points; the winding walk at %d" % (name, wrong_nearest, total, wrong_walk))
        print("%-10s exact so far %.3e; beta 2: %.3e; beta 3: %.3e; beta 4: %.3e" % (name, exact[0], dipole[2.0][0], dipole[3.0][0], dipole[4.0][0]), flush=True)
    print("exact form: worst %.6e at %s -> W_EXACT_TOL = 2^%d" % (exact[0], exact[1], round(math.log2(tolerance(exact[0])))))
    for beta, (e, where) in dipole.items():
        print("beta %g: worst %.6e at %s -> W_BETA_TOL = 2^%d" % (beta, e, where, round(math.log2(tolerance(e)))))


if __name__ == "__main__":
    main()
