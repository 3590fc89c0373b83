"""The two CPU measurements behind the constants of the point queries; needs no GPU.

    python scripts/nearest_slack.py

1. The pruning slack (include/tb_nearest.h TB_NEAREST_SLACK_ULPS).  tb_host_scene_nearest_excess over every case of tests/adversarial_cases.py x the
   host builders 0, 1, 3 and the point seeds 70, 71, 72 of tests/nearest_cases.py: the largest sqrt(tb_box_d2) - sqrt(D2) of a box above a
   brute-force winner, in units of 2^-23 x the largest coordinate magnitude of the root box and the point.  The constant is at least 4 x the worst.
2. The tolerance of the geometry test (tests/nearest_cases.py DISTANCE_C): the worst |Distance - d64| / (2^-23 M aspect(Prim)) of the host brute
   force against the float64 brute force, over every case but zero32 and the same seeds.  DISTANCE_C is the next power of two above 2 x the worst."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import adversarial_cases as ac  # noqa: E402
import mesh_cases as mc         # noqa: E402
import nearest_cases as nc      # noqa: E402
from tracerboy_amd import api   # noqa: E402

BUILDERS = (0, 1, 3)
SEEDS = (70, 71, 72)


def main():
    worst_excess, worst_ratio = (0.0, None), (0.0, None)
    for name in ac.NAMES:
        tri = ac.triangles(name)
        p, i = ac.soup(tri)
        scenes = {b: api.HostScene.from_meshes([api.Mesh(p, i)], mc.MATERIALS(), bvh_builder=b) for b in BUILDERS}
        asp = nc.aspect(tri)
        for seed in SEEDS:
            pos, maxd, kinds = nc.points(tri, seed=seed)
            pts = api.make_query_points(pos, maxd)
            for b in BUILDERS:
                e = scenes[b].nearest_excess(pts)
                if e > worst_excess[0]:
                    worst_excess = (e, (name, b, seed))
            if name == "zero32":
                continue
            got = scenes[0].nearest(pts)
            found = got["Prim"] != api.NEAREST_NONE
            d64 = nc.distance64(tri, pos[found])
            ratio = np.abs(got["Distance"][found].astype(np.float64) - d64) / (nc.ULP * nc.scale(tri, pos[found]) * asp[got["Prim"][found]])
            if ratio.max() > worst_ratio[0]:
                worst_ratio = (float(ratio.max()), (name, seed))
        print("%-10s excess so far %.3f ratio so far %.3f" % (name, worst_excess[0], worst_ratio[0]), flush=True)
    print("worst pruning excess: %.3f x 2^-23 x scale at %s" % worst_excess)
    print("worst distance ratio: %.3f at %s" % worst_ratio)


if __name__ == "__main__":
    main()
