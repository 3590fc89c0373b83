#!/usr/bin/env python3
"""Price builder 1's wave stage (option wave_tree, csrc/host/wave_cost.h) on the CPU: docs/experiments/r11.md.

For cornell-box with the stage off and on: the oracle's ray log (TB_ORACLE_RAY_LOG) of 64 x 64 x 32 at depth 8 on that tree, replayed with
scripts/simd_sim.py's Wave model -- the lock-step two-slot schedule at park_min 2 with a frame-group queue per 16 x 16 region -- and the stage's own
model rays over the same tree.  Prints one JSON object; the real log is the judge, the model only drives the search.

  python scripts/wave_tree_price.py [--size 64] [--frames 32] [--out profiles/r11/wave_tree_price.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import simd_sim  # noqa: E402

CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
CI, CL = 63.0, 88.0   # wave instructions per trip through the inner loop / the leaf step (scripts/isa_walk_steps.py on pt_variant_matte6)


def price(wave_tree, size, frames, depth, keep_log=None):
    import oracle_lib as ol
    from tracerboy_amd import api
    hs = api.HostScene(CORNELL, bvh_builder=1, wave_tree=wave_tree)
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = depth
    path = keep_log or tempfile.mktemp(suffix=".raylog")
    if os.path.exists(path): os.remove(path)
    os.environ["TB_ORACLE_RAY_LOG"] = path
    try:
        ol.render(hs.view(), hs.frame_constants(s, 0, 0.0), size, size, frames, threads=8)
    finally:
        del os.environ["TB_ORACLE_RAY_LOG"]
    samples = simd_sim.load(path)
    if not keep_log: os.remove(path)
    n = len(samples); rays = [r for v in samples.values() for r in v]
    w = simd_sim.lockstep_queue(samples, park_min=2, region=16)
    st = hs.wave_stage(); mc = hs.wave_cost()
    other = {"seed_%x" % sd: hs.wave_cost(seed=sd).cost for sd in (0x1234, 0xbeef)}   # rays the search never saw
    return {"wave_tree": wave_tree, "depth_nodes": int(hs.info().bvhMaxDepth), "samples": n, "rays_per_sample": len(rays) / n,
            "feeler_share": sum(1 for r in rays if r[0] == "S") / len(rays),
            "inner_steps_per_ray": sum(r[1].count("I") for r in rays) / len(rays), "leaf_steps_per_ray": sum(r[1].count("L") for r in rays) / len(rays),
            "log": {"inner_trips_per_64": w.inner_trips * 64.0 / n, "leaf_trips_per_64": w.leaf_trips * 64.0 / n,
                    "inner_occupancy": w.inner_active / max(w.inner_trips, 1) / 64.0, "leaf_occupancy": w.leaf_active / max(w.leaf_trips, 1) / 64.0,
                    "cost_per_sample": (w.inner_trips * CI + w.leaf_trips * CL) / n},
            "model": {"rays": int(st.rays), "inner_trips": int(mc.inner_trips), "leaf_trips": int(mc.leaf_trips), "idle_passes": int(mc.idle_passes),
                      "cost": mc.cost, "other_seeds_cost_per_wave": other},
            "stage": {"ran": int(st.ran), "moves": int(st.moves), "evaluations": int(st.evaluations), "milliseconds": st.milliseconds,
                      "cost_before": st.before.cost, "cost_after": st.after.cost, "depth_limit": int(st.depth_limit)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64); ap.add_argument("--frames", type=int, default=32); ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"scene": "cornell-box", "size": a.size, "frames": a.frames, "depth": a.depth, "insts": [CI, CL],
           "trees": [price(0, a.size, a.frames, a.depth), price(1, a.size, a.frames, a.depth)]}
    off, on = res["trees"]
    res["log_cost_change"] = on["log"]["cost_per_sample"] / off["log"]["cost_per_sample"] - 1.0
    res["model_cost_change"] = on["model"]["cost"] / off["model"]["cost"] - 1.0
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f: f.write(text + "\n")


if __name__ == "__main__":
    main()
