"""The adaptive launch tested once per call (option adaptive_test = 1: the live pixels through the frame-group kernels) against the per-frame
adaptive launch, the default frame-group call and the dense one-pixel-per-lane call, on one MI355X.  The method of
scripts/adaptive_ab.py: one context, the bench's C2 settings (cornell-box 1920x1080, depth 8, SAH) and the 870 k-triangle procedural scene (depth
6); 1024 plain frames, then the time of one 64-frame call per form from that same state (adaptive_min_frames = 1023, so that the call's first frame
already skips), the forms alternating, best of `--reps`.  The thresholds are those of DESIGN.md section 10's first table, so that the rows line up.

    python scripts/adaptive_per_call_ab.py [--reps 2] [--out profiles/adaptive_per_call_ab.json] [--modes per_call,adaptive,default,dense]

Against another build of the library (TB_LIB=..., tracerboy_amd/api.py) that lacks the option -- the parent commit's, for the same-box check that
the three older forms kept their speed -- leave per_call out of --modes.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tracerboy_amd import api  # noqa: E402

CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
SCENES = {"c2_cornell_box": (CORNELL, 8, {}, (0.0, 0.001, 0.0108, 0.0270)),
          "c3_proc870k": ("proc0:870000", 6, {"reinsertion_passes": 3, "reinsertion_share": 3}, (0.0, 0.001, 0.00304, 0.0252))}
MODES = ("per_call", "adaptive", "default", "dense")
W, H, BASE, CALL = 1920, 1080, 1024, 64


def errors(o, q):
    with np.errstate(all="ignore"):
        c = o[..., :3] / o[..., 3:4]; j = q[..., :3] / q[..., 3:4]
        black = (c[..., 0] <= 0) & (c[..., 1] <= 0) & (c[..., 2] <= 0)
        err = ((np.abs(j[..., 0] - c[..., 0]) + np.abs(j[..., 1] - c[..., 1])) + np.abs(j[..., 2] - c[..., 2])) / np.sqrt((c[..., 0] + c[..., 1]) + c[..., 2])
    return black, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_per_call_ab.json"))
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()
    modes = [m for m in MODES if m in args.modes.split(",")]
    res = {"frame": [W, H], "base_frames": BASE, "call_frames": CALL, "reps": args.reps, "library": os.path.relpath(api.LIB_PATH, ROOT), "scenes": {}}
    tb = api.TracerBoy(0)
    for name, (scene, depth, opts, thresholds) in SCENES.items():
        tb.SetOption("bvh_builder", 1)
        for k, v in opts.items():
            tb.SetOption(k, v)
        if scene.startswith("proc"):
            tb.LoadProcedural(0, 870000, 1234)
        else:
            tb.LoadScene(scene)
        s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = depth

        def base(mode, thr):
            tb.SetOption("adaptive", 1 if mode in ("adaptive", "per_call") else 0)
            if "per_call" in modes:
                tb.SetOption("adaptive_test", 1 if mode == "per_call" else 0)
            tb.SetOption("adaptive_min_frames", BASE - 1)       # the call's first frame (1024) may skip: the live list is packed from it on
            tb.SetOption("frame_group", -1 if mode == "dense" else 0)
            s.ConvergencePercentage = thr
            tb.InvalidateHistory(); tb.Render(W, H, BASE, s, 0.0)

        base("default", 0.0)
        o, q = tb.ReadAccumulation(jittered=True)
        black, err = errors(o, q)
        rows = {}
        for thr in thresholds:
            label = "%g" % thr
            live_share = float(1.0 - (black | (err < np.float32(thr))).mean())
            best = {}
            for _ in range(args.reps):
                for mode in modes:
                    base(mode, thr)
                    tb.Render(W, H, CALL, s, 0.0)
                    ms = tb.LastRenderMs()
                    row = {"ms": ms}
                    if mode in ("adaptive", "per_call"):
                        assert tb.GetOption("last_adaptive") == 1 and tb.GetOption("last_plan_rule_pipeline") == (8 if mode == "per_call" else 7)
                        row["kernel_ms"] = tb.GetOption("last_kernel_us") / 1000.0
                        row["live_pixels"] = tb.LivePixels()
                        row["copy_waves"] = tb.GetOption("last_copy_waves"); row["frame_group"] = tb.GetOption("last_plan_frame_group")
                    if mode not in best or ms < best[mode]["ms"]:
                        best[mode] = row
            rows[label] = {"threshold": thr, "live_share_at_start": live_share}
            if "per_call" in best:
                rows[label].update({"live_pixels": best["per_call"]["live_pixels"], "per_call_ms": best["per_call"]["ms"],
                                    "per_call_kernel_ms": best["per_call"]["kernel_ms"], "per_call_copy_waves": best["per_call"]["copy_waves"],
                                    "per_call_frame_group": best["per_call"]["frame_group"]})
            if "adaptive" in best:
                assert best["adaptive"]["live_pixels"] == rows[label].get("live_pixels", best["adaptive"]["live_pixels"])
                rows[label]["per_frame_ms"] = best["adaptive"]["ms"]
            for m in ("default", "dense"):
                if m in best:
                    rows[label][m + "_ms"] = best[m]["ms"]
            print(name, label, json.dumps(rows[label]), flush=True)
        res["scenes"][name] = rows
        for k in opts:
            tb.SetOption(k, -1 if k == "reinsertion_passes" else 100)
        tb.SetOption("adaptive", 0); tb.SetOption("frame_group", 0)
        if "per_call" in modes:
            tb.SetOption("adaptive_test", 0)
    tb.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
