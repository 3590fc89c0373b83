"""Sample budgets on one MI355X, by the method of scripts/adaptive_per_call_ab.py: one context, the bench's C2 settings
(cornell-box 1920x1080, depth 8, SAH) and the 870 k-triangle procedural scene (depth 6); 1024 plain frames, then the time of one 64-frame call per
form from that same state, the forms alternating, best of `--reps`.

  plain        no budget: the default frame-group call
  adaptive100  the per-call adaptive call with a threshold no error is below (the black rule still drops black pixels: the live share is reported)
  budget_all   an all-0xffffffff budget: what having a budget set costs
  crop_quarter a budget that is 0xffffffff in the centred window of half the width and half the height, 0 elsewhere
and, from HIP events, the list pass and fold of a budgeted call (last_render_ms - last_kernel_us: what the call spends outside its path-tracing
launch) and tb_budget_stop_converged on its own (option last_budget_stop_us: prepare, prefilter, stop).

    python scripts/sample_budget_ab.py timing [--reps 2] [--out profiles/sample_budget.json]
    python scripts/sample_budget_ab.py quality [--out profiles/sample_budget.json]

A copy of this file run inside a checkout of the parent commit (whose library has no budgets) measures plain and adaptive100 only: the same-box
yardstick.  `quality`: cornell-box 128x96, depth 3, truth = frames [4096, 5120), section 12's relMSE of a noise-target schedule (first call 64 frames,
then calls of 64), of the uniform render of the same total sample count, and of --adaptive-test call schedules at a few thresholds with their
totals.  Results are merged into the JSON file under "timing" / "quality"."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tracerboy_amd import api  # noqa: E402

CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
SCENES = {"c2_cornell_box": (CORNELL, 8, {}), "c3_proc870k": ("proc0:870000", 6, {"reinsertion_passes": 3, "reinsertion_share": 3})}
W, H, BASE, CALL = 1920, 1080, 1024, 64
NEVER = 0xffffffff


def rel_mse(x, ref):
    x, ref = np.asarray(x, np.float64)[..., :3], np.asarray(ref, np.float64)[..., :3]
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


def mean_of(acc):
    with np.errstate(all="ignore"):
        return np.where(acc[..., 3:4] > 0, acc[..., :3] / acc[..., 3:4], 0.0)


def timing(args):
    budgets = hasattr(api.TracerBoy, "SetSampleBudget")
    modes = ["plain", "adaptive100"] + (["budget_all", "crop_quarter"] if budgets else [])
    res = {"frame": [W, H], "base_frames": BASE, "call_frames": CALL, "reps": args.reps, "library_has_budgets": budgets, "scenes": {}}
    crop = np.zeros((H, W), np.uint32); crop[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = NEVER
    tb = api.TracerBoy(0)
    for name, (scene, depth, opts) in SCENES.items():
        tb.SetOption("bvh_builder", 1)
        for k, v in opts.items():
            tb.SetOption(k, v)
        if scene.startswith("proc"):
            tb.LoadProcedural(0, 870000, 1234)
        else:
            tb.LoadScene(scene)
        s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = depth

        def base(mode):
            tb.SetOption("adaptive", 1 if mode == "adaptive100" else 0); tb.SetOption("adaptive_test", 1); tb.SetOption("adaptive_min_frames", BASE - 1)
            s.ConvergencePercentage = 0.0
            if budgets:
                tb.SetSampleBudget(None)
            tb.InvalidateHistory(); tb.Render(W, H, BASE, s, 0.0)
            if mode == "budget_all":
                tb.SetSampleBudget(np.full((H, W), NEVER, np.uint32))
            if mode == "crop_quarter":
                tb.SetSampleBudget(crop)

        best = {}
        for _ in range(args.reps):
            for mode in modes:
                base(mode)
                tb.Render(W, H, CALL, s, 0.0)
                row = {"ms": tb.LastRenderMs(), "kernel_ms": tb.GetOption("last_kernel_us") / 1000.0, "live_pixels": tb.LivePixels(),
                       "rule": tb.GetOption("last_plan_rule_pipeline")}
                row["list_pass_and_fold_ms"] = row["ms"] - row["kernel_ms"]
                if mode not in best or row["ms"] < best[mode]["ms"]:
                    best[mode] = row
        if budgets:                                             # the noise target on its own: its three passes between HIP events, best of 5
            base("budget_all")
            stop = []
            for _ in range(5):
                tb.SetSampleBudget(np.full((H, W), NEVER, np.uint32))
                stopped, live = tb.StopConverged(0.05, 64); stop.append(tb.GetOption("last_budget_stop_us") / 1000.0)
            best["stop_converged"] = {"gpu_ms": min(stop), "stopped": stopped, "live": live, "rel_error": 0.05}
        print(name, json.dumps(best), flush=True)
        res["scenes"][name] = best
        for k in opts:
            tb.SetOption(k, -1 if k == "reinsertion_passes" else 100)
        tb.SetOption("adaptive", 0)
    tb.close()
    return res


def quality(args):
    w, h, depth, first, chunk, cap = 128, 96, 3, 64, 64, 4096
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = depth
    res = {"frame": [w, h], "depth": depth, "truth_frames": [4096, 5120], "first_call": first, "chunk": chunk, "cap": cap, "noise_target": [], "adaptive": []}
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.BeginAccumulation(w, h, s, 0.0, first_frame=4096); tb.Render(w, h, 1024, s, 0.0)
        truth = mean_of(tb.ReadAccumulation())

        def uniform(total):
            frames = max(1, int(round(total / float(w * h))))
            tb.InvalidateHistory(); tb.Render(w, h, frames, s, 0.0)
            return frames, rel_mse(mean_of(tb.ReadAccumulation()), truth)

        for target in args.targets:
            tb.SetSampleBudget(None); tb.InvalidateHistory()
            tb.Render(w, h, first, s, 0.0); done = first
            while done < cap:
                stopped, live = tb.StopConverged(target, first)
                if live == 0:
                    break
                tb.Render(w, h, chunk, s, 0.0); done += chunk
            acc = tb.ReadAccumulation()
            total = float(acc[..., 3].sum())                    # box filter: sum w = samples
            row = {"rel_error": target, "frames": done, "samples": total, "rel_mse": rel_mse(mean_of(acc), truth)}
            tb.SetSampleBudget(None)
            row["uniform_frames"], row["uniform_rel_mse"] = uniform(total)
            res["noise_target"].append(row); print("noise_target", json.dumps(row), flush=True)
        tb.SetOption("adaptive", 1); tb.SetOption("adaptive_test", 1); tb.SetOption("adaptive_min_frames", first - 1)
        for thr in args.thresholds:
            s.ConvergencePercentage = thr
            tb.InvalidateHistory(); tb.Render(w, h, first, s, 0.0); done = first
            while done < cap:
                tb.Render(w, h, chunk, s, 0.0); done += chunk
                if tb.LivePixels() == 0:
                    break
            acc = tb.ReadAccumulation()
            row = {"threshold": thr, "frames": done, "samples": float(acc[..., 3].sum()), "rel_mse": rel_mse(mean_of(acc), truth)}
            res["adaptive"].append(row); print("adaptive", json.dumps(row), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "quality"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_budget.json"))
    ap.add_argument("--key", default=None, help="the key the result is stored under (default: timing / quality)")
    ap.add_argument("--targets", type=float, nargs="*", default=[0.1, 0.05, 0.025])
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.2, 0.1, 0.05])
    args = ap.parse_args()
    res = timing(args) if args.what == "timing" else quality(args)
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc[args.key or args.what] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
