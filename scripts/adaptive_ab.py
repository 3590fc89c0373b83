"""The adaptive launch against the plain one on one MI355X: one context, the bench's C2 settings (cornell-box 1920x1080,
depth 8, SAH) and the 870 k-triangle procedural scene (depth 6).  1024 plain frames, then for each ConvergencePercentage -- 0 (every lit pixel live),
0.001 (the reference's default) and two values taken from the error distribution to leave about 50 % and 10 % live -- the time of one 64-frame call
(adaptive_min_frames = 1023, so that the call's first frame already skips):
adaptive, adaptive off (frame groups, the default) and frame_group = -1 (the dense one-pixel-per-lane kernel); and the live-list pass alone
(the adaptive call's events: whole call minus its path-tracing launch).  Each call starts from the same state (1024 frames rendered again, the
same bits), the three forms alternate, and the best of `--reps` is kept.

    python scripts/adaptive_ab.py [--reps 3] [--out profiles/adaptive_ab.json]
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
SCENES = {"c2_cornell_box": (CORNELL, 8, {}), "c3_proc870k": ("proc0:870000", 6, {"reinsertion_passes": 3, "reinsertion_share": 3})}
W, H, BASE, CALL = 1920, 1080, 1024, 64


def errors(o, q):
    with np.errstate(all="ignore"):
        c = o[..., :3] / o[..., 3:4]; j = q[..., :3] / q[..., 3:4]
        black = (c[..., 0] <= 0) & (c[..., 1] <= 0) & (c[..., 2] <= 0)
        err = ((np.abs(j[..., 0] - c[..., 0]) + np.abs(j[..., 1] - c[..., 1])) + np.abs(j[..., 2] - c[..., 2])) / np.sqrt((c[..., 0] + c[..., 1]) + c[..., 2])
    return black, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_ab.json"))
    args = ap.parse_args()
    res = {"frame": [W, H], "base_frames": BASE, "call_frames": CALL, "reps": args.reps, "scenes": {}}
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

        def base(mode, thr):
            tb.SetOption("adaptive", 1 if mode == "adaptive" else 0)
            tb.SetOption("adaptive_min_frames", BASE - 1)       # the call's first frame (1024) may skip: the live list is packed from it on
            tb.SetOption("frame_group", -1 if mode == "dense" else 0)
            s.ConvergencePercentage = thr
            tb.InvalidateHistory(); tb.Render(W, H, BASE, s, 0.0)

        base("default", 0.0)
        o, q = tb.ReadAccumulation(jittered=True)
        black, err = errors(o, q)
        e = np.sort(err[~black & np.isfinite(err)])
        thresholds = {"all_lit_live": 0.0, "reference_0.001": 0.001, "about_50pct_live": float(np.float32(e[len(e) // 2])),
                      "about_10pct_live": float(np.float32(e[int(len(e) * 0.9)]))}
        rows = {}
        for label, thr in thresholds.items():
            live_share = float(1.0 - (black | (err < np.float32(thr))).mean())
            best = {}
            for _ in range(args.reps):
                for mode in ("adaptive", "default", "dense"):
                    base(mode, thr)
                    tb.Render(W, H, CALL, s, 0.0)
                    ms = tb.LastRenderMs()
                    row = {"ms": ms}
                    if mode == "adaptive":
                        assert tb.GetOption("last_adaptive") == 1
                        row["kernel_ms"] = tb.GetOption("last_kernel_us") / 1000.0
                        row["live_list_ms"] = ms - row["kernel_ms"]
                        row["live_pixels"] = tb.LivePixels()
                    if mode not in best or ms < best[mode]["ms"]:
                        best[mode] = row
            rows[label] = {"threshold": thr, "live_share_at_start": live_share, "live_pixels": best["adaptive"]["live_pixels"],
                           "adaptive_ms": best["adaptive"]["ms"], "adaptive_kernel_ms": best["adaptive"]["kernel_ms"],
                           "live_list_ms": best["adaptive"]["live_list_ms"], "default_ms": best["default"]["ms"], "dense_ms": best["dense"]["ms"]}
            print(name, label, json.dumps(rows[label]), flush=True)
        res["scenes"][name] = rows
        for k in opts:
            tb.SetOption(k, -1 if k == "reinsertion_passes" else 100)
    tb.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
