#!/usr/bin/env python3
"""What winding numbers deliver on one MI355X: Mqueries/s of tb_winding_numbers, tb_bake_winding_field and
tb_bake_distance_field_winding; the moment fit beside the refit.

    python scripts/winding_rate.py [profiles/winding_rate.json [SCENE ...]]

Scenes: cornell-box and tb_load_procedural(0, 870 000) -- or those named, as scripts/nearest_rate.py names them.  Points: the 128^3 = 2^21 cell
centres of a grid over the scene's bounds, on the device, in cell order (`grid`) and in a seeded random order (`grid_shuf`).
Forms, every one the synchronous call from Python with a host clock around it, scripts/nearest_rate.py's method:
  numbers b<beta>       WindingNumbers on the set, device path (4 B per point), beta 2, 3 (the default) and 4; beta = inf -- every triangle for every
                        point -- on scenes of at most EXACT_MAX_TRIANGLES triangles only: on the 870 k scene it is 1.8 x 10^12 solid angles, left out
  field                 BakeWindingField(device=True) of the grid, default beta (positions made in the kernel); with the set `grid` only
  distance / distance_w BakeDistanceField(device=True) of the grid, unsigned, and with winding_beta = the default: the sign pass's price
The parent commit offers nothing to compare with, so no ratio is formed.  Everything runs once first.  Then ROUNDS rounds in which the forms
alternate; in a round a form repeats its call for at least WINDOW seconds.  Reported per form: the median window, the slowest and the fastest, and
the kernels' own microseconds of one more call after the rounds (option last_winding_us; last_nearest_us for `distance`).
Fit: a commit of displaced positions (scripts/refit_rate.py's) and the winding call after it, FIT_ROUNDS times: the refit's kernels (last_refit_us)
beside the moment fit's (last_winding_fit_us), medians."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
SIDE = 128
N = SIDE ** 3
ROUNDS, WINDOW, FIT_ROUNDS = 7, 0.2, 7
BETAS = (2.0, 3.0, 4.0)
EXACT_MAX_TRIANGLES = 1000


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    import numpy as np
    import torch
    from tracerboy_amd import api, build
    from refit_rate import device_positions
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "winding_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("winding_rate.py measures on the GPU: no device found")
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "points": N, "rounds": ROUNDS, "window_s": WINDOW,
              "default_beta": api.WINDING_BETA, "unit": "Mqueries/s; microseconds for fit", "scenes": {}}
    for scene in sys.argv[2:] or ["cornell-box", "proc0:870000"]:
        with api.TracerBoy(0) as tb:
            if scene == "cornell-box":
                tb.LoadScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt"))
            else:
                kind, triangles = scene[4:].split(":")
                tb.LoadProcedural(int(kind), int(triangles), 1234)
            info = tb.SceneInfo()
            lo, hi = np.float64(info.sceneMin[:]), np.float64(info.sceneMax[:])
            grid = api.ProbeGrid.in_bounds(lo, hi, (SIDE, SIDE, SIDE))
            cells = torch.full((N, 4), float("inf"), dtype=torch.float32, device="cuda:0")
            cells[:, 0:3] = torch.from_numpy(api.probe_grid_positions(grid)).cuda()
            g = torch.Generator(device="cuda:0"); g.manual_seed(3)
            sets = {"grid": cells, "grid_shuf": cells[torch.randperm(N, generator=g, device="cuda:0")].contiguous()}
            betas = BETAS + ((float("inf"),) if info.numTriangles <= EXACT_MAX_TRIANGLES else ())
            calls = {}
            for name, p in sets.items():
                for beta in betas:
                    calls[(name, "numbers b%g" % beta)] = (lambda p=p, beta=beta: tb.WindingNumbers(p, beta=beta), "last_winding_us")
            calls[("grid", "field")] = (lambda: tb.BakeWindingField(grid, device=True), "last_winding_us")
            calls[("grid", "distance")] = (lambda: tb.BakeDistanceField(grid, device=True), "last_nearest_us")
            calls[("grid", "distance_w")] = (lambda: tb.BakeDistanceField(grid, device=True, winding_beta=api.WINDING_BETA), "last_winding_us")
            first = tb.WindingNumbers(cells)                           # everything once; and the field is the numbers
            differ = int((calls[("grid", "field")][0]().reshape(-1).view(torch.int32) != first.view(torch.int32)).sum())
            inside = float(torch.from_numpy(api.winding_inside(first.cpu().numpy())).float().mean())
            for call, option in calls.values():
                call()
            windows = {key: [] for key in calls}
            for _ in range(ROUNDS):
                for key, (call, option) in calls.items():
                    n, t0 = 0, time.perf_counter()
                    while True:
                        call(); n += 1
                        dt = time.perf_counter() - t0
                        if dt >= WINDOW:
                            break
                    windows[key].append(n * N / dt / 1e6)
            kernel_us = {}                                           # after the rounds: every form is warm
            for key, (call, option) in calls.items():
                call(); kernel_us[key] = int(tb.GetOption(option))
            row = {"triangles": info.numTriangles, "bvh_max_depth": info.bvhMaxDepth, "field_differs_from_numbers": differ, "share_inside": inside, "sets": {}}
            for (name, form), v in windows.items():
                s = stats(v); s["kernel_us"] = kernel_us[(name, form)]; s["kernel_mqueries_per_s"] = N / max(kernel_us[(name, form)], 1)
                row["sets"].setdefault(name, {})[form] = s
                print("%-14s %-10s %-12s %9.1f  [%9.1f .. %9.1f] Mqueries/s   kernel %8d us" % (scene, name, form, s["median"], s["min"], s["max"], s["kernel_us"]),
                      flush=True)
            p, moved = device_positions(torch, tb)                   # the fit beside the refit
            flip, refit_us, fit_us = [moved, p], [], []
            for _ in range(FIT_ROUNDS + 1):
                flip.reverse()
                tb.UpdatePositions(flip[0]); tb.CommitGeometry()
                refit_us.append(float(tb.GetOption("last_refit_us")))
                tb.WindingNumbers(cells[:256])
                fit_us.append(float(tb.GetOption("last_winding_fit_us")))
            row["fit"] = {"refit_us": stats(refit_us[1:]), "winding_fit_us": stats(fit_us[1:])}
            print("%-14s refit %8.1f us   moment fit %8.1f us (medians of %d)" % (scene, row["fit"]["refit_us"]["median"], row["fit"]["winding_fit_us"]["median"], FIT_ROUNDS),
                  flush=True)
            result["scenes"][scene] = row
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
