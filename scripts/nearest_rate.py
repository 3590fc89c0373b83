#!/usr/bin/env python3
"""What point queries deliver on one MI355X: Mqueries/s of tb_nearest_points and tb_bake_distance_field.

    python scripts/nearest_rate.py [profiles/nearest_rate.json [SCENE ...]]

Scenes: cornell-box and tb_load_procedural(0, 870 000) -- or those named: cornell-box, procK:N = tb_load_procedural(K, N).  Point sets, 128^3 =
2^21 points each, made on the device with torch:
  grid       the cell centres of a 128 x 128 x 128 grid over the scene's bounds, in cell order (i fastest)
  grid_shuf  the same points in a seeded random order
  near       points within 1 % of the extent of the surface: the grid points' nearest surface points, moved by a seeded random offset of up to
             0.01 x the largest side of the bounds
Forms, every one the synchronous call from Python with a host clock around it:
  records    NearestPoints on the set, device path (32-B records)
  field      BakeDistanceField(device=True) of the grid (4 B per cell, positions made in the kernel); reported with the set `grid` only
The parent commit offers nothing to compare with, so no ratio is formed: the numbers are recorded.  Everything runs once first.  Then ROUNDS
rounds in which sets and forms alternate; in a round a form repeats its call for at least WINDOW seconds and the window's rate is points / time.
Reported per form: the median window, the slowest and the fastest, and the kernel's own microseconds of the last call (option last_nearest_us)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE = 128
N = SIDE ** 3
ROUNDS, WINDOW = 7, 0.2


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    import numpy as np
    import torch
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nearest_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("nearest_rate.py measures on the GPU: no device found")
    # library: TB_LIB selects a measurement build (scripts/build_variant.py: -DTB_PQ_STACK_BOUNDS=1, the stack with the bound beside the ref)
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "library": os.path.basename(api.LIB_PATH), "points": N, "rounds": ROUNDS, "window_s": WINDOW,
              "unit": "Mqueries/s", "scenes": {}}
    for scene in sys.argv[2:] or ["cornell-box", "proc0:870000"]:
        with api.TracerBoy(0) as tb:
            if scene == "cornell-box":
                tb.LoadScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt"))
            else:
                kind, triangles = scene[4:].split(":")
                tb.LoadProcedural(int(kind), int(triangles), 1234)
            info = tb.SceneInfo()
            lo, hi = np.float64(info.sceneMin[:]), np.float64(info.sceneMax[:])
            extent = float((hi - lo).max())
            grid = api.ProbeGrid.in_bounds(lo, hi, (SIDE, SIDE, SIDE))
            cells = torch.full((N, 4), float("inf"), dtype=torch.float32, device="cuda:0")
            cells[:, 0:3] = torch.from_numpy(api.probe_grid_positions(grid)).cuda()
            first = tb.NearestPoints(cells)
            g = torch.Generator(device="cuda:0"); g.manual_seed(3)
            d = torch.randn((N, 3), generator=g, dtype=torch.float32, device="cuda:0")
            d = d / torch.linalg.norm(d, dim=1, keepdim=True).clamp_min(1e-20) * (torch.rand((N, 1), generator=g, dtype=torch.float32, device="cuda:0") * 0.01 * extent)
            near = cells.clone(); near[:, 0:3] = first[:, 0:3] + d
            sets = {"grid": cells, "grid_shuf": cells[torch.randperm(N, generator=g, device="cuda:0")].contiguous(), "near": near}
            calls = {(name, "records"): (lambda p=p: tb.NearestPoints(p)) for name, p in sets.items()}
            calls[("grid", "field")] = lambda: tb.BakeDistanceField(grid, device=True)
            field = calls[("grid", "field")]()                      # everything once; and the field is the records' distances
            differ = int((field.reshape(-1) != first[:, 3]).sum())
            kernel_us = {}
            for key, call in calls.items():
                call(); kernel_us[key] = int(tb.GetOption("last_nearest_us"))
            windows = {key: [] for key in calls}
            for _ in range(ROUNDS):
                for key, call in calls.items():
                    n, t0 = 0, time.perf_counter()
                    while True:
                        call(); n += 1
                        dt = time.perf_counter() - t0
                        if dt >= WINDOW:
                            break
                    windows[key].append(n * N / dt / 1e6)
            row = {"triangles": info.numTriangles, "bvh_max_depth": info.bvhMaxDepth, "field_differs_from_records": differ, "sets": {}}
            for (name, form), v in windows.items():
                s = stats(v); s["kernel_us"] = kernel_us[(name, form)]; s["kernel_mqueries_per_s"] = N / max(kernel_us[(name, form)], 1)
                row["sets"].setdefault(name, {})[form] = s
                print("%-14s %-10s %-8s %9.1f  [%9.1f .. %9.1f] Mqueries/s   kernel %8d us" % (scene, name, form, s["median"], s["min"], s["max"], s["kernel_us"]),
                      flush=True)
            result["scenes"][scene] = row
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
