#!/usr/bin/env python3
"""What a moved scene costs on one MI355X: the refit commit against the only ways the parent commit has to the same result.

    python scripts/refit_rate.py [profiles/refit_rate.json [SCENE ...]]

Scenes: cornell-box and tb_load_procedural(0, N) for N = 10 000, 870 000 and 3 000 000 -- or those named: cornell-box, procK:N.  Every vertex that
does not belong to an emissive geometry is displaced by a seeded offset of 5 % of the scene's extent (torch, on the device).  Forms:
  commit_chain   tb_update_positions (device pointer) + tb_commit_geometry with one launch per level of the schedule (TB_REFIT_FORM=0), from the call
                 to a synced stream, host clock; kernels_chain: its kernels alone (option last_refit_us, HIP events)
  commit_fused   the same with the top levels fused into one single-workgroup kernel (TB_REFIT_FORM=1); kernels_fused
  commit         what ships (TB_REFIT_FORM unset)
  rebuild        tb_update_positions + tb_commit_geometry(TB_GEOMETRY_REBUILD)
  reload         tb_load_procedural / tb_load_scene of the scene: all the parent commit can do (and it loads the UNMOVED scene)
Everything runs once first (the first update of a topology also makes the refit's tables: table_build_ms).  Then ROUNDS rounds in which the forms alternate; in a round a form repeats for at least WINDOW seconds (the slow forms at
least once) and the window's value is the mean time of a call, in microseconds.  Reported per form: the median window, the fastest and the slowest.
Then the closest-hit rate of tb_trace_rays (2^20 jittered camera rays, device path, Mrays/s) on the refit tree and on the rebuilt tree of the same
moved scene, alternating in the same way (each switch is a commit)."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
ROUNDS, WINDOW = 5, 0.2
N_RAYS = 1 << 20
FORMS = {"commit_chain": "0", "commit_fused": "1", "commit": ""}


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def load(tb, scene):
    if scene == "cornell-box":
        tb.LoadScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt"))
    else:
        kind, triangles = scene[4:].split(":")
        tb.LoadProcedural(int(kind), int(triangles), 1234)


def device_positions(torch, tb):
    """(positions, displaced positions) on the device, from the context's own view; the vertices of emissive geometries stay."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dynamic_cases as dc
    view = tb.HostSceneView()
    image = dc.bvh_bytes(view)
    pos = dc.positions_of(view, image)
    keep = torch.from_numpy(dc.emissive_vertices(view)).to("cuda:0")
    p = torch.from_numpy(pos).to("cuda:0")
    g = torch.Generator(device="cuda:0"); g.manual_seed(31)
    moved = p + (torch.rand(p.shape, generator=g, dtype=torch.float32, device="cuda:0") * 2 - 1) * (0.05 * dc.extent(pos))
    moved = torch.where(keep[:, None], p, moved).contiguous()
    return p, moved


def main():
    import torch
    from tracerboy_amd import api, build
    from ray_query_rate import camera_rays
    import ray_query_rate
    ray_query_rate.N = N_RAYS
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refit_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("refit_rate.py measures on the GPU: no device found")
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "rounds": ROUNDS, "window_s": WINDOW,
              "unit": "microseconds per call; Mrays/s for trace_*", "rays": N_RAYS, "scenes": {}}
    for scene in sys.argv[2:] or ["cornell-box", "proc0:10000", "proc0:870000", "proc0:3000000"]:
        with api.TracerBoy(0) as tb:
            load(tb, scene)
            info = tb.SceneInfo()
            p, moved = device_positions(torch, tb)
            flip = [moved, p]

            def commit(form, rebuild=False):
                os.environ["TB_REFIT_FORM"] = FORMS.get(form, "")
                try:
                    flip.reverse()
                    tb.UpdatePositions(flip[0]); tb.CommitGeometry(rebuild)
                finally:
                    os.environ["TB_REFIT_FORM"] = ""

            def call(form):
                if form == "reload":
                    load(tb, scene)
                elif form == "rebuild":
                    commit(form, True)
                else:
                    commit(form)

            forms = list(FORMS) + ["rebuild", "reload"]
            t0 = time.perf_counter(); tb.UpdatePositions(p[:1]); table_build_ms = (time.perf_counter() - t0) * 1e3
            for f in forms:
                call(f)                                              # everything once
            windows = {f: [] for f in forms}; kernels = {"kernels_chain": [], "kernels_fused": []}
            for _ in range(ROUNDS):
                for f in forms:
                    if f in FORMS:
                        call(f)                                      # untimed: the first update after a rebuild or a reload makes the tables again
                    calls, t0 = 0, time.perf_counter()
                    while True:
                        call(f); calls += 1
                        dt = time.perf_counter() - t0
                        if dt >= WINDOW:
                            break
                    windows[f].append(dt / calls * 1e6)
                    if f in ("commit_chain", "commit_fused"):
                        kernels["kernels_" + f[7:]].append(float(tb.GetOption("last_refit_us")))
            row = {"triangles": info.numTriangles, "vertices": info.numVertices, "bvh_max_depth": info.bvhMaxDepth, "table_build_ms": table_build_ms,
                   "forms": {f: stats(v) for f, v in list(windows.items()) + list(kernels.items())}}
            # closest-hit rate on the refit tree against the rebuilt tree of the same moved scene
            load(tb, scene)
            rays = camera_rays(torch, tb.GetCamera(), 1)
            rates = {"trace_refit": [], "trace_rebuilt": []}
            answers = {}
            for _ in range(ROUNDS):
                for name in rates:
                    if name == "trace_refit":                        # back to the loaded topology, then the refit of the move
                        load(tb, scene); tb.UpdatePositions(moved); tb.CommitGeometry()
                    else:
                        tb.CommitGeometry(rebuild=True)
                    answers[name] = tb.TraceRays(rays, api.RAYS_CLOSEST)[:, 0].clone()
                    calls, t0 = 0, time.perf_counter()
                    while True:
                        tb.TraceRays(rays, api.RAYS_CLOSEST); calls += 1
                        dt = time.perf_counter() - t0
                        if dt >= WINDOW:
                            break
                    rates[name].append(calls * N_RAYS / dt / 1e6)
            row["forms"].update({k: stats(v) for k, v in rates.items()})
            row["trace_t_differ"] = int((answers["trace_refit"] != answers["trace_rebuilt"]).sum())
            result["scenes"][scene] = row
            print(scene, info.numTriangles, "triangles, depth", info.bvhMaxDepth, "T differs on", row["trace_t_differ"], "rays", flush=True)
            for f, s in row["forms"].items():
                print("    %-14s %12.1f  [%12.1f .. %12.1f]" % (f, s["median"], s["min"], s["max"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
