#!/usr/bin/env python3
"""What new shading normals cost a deforming scene on one MI355X: the recomputation at the commit against the only way the
parent commit has, normals made by the caller in torch and handed to tb_update_normals.

    python scripts/normals_rate.py [profiles/normals_rate.json [SCENE ...]]

Scenes: cornell-box and tb_load_procedural(0, N) for N = 10 000, 870 000 and 3 000 000 -- or those named: cornell-box, procK:N.  Every vertex that
does not belong to an emissive geometry is displaced as scripts/refit_rate.py displaces it.  Rows:
  recompute   tb_update_positions (device pointer) + tb_recompute_normals (everything) + tb_commit_geometry, from the call to a synced stream,
              host clock; recompute_kernels: option last_refit_us, the refit's kernels and the two normal launches (HIP events)
  torch       the caller's way: face vectors by torch.cross, three index_add_ into a per-vertex sum, a normalise, all on the device; then
              tb_update_positions + tb_update_normals (device pointers) + tb_commit_geometry; torch_kernels: last_refit_us of that commit plus
              the torch kernels' own time (torch.cuda events around them)
Everything runs once first (the first call of a topology makes the tables: table_build_ms).  Then ROUNDS rounds in which the rows alternate; in a
round a row repeats for at least WINDOW seconds and the window's value is the mean time of a call, in microseconds.  Reported per row: the median
window, the fastest and the slowest.  max_normal_difference: the largest component difference between the two ways' normals (the torch sum is
atomic, its order is not the rule's).
Then, for proc0:870000, tb_load_meshes of the scene's arrays (numpy, and device tensors) against tb_load_procedural of the same scene, in
milliseconds, LOAD_ROUNDS alternations."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
ROUNDS, WINDOW, LOAD_ROUNDS = 5, 0.2, 3
LOAD_SCENE = (0, 870000, 1234)


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def torch_normals(torch, p, tri, keep, loaded):
    v0, v1, v2 = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    f = torch.cross(v2 - v0, v2 - v1, dim=1)
    acc = torch.zeros_like(p)
    for k in range(3):
        acc.index_add_(0, tri[:, k], f)
    n = acc / acc.norm(dim=1, keepdim=True).clamp_min(1e-20)
    return torch.where(keep[:, None], loaded, n).contiguous()        # an emissive geometry's normals stay (section 21)


def main():
    import numpy as np
    import torch
    import dynamic_cases as dc
    import mesh_cases as mc
    from refit_rate import load, device_positions
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "normals_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("normals_rate.py measures on the GPU: no device found")
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "rounds": ROUNDS, "window_s": WINDOW,
              "unit": "microseconds per commit; milliseconds for loads", "scenes": {}}
    for scene in sys.argv[2:] or ["cornell-box", "proc0:10000", "proc0:870000", "proc0:3000000"]:
        with api.TracerBoy(0) as tb:
            load(tb, scene)
            info = tb.SceneInfo()
            view = tb.HostSceneView()
            p, moved = device_positions(torch, tb)
            tri = torch.from_numpy(dc.sorted_tri_vertices(view).astype(np.int64)).to("cuda:0")
            keep = torch.from_numpy(dc.emissive_vertices(view)).to("cuda:0")
            loaded = torch.from_numpy(np.ascontiguousarray(mc.vertex_buffer(view)[:, 0:3])).to("cuda:0")
            nv = int(info.numVertices)
            flip = [moved, p]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch_us = [0.0]

            def call(row):
                flip.reverse()
                if row == "recompute":
                    tb.UpdatePositions(flip[0]); tb.RecomputeNormals(0, nv); tb.CommitGeometry()
                else:
                    ev[0].record(); n = torch_normals(torch, flip[0], tri, keep, loaded); ev[1].record()
                    tb.UpdatePositions(flip[0]); tb.UpdateNormals(n); tb.CommitGeometry()
                    torch_us[0] = ev[0].elapsed_time(ev[1]) * 1e3

            rows = ["recompute", "torch"]
            t0 = time.perf_counter(); tb.RecomputeNormals(0, 1); table_build_ms = (time.perf_counter() - t0) * 1e3
            for r in rows:
                call(r)                                                  # everything once
            windows = {r: [] for r in rows}; kernels = {r + "_kernels": [] for r in rows}
            for _ in range(ROUNDS):
                for r in rows:
                    calls, t0 = 0, time.perf_counter()
                    while True:
                        call(r); calls += 1
                        dt = time.perf_counter() - t0
                        if dt >= WINDOW:
                            break
                    windows[r].append(dt / calls * 1e6)
                    kernels[r + "_kernels"].append(float(tb.GetOption("last_refit_us")) + (torch_us[0] if r == "torch" else 0.0))
            # the two ways' normals of the same positions
            tb.UpdatePositions(moved); tb.RecomputeNormals(0, nv); tb.CommitGeometry()
            ours = np.ascontiguousarray(mc.vertex_buffer(tb.HostSceneView())[:, 0:3])
            theirs = torch_normals(torch, moved, tri, keep, loaded).cpu().numpy()
            named = np.zeros(nv, bool); named[tri.cpu().numpy().reshape(-1)] = True
            row = {"triangles": info.numTriangles, "vertices": nv, "table_build_ms": table_build_ms,
                   "max_normal_difference": float(np.abs(ours[named] - theirs[named]).max()),
                   "forms": {k: stats(v) for k, v in list(windows.items()) + list(kernels.items())}}
            result["scenes"][scene] = row
            print(scene, info.numTriangles, "triangles,", nv, "vertices; normals differ by at most", row["max_normal_difference"], flush=True)
            for f, s in row["forms"].items():
                print("    %-18s %12.1f  [%12.1f .. %12.1f]" % (f, s["median"], s["min"], s["max"]), flush=True)
    if len(sys.argv) <= 2:
        hs = api.HostScene(procedural=LOAD_SCENE)
        meshes, materials = mc.cut_meshes(hs)
        camera = hs.camera()
        on_device = mc.to_torch(meshes, int32=True)
        loads = {"load_procedural": [], "load_meshes_numpy": [], "load_meshes_device": []}
        with api.TracerBoy(0) as tb:
            for k in range(LOAD_ROUNDS + 1):                             # the first round is the warm-up
                for name in loads:
                    t0 = time.perf_counter()
                    if name == "load_procedural":
                        tb.LoadProcedural(*LOAD_SCENE)
                    else:
                        tb.LoadMeshes(meshes if name == "load_meshes_numpy" else on_device, materials, camera=camera, environment=np.ones((1, 1, 4), np.float32))
                    if k:
                        loads[name].append((time.perf_counter() - t0) * 1e3)
        result["load_870k_ms"] = {k: stats(v) for k, v in loads.items()}
        for f, s in result["load_870k_ms"].items():
            print("    %-18s %12.1f ms [%12.1f .. %12.1f]" % (f, s["median"], s["min"], s["max"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
