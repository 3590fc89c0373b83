#!/usr/bin/env python3
"""What light probes cost on one MI355X: GPU time of a bake's four stages, and of the sampler.

    python scripts/probe_rate.py [profiles/probe_rate.json]

Scenes: cornell-box and tb_load_procedural(0, 870 000).  On each a 16 x 16 x 16 grid of 4096 probes inside the scene's box is baked REPEATS times at
M = 16 with 16 samples (2^20 rays: one batch), positions in a device tensor, records into a device tensor.  Recorded per scene, as the median, the
fastest and the slowest of the repeats after one bake that is not counted: the options last_probes_rays_us (the ray records), last_probes_trace_us (the
radiance query), last_probes_hits_us (the closest-hit query) and last_probes_project_us (the SH projection) -- HIP events, microseconds -- and
(rays + project) / (trace + hits): what this section adds around the two queries as a share of them.
SampleProbes at 2^20 seeded points of the same box against the baked grid, device tensors: the host's clock around the call, which ends in a
synchronise of the context's stream (the library exposes no events for it), so launch and allocation of the result are inside.  No time here is a gate."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID, RES, SAMPLES, REPEATS, POINTS = (16, 16, 16), 16, 16, 7, 1 << 20
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
STAGES = ("rays_us", "trace_us", "hits_us", "project_us")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    import torch
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probe_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("probe_rate.py measures on the GPU: no device found")
    settings = api.GetDefaultOutputSettings()
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "grid": list(GRID), "resolution": RES, "samples": SAMPLES,
              "repeats": REPEATS, "sample_points": POINTS, "unit": "microseconds of GPU time (HIP events); sample_us: host clock around the synchronous call", "scenes": {}}
    with api.TracerBoy(0) as tb:
        for name in ("cornell-box", "proc0:870000"):
            tb.LoadScene(CORNELL) if name == "cornell-box" else tb.LoadProcedural(0, 870000, 1234)
            info = tb.SceneInfo()
            lo, hi = np.array(info.sceneMin[:]), np.array(info.sceneMax[:])
            grid = api.ProbeGrid.in_bounds(lo, hi, GRID)
            pos = torch.from_numpy(api.probe_grid_positions(grid)).to("cuda:0")
            rows = {k: [] for k in STAGES}
            for i in range(REPEATS + 1):
                probes = tb.BakeProbes(pos, RES, SAMPLES, settings=settings)
                if i:
                    for k in STAGES:
                        rows[k].append(tb.GetOption("last_probes_" + k))
            r = {k: stats(v) for k, v in rows.items()}
            r["batches"] = tb.GetOption("last_probes_batches"); r["triangles"] = info.numTriangles
            r["rays_plus_project_share_of_trace_plus_hits"] = (r["rays_us"]["median"] + r["project_us"]["median"]) / max(r["trace_us"]["median"] + r["hits_us"]["median"], 1)
            rng = np.random.default_rng(25)
            pts = torch.from_numpy((lo + rng.random((POINTS, 3)) * (hi - lo)).astype(np.float32)).to("cuda:0")
            nrm = rng.normal(size=(POINTS, 3)); nrm = torch.from_numpy((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)).to("cuda:0")
            times = []
            for i in range(REPEATS + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); tb.SampleProbes(grid, probes, pts, nrm, resolution=RES); t1 = time.perf_counter()
                if i:
                    times.append(int((t1 - t0) * 1e6 + 0.5))
            r["sample_us"] = stats(times)
            result["scenes"][name] = r
            print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
