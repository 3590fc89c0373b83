#!/usr/bin/env python3
"""What the image-quality metrics cost on one MI355X.

    python scripts/compare_timing.py [profiles/compare_timing.json]

tb_compare(TB_COMPARE_MEAN) at 1920 x 1080 and 3840 x 2160, with and without SSIM: GPU microseconds from the HIP events around the call's kernels
(tb_compare_result::gpu_us), 3 warm-up calls, then the median of 10 with minimum and maximum -- the method of scripts/fsr_timing.py.  Beside each,
from the same run: what the comparison replaces, one tb_read_accum of the RGBA32F surface of that size into a pageable host array that was
allocated and touched beforehand (wall clock around the synchronous call: the copy, not the allocation), and the bytes floor 2 x 16 B x w x h / 8 TB/s with the share of it the call reaches."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
WARMUP, ROUNDS = 3, 10
SIZES = ((1920, 1080), (3840, 2160))
HBM_BYTES_PER_S = 8.0e12


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "compare_timing.json")
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 3
    with_ssim, without = api.GetDefaultCompareSettings(), api.GetDefaultCompareSettings()
    without.flags = 0
    result = {"kernel_digest": build.kernel_digest(), "warmup": WARMUP, "rounds": ROUNDS, "sizes": {}}
    for (w, h) in SIZES:
        with api.TracerBoy(0) as tb:
            tb.LoadScene(CORNELL)
            tb.Render(w, h, 2, s, 0.0)
            acc = tb.ReadAccumulation()
            reference = np.ones_like(acc); reference[..., :3] = acc[..., :3] / acc[..., 3:4]
            tb.Render(w, h, 2, s, 0.0)            # the test picture: four frames against the mean of the first two
            tb.SetReference(reference)
            host = np.zeros((h, w, 4), np.float32)            # allocated and touched once: the figure is the copy's, not first-touch page faults
            host_ptr = host.ctypes.data_as(C.c_void_p)
            samples = {"ssim_us": [], "pointwise_us": [], "read_accum_us": []}
            last = None
            for i in range(WARMUP + ROUNDS):      # the variants alternate inside every round
                a = tb.Compare(0, with_ssim); b = tb.Compare(0, without)
                t0 = time.perf_counter(); tb._check(tb._L.tb_read_accum(tb._ctx, host_ptr, None)); t1 = time.perf_counter()
                if i >= WARMUP:
                    samples["ssim_us"].append(a["gpu_us"]); samples["pointwise_us"].append(b["gpu_us"]); samples["read_accum_us"].append((t1 - t0) * 1e6)
                last = a
            floor_us = 2.0 * 16.0 * w * h / HBM_BYTES_PER_S * 1e6
            entry = {k: stats(v) for k, v in samples.items()}
            entry["bytes_floor_us"] = floor_us
            entry["pointwise_share_of_floor"] = floor_us / entry["pointwise_us"]["median"]
            entry["ssim_share_of_floor"] = floor_us / entry["ssim_us"]["median"]
            entry["metrics"] = {k: last[k] for k in ("pixels", "mse", "rel_mse", "psnr", "ssim", "ssim_windows")}
            result["sizes"]["%dx%d" % (w, h)] = entry
            print("%dx%d: with SSIM %.1f us, pointwise alone %.1f us, tb_read_accum %.0f us, bytes floor %.1f us (pointwise reaches %.0f %% of it)" % (
                w, h, entry["ssim_us"]["median"], entry["pointwise_us"]["median"], entry["read_accum_us"]["median"], floor_us, 100 * entry["pointwise_share_of_floor"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
