#!/usr/bin/env python3
"""How far the mean and the a-trous-denoised still are from a converged render: the cornell box at 256 x 256, relMSE, PSNR
and SSIM at 4, 16 and 64 frames against a 16384-frame reference of another time seed, all through tb_compare.

    python scripts/compare_quality.py [profiles/compare_quality.json]

Prints the table of DESIGN.md section 18 in markdown."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
W = H = 256
REFERENCE_FRAMES, FRAMES = 16384, (4, 16, 64)


def main():
    from tracerboy_amd import api
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "compare_quality.json")
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 4
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.Render(W, H, REFERENCE_FRAMES, s, 7.0)
        acc = tb.ReadAccumulation()
        reference = np.ones_like(acc); reference[..., :3] = acc[..., :3] / acc[..., 3:4]
    rows = []
    with api.TracerBoy(0) as tb:
        tb.SetOption("aov", 1)
        tb.LoadScene(CORNELL)
        tb.SetReference(reference)
        done = 0
        for n in FRAMES:
            tb.Render(W, H, n - done, s, 0.0); done = n
            mean = tb.Compare(0)
            tb.Denoise(read=False)
            denoised = tb.Compare(1)
            rows.append({"frames": n, "mean": {k: mean[k] for k in ("rel_mse", "psnr", "ssim", "mse")},
                         "denoised": {k: denoised[k] for k in ("rel_mse", "psnr", "ssim", "mse")}})
    print("| frames | relMSE mean | relMSE denoised | PSNR mean (dB) | PSNR denoised (dB) | SSIM mean | SSIM denoised |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        m, d = r["mean"], r["denoised"]
        print("| %d | %.5f | %.5f | %.2f | %.2f | %.4f | %.4f |" % (r["frames"], m["rel_mse"], d["rel_mse"], m["psnr"], d["psnr"], m["ssim"], d["ssim"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"scene": "cornell-box", "width": W, "height": H, "reference_frames": REFERENCE_FRAMES, "max_bounces": 4, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
