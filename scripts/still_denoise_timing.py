"""What the denoise of a progressive render costs on one MI355X: GPU time of the whole chain of tb_denoise -- prepare,
prefilter, the a-trous passes, finish -- from HIP events (option last_denoise_us), at 1080p and 4K, cornell-box, 16 spp, default filter settings
(5 passes), and of the chain without a filter pass (the three passes of dn_kernels.hip alone).

    python scripts/still_denoise_timing.py [profiles/still_denoise.json]

One context per size, both rendered before anything is timed; a warming call each, then ROUNDS rounds that alternate between the two sizes and,
inside a round, between the chain with and without its filter passes, so that every figure has ROUNDS samples spread over the whole run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
ROUNDS, SPP = 9, 16
SIZES = ((1920, 1080), (3840, 2160))


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    from tracerboy_amd import api, build
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "still_denoise.json")
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 3
    full, light = api.GetDefaultDenoiserSettings(), api.GetDefaultDenoiserSettings()
    light.WaveletIterations = 0
    ctx, us = [], {size: {"chain": [], "no_filter_pass": []} for size in SIZES}
    try:
        for (w, h) in SIZES:
            tb = api.TracerBoy(0)
            ctx.append(tb)
            tb.SetOption("aov", 1); tb.LoadScene(CORNELL)
            tb.Render(w, h, SPP, s, 0.0)
            tb.Denoise(full, read=False); tb.Denoise(light, read=False)          # warmed: buffers allocated, kernels loaded
        for _ in range(ROUNDS):
            for tb, size in zip(ctx, SIZES):
                tb.Denoise(full, read=False); us[size]["chain"].append(tb.GetOption("last_denoise_us"))
                tb.Denoise(light, read=False); us[size]["no_filter_pass"].append(tb.GetOption("last_denoise_us"))
    finally:
        for tb in ctx:
            tb.close()
    rows = []
    for (w, h) in SIZES:
        c, l = us[(w, h)]["chain"], us[(w, h)]["no_filter_pass"]
        surface = w * h * 16
        rows.append({"width": w, "height": h, "spp": SPP, "iterations": full.WaveletIterations, "surface_bytes": surface,
                     "chain_us": median(c), "chain_us_min": min(c), "chain_us_max": max(c), "chain_us_all": c,
                     "no_filter_pass_us": median(l), "no_filter_pass_us_min": min(l), "no_filter_pass_us_max": max(l), "no_filter_pass_us_all": l,
                     # prepare reads 2 surfaces and writes 1, prefilter and finish read 1 and write 1 each (the prefilter's taps hit the caches)
                     "no_filter_pass_gb_per_s": round(7 * surface / (median(l) * 1e-6) / 1e9, 1),
                     "filter_pass_us_each": round((median(c) - median(l)) / max(1, full.WaveletIterations), 1)})
    result = {"what": "tb_denoise on one MI355X, cornell-box, %d spp, GPU microseconds from HIP events; medians of %d alternating rounds" % (SPP, ROUNDS),
              "kernel_digest": build.kernel_digest(), "sizes": rows}
    with open(out, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
