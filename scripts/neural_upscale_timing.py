#!/usr/bin/env python3
"""What the neural 2 x super-resolution costs on one MI355X.

    python scripts/neural_upscale_timing.py [profiles/neural_upscale_timing.json [weights.bin]]
    python scripts/neural_upscale_timing.py --run FORM WxH [weights.bin]       # under a kernel trace, in a run of its own
    python scripts/neural_upscale_timing.py --split kernel_trace.csv [out.json]

The first form: GPU microseconds of one network, pack to finish, from HIP events (option last_sr_us of tb_run_sr) at 960 x 540 -> 1920 x 1080 and
1920 x 1080 -> 3840 x 2160, in both forms of the convolutions (option sr_conv_form): 3 warm-up calls, then the median and min-max of 10.  Beside
them the useful FLOP/s, from the layer shapes: 2 x K x K x inputs x outputs per pixel of the layer's size, 169 840 FLOP per output pixel with the
reference's weights.  The verdict follows the rule of section 16: the staged form is the default only where its median is below the plain form's
at both sizes by more than the plain form's min-max spread.

--run: 3 + 5 networks and nothing else, for `rocprofv3 --kernel-trace -- python scripts/neural_upscale_timing.py --run ...`; --split reads that
trace's kernel_trace.csv: the dispatches come as pack, seven convolutions, finish; the last 5 networks give the median per layer.

Without a weights file the script takes the reference's from tests/golden/dml_sr/."""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, CALLS = 3, 10
SIZES = ((960, 540), (1920, 1080))
PEAK_FP16_MFMA = 2.5e15   # dense fp16 / bf16 MFMA FLOP/s of one MI355X
REAL_WEIGHTS = os.path.join(ROOT, "tests", "golden", "dml_sr", "weights.bin")
STEPS = ("pack", "conv1", "conv2", "conv3", "conv_up1", "conv4", "conv5", "conv6", "finish")


def flop_per_output_pixel(info):
    """layers 0-2 run at a quarter of the output's pixels"""
    return sum(2 * k * k * i * o * (0.25 if l < 3 else 1.0) for l, (i, o, k) in enumerate(zip(info.in_channels, info.out_channels, info.kernel)))


def picture(w, h):
    rng = np.random.default_rng(1)
    return np.concatenate([rng.random((h, w, 3), np.float32), np.ones((h, w, 1), np.float32)], -1)


def measure(tb, w, h, form, calls=CALLS):
    tb.SetOption("sr_conv_form", form)
    color, us = picture(w, h), []
    for k in range(WARMUP + calls):
        tb.RunUpscaleNeural(color)
        if k >= WARMUP:
            us.append(tb.GetOption("last_sr_us"))
    s = sorted(us)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def split(trace, out_path):
    rows = [r for r in csv.DictReader(open(trace)) if any(n in r["Kernel_Name"] for n in ("nn_pack_input", "nn_convk", "nn_sr_finish"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) % len(STEPS) == 0 and len(rows) >= 5 * len(STEPS), "%d dispatches: not whole networks of %d" % (len(rows), len(STEPS))
    nets = [rows[i:i + len(STEPS)] for i in range(0, len(rows), len(STEPS))][-5:]
    us = {step: sorted((int(n[i]["End_Timestamp"]) - int(n[i]["Start_Timestamp"])) / 1e3 for n in nets)[2] for i, step in enumerate(STEPS)}
    result = {"what": "per-layer GPU microseconds of one network from a kernel trace: the median of the last 5 networks", "us": us,
              "sum_us": round(sum(us.values()), 1), "kernels": [nets[-1][i]["Kernel_Name"][:60] for i in range(len(STEPS))]}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--split":
        return split(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    from tracerboy_amd import api, build
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        form, (w, h) = int(sys.argv[2]), (int(v) for v in sys.argv[3].split("x"))
        with api.TracerBoy(0) as tb:
            tb.LoadUpscaleWeights(sys.argv[4] if len(sys.argv) > 4 else REAL_WEIGHTS)
            measure(tb, w, h, form, calls=5)
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "neural_upscale_timing.json")
    path = sys.argv[2] if len(sys.argv) > 2 else REAL_WEIGHTS
    info = api.SrWeightsInfo(path)
    per_pixel = flop_per_output_pixel(info)
    sizes = []
    with api.TracerBoy(0) as tb:
        tb.LoadUpscaleWeights(path)
        default_form = tb.GetOption("sr_conv_form")
        for w, h in SIZES:
            flop = per_pixel * 4 * w * h
            row = {"input": [w, h], "output": [2 * w, 2 * h], "flop": flop}
            for form, name in ((0, "plain"), (1, "staged")):
                t = measure(tb, w, h, form)
                t["tflop_per_s"] = round(flop / (t["median"] * 1e-6) / 1e12, 1)
                t["share_of_fp16_mfma_peak"] = round(flop / (t["median"] * 1e-6) / PEAK_FP16_MFMA, 4)
                row[name] = t
            row["staged_clears_the_rule"] = row["plain"]["median"] - row["staged"]["median"] > row["plain"]["max"] - row["plain"]["min"]
            sizes.append(row)
    result = {"what": "the neural 2 x super-resolution on one MI355X: one network, pack to finish, in both forms of its convolutions; GPU microseconds "
                      "from HIP events (last_sr_us), %d warm-up calls, %d measured" % (WARMUP, CALLS),
              "kernel_digest": build.kernel_digest(), "in_channels": list(info.in_channels), "out_channels": list(info.out_channels),
              "kernel": list(info.kernel), "flop_per_output_pixel": per_pixel, "fp16_mfma_peak_flop_per_s": PEAK_FP16_MFMA, "sizes": sizes,
              "staged_is_the_default": all(r["staged_clears_the_rule"] for r in sizes), "default_form_of_this_build": default_form}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
