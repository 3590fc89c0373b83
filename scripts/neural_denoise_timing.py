#!/usr/bin/env python3
"""What the neural still denoiser costs on one MI355X.

    python scripts/neural_denoise_timing.py [profiles/neural_timing.json [weights.tza]]

GPU microseconds of one network at 1920 x 1080 with 9-input weights, pack to unpack, from HIP events (option last_neural_us of tb_run_neural): 3
warm-up calls, then the median of 10.  Beside it the FLOPs of the 16 convolutions on the picture extended to 1920 x 1088, counted from the layer
shapes (2 x 9 x inputs x outputs per pixel of the layer's level), and the share of the fp16 MFMA peak that time comes to.

Without a weights file the script takes OIDN's rt_ldr_alb_nrm.tza from tests/golden/oidn/ (tests/neural_ref.py joins its two parts)."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, WARMUP, CALLS = 1920, 1080, 3, 10
PEAK_FP16_MFMA = 2.5e15   # dense fp16 / bf16 MFMA FLOP/s of one MI355X
LEVEL = (0, 0, 1, 2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0)   # the level a layer writes at: 0 = the picture, 4 = a sixteenth of it each way


def main():
    import neural_ref as nr
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "neural_timing.json")
    with tempfile.TemporaryDirectory() as tmp:
        path = sys.argv[2] if len(sys.argv) > 2 else nr.real_weights_file(tmp)
        info = api.NeuralWeightsInfo(path)
        pw, ph = -(-W // 16) * 16, -(-H // 16) * 16
        flop = sum(2 * 9 * i * o * (pw >> l) * (ph >> l) for i, o, l in zip(info.in_channels_of, info.out_channels, LEVEL))
        rng = np.random.default_rng(1)
        planes = [np.concatenate([rng.random((H, W, 3), np.float32), np.ones((H, W, 1), np.float32)], -1) for _ in range(3)]
        with api.TracerBoy(0) as tb:
            tb.LoadNeuralWeights(path)
            us = []
            for k in range(WARMUP + CALLS):
                tb.RunNeural(*planes)
                if k >= WARMUP:
                    us.append(tb.GetOption("last_neural_us"))
    s = sorted(us)
    median = s[len(s) // 2]
    result = {"what": "the neural still denoiser on one MI355X: one network at %d x %d (run at %d x %d), 9 inputs, pack to unpack; GPU microseconds from HIP "
                      "events, %d warm-up calls, %d measured" % (W, H, pw, ph, WARMUP, CALLS),
              "kernel_digest": build.kernel_digest(), "in_channels": info.in_channels, "out_channels": list(info.out_channels),
              "last_neural_us": {"median": median, "min": s[0], "max": s[-1], "n": len(s)},
              "flop": flop, "tflop_per_s": round(flop / (median * 1e-6) / 1e12, 1),
              "fp16_mfma_peak_flop_per_s": PEAK_FP16_MFMA, "share_of_fp16_mfma_peak": round(flop / (median * 1e-6) / PEAK_FP16_MFMA, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
