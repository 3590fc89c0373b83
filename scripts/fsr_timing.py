#!/usr/bin/env python3
"""What FSR 1 upscaling costs on one MI355X.

    python scripts/fsr_timing.py [profiles/fsr_timing.json]

1. The two passes alone: GPU microseconds of EASU and RCAS from HIP events (options last_easu_us / last_rcas_us of tb_upscale), 960 x 540 -> 1920 x 1080
   and 1920 x 1080 -> 3840 x 2160, each surface type in a call of its own.  Beside each pass a device-to-device copy that moves the bytes the pass
   must move, timed with events too: EASU reads the input once and writes the output once, RCAS reads and writes the output size once; a copy of n
   bytes reads n and writes n, so the yardstick for a pass that reads r and writes w bytes is a copy of (r + w) / 2 bytes.  A pass close to its copy
   is bandwidth-bound; a pass several times its copy is bound by its instructions.
2. The figure a user sees: one real-time frame rendered at 960 x 540, post-processed and upscaled to 1920 x 1080 (tb_render_realtime + tb_upscale)
   against one real-time frame rendered at 1920 x 1080 and post-processed (tb_render_realtime + tb_post_process), wall clock around calls that end in a
   device synchronise, the 8-bit picture copied to the host in both.

Everything is warmed first; the variants alternate inside every round, so each figure's samples are spread over the whole run."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
PASS_ROUNDS, FRAME_ROUNDS, FRAMES = 25, 7, 40
PAIRS = (((960, 540), (1920, 1080)), ((1920, 1080), (3840, 2160)))
SURFACES = (("unorm8", 4), ("f32", 16))


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    import torch
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fsr_timing.json")
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 3
    dn, ps = api.GetDefaultDenoiserSettings(), api.GetDefaultPostProcessSettings()
    ctx = {}

    def upscale(tb, ow, oh, surface, host):
        """tb_upscale with one chain only; host: the array the picture is copied into"""
        p = host.ctypes.data_as(C.c_void_p)
        tb._check(tb._L.tb_upscale(tb._ctx, C.byref(ps), 0, ow, oh, -1.0, p if surface == "f32" else None, p if surface == "unorm8" else None))

    def copy_buffers(nbytes):
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        return src, dst

    try:
        for size in ((960, 540), (1920, 1080)):
            tb = api.TracerBoy(0)
            ctx[size] = tb
            tb.LoadScene(CORNELL)
            for _ in range(3):
                tb.RenderRealTime(size[0], size[1], s, dn, 0.0)
        # ---- 1. the passes and their copies -------------------------------------------------------------------------------------------
        host = {(pair, name): np.empty((pair[1][1], pair[1][0], 4), np.uint8 if name == "unorm8" else np.float32) for pair in PAIRS for name, _ in SURFACES}
        copies, rows = {}, {}
        for pair in PAIRS:
            (iw, ih), (ow, oh) = pair
            for name, texel in SURFACES:
                easu_bytes, rcas_bytes = (iw * ih + ow * oh) * texel, 2 * ow * oh * texel
                copies[(pair, name)] = {"easu": copy_buffers(easu_bytes // 2), "rcas": copy_buffers(rcas_bytes // 2)}
                rows[(pair, name)] = {"in": [iw, ih], "out": [ow, oh], "surface": name, "easu_bytes": easu_bytes, "rcas_bytes": rcas_bytes,
                                      "easu_us": [], "rcas_us": [], "easu_copy_us": [], "rcas_copy_us": []}
                upscale(ctx[pair[0]], ow, oh, name, host[(pair, name)])                      # warmed: surfaces allocated, kernels loaded
                for k in ("easu", "rcas"):
                    copies[(pair, name)][k][1].copy_(copies[(pair, name)][k][0])
        torch.cuda.synchronize()
        for _ in range(PASS_ROUNDS):
            for pair in PAIRS:
                for name, _ in SURFACES:
                    tb, row = ctx[pair[0]], rows[(pair, name)]
                    upscale(tb, pair[1][0], pair[1][1], name, host[(pair, name)])
                    row["easu_us"].append(tb.GetOption("last_easu_us")); row["rcas_us"].append(tb.GetOption("last_rcas_us"))
                    for k in ("easu", "rcas"):
                        src, dst = copies[(pair, name)][k]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); dst.copy_(src); e1.record(); e1.synchronize()
                        row[k + "_copy_us"].append(round(e0.elapsed_time(e1) * 1e3, 1))
        passes = []
        for key, row in rows.items():
            for k in ("easu", "rcas"):
                p, c = stats(row[k + "_us"]), stats(row[k + "_copy_us"])
                row[k] = {"us": p, "copy_us": c, "times_the_copy": round(p["median"] / c["median"], 2),
                          "gb_per_s": round(row[k + "_bytes"] / (p["median"] * 1e-6) / 1e9, 1)}
                del row[k + "_us"], row[k + "_copy_us"]
            passes.append(row)
        # ---- 2. a displayed 1080p frame: rendered small and upscaled, against rendered at full size ------------------------------------------
        small, full = ctx[(960, 540)], ctx[(1920, 1080)]
        picture = np.empty((1080, 1920, 4), np.uint8)
        pp = picture.ctypes.data_as(C.c_void_p)

        def frame_upscaled():
            small.RenderRealTime(960, 540, s, dn, 0.0)
            upscale(small, 1920, 1080, "unorm8", picture)

        def frame_full():
            full.RenderRealTime(1920, 1080, s, dn, 0.0)
            full._check(full._L.tb_post_process(full._ctx, C.byref(ps), 0, None, pp))

        for f in (frame_upscaled, frame_full):
            for _ in range(3):
                f()
        ms = {"upscaled": [], "full": []}
        for _ in range(FRAME_ROUNDS):
            for name, f in (("upscaled", frame_upscaled), ("full", frame_full)):
                t0 = time.perf_counter()
                for _ in range(FRAMES):
                    f()
                ms[name].append(round((time.perf_counter() - t0) / FRAMES * 1e3, 3))
        frame = {"what": "milliseconds per displayed 1920 x 1080 frame, wall clock, %d frames per window, %d alternating windows each" % (FRAMES, FRAME_ROUNDS),
                 "render_960x540_post_upscale_ms": stats(ms["upscaled"]), "render_1920x1080_post_ms": stats(ms["full"]),
                 "upscale_us_of_it": small.GetOption("last_upscale_us")}
        frame["full_over_upscaled"] = round(frame["render_1920x1080_post_ms"]["median"] / frame["render_960x540_post_upscale_ms"]["median"], 2)
    finally:
        for tb in ctx.values():
            tb.close()
    result = {"what": "FSR 1 on one MI355X, cornell-box real-time frames, MaxBounces 3; GPU microseconds from HIP events, medians of %d alternating rounds" % PASS_ROUNDS,
              "kernel_digest": build.kernel_digest(), "passes": passes, "frame": frame}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
