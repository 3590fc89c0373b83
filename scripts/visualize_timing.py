#!/usr/bin/env python3
"""What the path inspector costs on one MI355X.

    python scripts/visualize_timing.py LABEL [profiles/visualize_rays.json]

1. The overlay (tb_visualize_rays, option last_visualize_us: HIP events around vis_overlay) on a 1920 x 1080 cornell-box frame with the buffer full
   -- 4096 frames of the centre pixel recorded, 1024 rays stored -- drawn with RayCount 64 and with all 1024; beside them tb_post_process of the same
   frame, HIP events on the context's stream around the call, for scale.
2. The recorder (tb_record_paths, option last_paths_us: both runs of pt_paths and the scan between them) for 64 and for 4096 frames of the centre
   pixel, on cornell-box and on Teapot.

Everything runs once first; then 9 rounds in which the shapes alternate, so each figure's samples are spread over the whole run: median, min, max.
The figures go into the JSON file under "forms"[LABEL], beside those of other labels: the ray loop of vis_overlay has two forms, chosen when the
library is compiled (vis_kernels.hip TB_VIS_RAYS_IN_LDS), and each is measured by a process of its own --

    python scripts/build_variant.py vislds --flags=-DTB_VIS_RAYS_IN_LDS=1 --tus kernels/vis_kernels.hip
    python scripts/visualize_timing.py scalar
    TB_LIB=$PWD/tracerboy_amd/_sweep/libtracerboy_hip_vislds.so python scripts/visualize_timing.py lds
and once more as scalar_2 / lds_2, so that the two forms alternate."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = {name: os.path.join(ROOT, "tests", "golden", "scenes", name, "scene.pbrt") for name in ("cornell-box", "Teapot")}
ROUNDS, W, H = 9, 1920, 1080


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    import torch
    from tracerboy_amd import api, build
    label = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "visualize_rays.json")
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 4
    ctx = {}
    try:
        for name, path in SCENES.items():
            tb = api.TracerBoy(0)
            ctx[name] = tb
            tb.LoadScene(path)
            tb.Render(W, H, 1, s, 0.0)
        box = ctx["cornell-box"]
        stream = torch.cuda.ExternalStream(box.Stream())
        few, every = api.GetDefaultVisualizeSettings(), api.GetDefaultVisualizeSettings()
        few.RayCount = 64
        _, total = box.RecordPaths(W // 2, H // 2, 0, 4096)
        stored = len(box.ReadPaths())
        assert stored == 1024 < total

        def post():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            box._check(box._L.tb_post_process(box._ctx, None, 0, None, None))
            e1.record(stream); e1.synchronize()
            return round(e0.elapsed_time(e1) * 1e3, 1)

        def overlay(settings):
            box._check(box._L.tb_visualize_rays(box._ctx, settings, None, None))
            return box.GetOption("last_visualize_us")

        def record(name, n):
            ctx[name].ClearPaths()
            ctx[name].RecordPaths(W // 2, H // 2, 0, n)
            return ctx[name].GetOption("last_paths_us")

        import ctypes as C
        shapes = {"post_process_us": post, "overlay_64_rays_us": lambda: overlay(C.byref(few)), "overlay_1024_rays_us": lambda: overlay(C.byref(every))}
        for name in SCENES:
            for n in (64, 4096):
                shapes["record_%s_%d_frames_us" % (name, n)] = (lambda name=name, n=n: record(name, n))
        # the overlay reads the buffer as the 4096-frame call left it: the recorder's shapes run on the other context, or refill it
        samples = {k: [] for k in shapes}
        for rnd in range(ROUNDS + 1):                                # round 0 warms: surfaces allocated, kernels loaded
            for k, f in shapes.items():
                if k.startswith("record_cornell-box"):
                    continue
                v = f()
                if rnd:
                    samples[k].append(v)
        for rnd in range(ROUNDS + 1):
            for k, f in shapes.items():
                if k.startswith("record_cornell-box"):
                    v = f()
                    if rnd:
                        samples[k].append(v)
        figures = {k: stats(v) for k, v in samples.items()}
    finally:
        for tb in ctx.values():
            tb.close()
    result = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            result = json.load(f)
    result["what"] = ("the path inspector on one MI355X: GPU microseconds from HIP events, everything run once first, then median / min / max of %d rounds "
                      "in which the shapes alternate; %d x %d, MaxBounces 4, the centre pixel; one process per form of vis_overlay's ray loop" % (ROUNDS, W, H))
    result.setdefault("forms", {})[label] = {"kernel_digest": build.kernel_digest(), "library": os.path.basename(api.LIB_PATH), "rays_stored": stored,
                                             "rays_total_of_4096_frames": total, **figures}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result["forms"][label]))


if __name__ == "__main__":
    main()
