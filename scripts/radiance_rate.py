#!/usr/bin/env python3
"""What radiance queries deliver on one MI355X: Mpaths/s of tb_trace_radiance by ray set and form.

    python scripts/radiance_rate.py [profiles/radiance_rate.json [SCENE ...]]

Scenes: cornell-box and tb_load_procedural(0, 870 000) -- or those named: cornell-box, procK:N.  Ray sets, on device tensors:
  cam1       the camera rays of a 1920 x 1080 frame from tb_make_camera_rays (frame 0), 1 sample
  cam16      the same rays, 16 samples
  hemi       hemisphere mode about the normals of those rays' first hits (tb_trace_rays), in pixel order, HEMI_SAMPLES samples; a camera ray that hit
             nothing leaves a zero normal, which is not traced and not counted
  hemi_shuf  the same hits in a seeded random order
Forms, every one the synchronous call from Python with a host clock around it (the diagnostics of context_radiance.cpp):
  plain          one ray per lane: a wave takes 64 rays and leaves when all are done        TB_RAD_FORM=0
  refill         the refilling persistent grid, pools of RAD_CHUNK rays                     TB_RAD_FORM=1
  refill_half    ... of half that                                                           TB_RAD_FORM=1 TB_RAD_CHUNK=32
  refill_double  ... of twice that                                                          TB_RAD_FORM=1 TB_RAD_CHUNK=128
Beside them, for scale only: tb_render of the same frame count (1 and 16 frames of 1920 x 1080 from frame 0) on the same context in Msamples/s --
what the renderer offers for camera rays, with its scenes in LDS and its tuned kernels -- and the ratio query / render; it is no gate.
Everything runs once first, and the forms' answers are compared.  Then ROUNDS rounds in which the forms alternate; in a round a form repeats its
call for at least WINDOW seconds and the window's rate is paths / time.  Reported per form: the median window, the slowest and the fastest."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
ROUNDS, WINDOW = 7, 0.2
HEMI_SAMPLES = 4
CHUNK = 64  # RAD_CHUNK (kernels/rad_launch.h)
FORMS = {"plain": {"TB_RAD_FORM": "0"}, "refill": {"TB_RAD_FORM": "1"}, "refill_half": {"TB_RAD_FORM": "1", "TB_RAD_CHUNK": str(CHUNK // 2)},
         "refill_double": {"TB_RAD_FORM": "1", "TB_RAD_CHUNK": str(CHUNK * 2)}}
KNOBS = ("TB_RAD_FORM", "TB_RAD_CHUNK")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def window(call, units):
    calls, t0 = 0, time.perf_counter()
    while True:
        call(); calls += 1
        dt = time.perf_counter() - t0
        if dt >= WINDOW:
            return calls * units / dt / 1e6


def main():
    import torch
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "radiance_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("radiance_rate.py measures on the GPU: no device found")
    settings = api.GetDefaultOutputSettings()
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "frame": [W, H], "rounds": ROUNDS, "window_s": WINDOW,
              "hemi_samples": HEMI_SAMPLES, "chunk": CHUNK, "unit": "Mpaths/s (render: Msamples/s)", "scenes": {}}
    for scene in sys.argv[2:] or ["cornell-box", "proc0:870000"]:
        with api.TracerBoy(0) as tb:
            if scene == "cornell-box":
                tb.LoadScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt"))
            else:
                kind, triangles = scene[4:].split(":")
                tb.LoadProcedural(int(kind), int(triangles), 1234)
            info = tb.SceneInfo()
            cam, advance = tb.MakeCameraRays(W, H, 0, settings=settings, device=True)
            n = int(cam.shape[0])
            query = cam.clone(); query[:, 3] = float("inf"); query.view(torch.int32)[:, 7] = 0
            hits = tb.TraceRays(query, api.RAYS_CLOSEST)
            t, nrm = hits[:, 0], hits[:, 8:11]
            nrm = torch.where(((nrm * cam[:, 4:7]).sum(1) > 0)[:, None], -nrm, nrm)
            nrm = torch.where((t > 0)[:, None], nrm / torch.linalg.norm(nrm, dim=1, keepdim=True).clamp_min(1e-20), torch.zeros_like(nrm))
            hemi = cam.clone()
            hemi[:, 0:3] = cam[:, 0:3] + cam[:, 4:7] * t.clamp_min(0)[:, None]; hemi[:, 4:7] = nrm
            g = torch.Generator(device="cuda:0"); g.manual_seed(3)
            hit_count = int((t > 0).sum())
            sets = {"cam1": (cam, 1, api.RADIANCE_RAY, n), "cam16": (cam, 16, api.RADIANCE_RAY, n * 16),
                    "hemi": (hemi, HEMI_SAMPLES, api.RADIANCE_HEMISPHERE, hit_count * HEMI_SAMPLES),
                    "hemi_shuf": (hemi[torch.randperm(n, generator=g, device="cuda:0")].contiguous(), HEMI_SAMPLES, api.RADIANCE_HEMISPHERE, hit_count * HEMI_SAMPLES)}
            result["scenes"][scene] = {"triangles": info.numTriangles, "bvh_max_depth": info.bvhMaxDepth, "rays": n, "first_hits": hit_count, "sets": {}, "render": {}}
            for frames in (1, 16):                                  # for scale: the renderer on the same frame count
                def render():
                    tb.InvalidateHistory(); tb.Render(W, H, frames, settings, 0.0)
                render()
                result["scenes"][scene]["render"][str(frames)] = stats([window(render, n * frames) for _ in range(ROUNDS)])
                print(scene, "tb_render x%d %9.1f Msamples/s" % (frames, result["scenes"][scene]["render"][str(frames)]["median"]), flush=True)
            for name, (rays, samples, mode, paths) in sets.items():
                def call(form):
                    for k in KNOBS:
                        os.environ[k] = FORMS[form].get(k, "")
                    try:
                        return tb.TraceRadiance(rays, samples, 0, advance, mode=mode, settings=settings)
                    finally:
                        for k in KNOBS:
                            os.environ[k] = ""

                answers, ran = {}, {}
                for f in FORMS:                                     # everything once; and the forms agree
                    answers[f] = call(f); ran[f] = (tb.GetOption("last_radiance_form"), tb.GetOption("last_radiance_variant"))
                differ = {f: int((answers[f].view(torch.int32) != answers["plain"].view(torch.int32)).any(1).sum()) for f in FORMS}
                windows = {f: [] for f in FORMS}
                for _ in range(ROUNDS):
                    for f in FORMS:
                        windows[f].append(window(lambda: call(f), paths))
                row = {"samples": samples, "paths": paths, "ran_form_variant": ran, "rays_that_differ_from_plain": differ, "forms": {f: stats(v) for f, v in windows.items()}}
                if name in ("cam1", "cam16"):
                    r = result["scenes"][scene]["render"][str(samples)]["median"]
                    row["share_of_render"] = {f: row["forms"][f]["median"] / r for f in FORMS}
                result["scenes"][scene]["sets"][name] = row
                print(scene, name, "differ", differ, flush=True)
                for f in FORMS:
                    s = row["forms"][f]
                    print("    %-13s %9.1f  [%9.1f .. %9.1f] Mpaths/s" % (f, s["median"], s["min"], s["max"]), flush=True)
                del answers
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
