#!/usr/bin/env python3
"""What ray queries deliver on one MI355X: Mrays/s of tb_trace_rays by mode and form.

    python scripts/ray_query_rate.py [profiles/ray_query_rate.json [SCENE ...]]

Scenes: cornell-box and tb_load_procedural(0, 870 000) -- or those named: cornell-box, procK:N = tb_load_procedural(K, N) (the sweep over scene
sizes behind RQ_REFILL_TRIANGLES: profiles/ray_query_sizes.json proc0:2000 proc0:10000 proc0:50000 proc0:200000).  Ray sets, 2^22 rays each, made on the device with torch from seeds:
  camera    the camera rays of a 1920 x 1080 frame in pixel order, jittered, as many frames as fill the set
  ao        from their hits, cosine-distributed about the hit normal, TMax = a quarter of the scene's diagonal (a miss leaves a disabled ray)
  ao_shuf   the same AO rays in a seeded random order
Forms, every one the synchronous call from Python with a host clock around it:
  a  closest      closest mode, device path
  b  hook_host    the parent's TraceClosest on the same rays, end to end on host arrays -- all that the parent commit can be measured on
  c  occluded     occluded mode as it ships: the any-hit walk, one ray per lane below RQ_REFILL_TRIANGLES triangles, refilling from there
  d  from_closest occluded mode answered by the closest-hit walk and t < TMax (diagnostic TB_RQ_REFILL=-1): what the any-hit walk has to beat
  e  one_shot     the any-hit walk without refill, one ray per lane: a wave takes 64 rays and leaves when all are done (TB_RQ_REFILL=0)
     refill_16 / refill_32 / refill_64: the refilling any-hit walk at that many idle lanes per refill (64: a wave refills when all its rays are done)
Everything runs once first.  Then ROUNDS rounds in which the forms alternate; in a round a form repeats its call for at least WINDOW seconds and
the window's rate is rays / time.  Reported per form: the median window, the slowest and the fastest."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, W, H = 1 << 22, 1920, 1080
ROUNDS, WINDOW = 7, 0.2
DEVICE_FORMS = {"closest": None, "occluded": "", "from_closest": "-1", "one_shot": "0", "refill_64": "64", "refill_16": "16", "refill_32": "32"}


def camera_rays(torch, cam, seed):
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    f32 = dict(dtype=torch.float32, device="cuda:0")
    i = torch.arange(N, device="cuda:0")
    pix = i % (W * H)
    x, y = (pix % W).to(torch.float32), (pix // W).to(torch.float32)
    jitter = torch.rand((N, 2), generator=g, **f32)
    u, v = (x + jitter[:, 0]) / W, 1.0 - (y + jitter[:, 1]) / H
    pos, look, right, up = (torch.tensor(list(a), **f32) for a in (cam.Position, cam.LookAt, cam.Right, cam.Up))
    forward = (look - pos) / torch.linalg.norm(look - pos)
    focal = pos - cam.FocalDistance * forward
    lens_w = cam.LensHeight * W / H
    lens = pos + right * ((u * 2 - 1) * lens_w / 2)[:, None] + up * ((v * 2 - 1) * cam.LensHeight / 2)[:, None]
    d = lens - focal
    rays = torch.empty((N, 8), **f32)
    rays[:, 0:3] = focal; rays[:, 3] = math.inf
    rays[:, 4:7] = d / torch.linalg.norm(d, dim=1, keepdim=True); rays[:, 7] = 0.0
    return rays


def ao_rays(torch, rays, hits, diagonal, seed):
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    o, d, t, n = rays[:, 0:3], rays[:, 4:7], hits[:, 0], hits[:, 8:11]
    n = torch.where(((n * d).sum(1) > 0)[:, None], -n, n)          # towards the ray's side
    n = n / torch.linalg.norm(n, dim=1, keepdim=True).clamp_min(1e-20)
    r = torch.rand((N, 2), generator=g, dtype=torch.float32, device="cuda:0")
    phi, s = 2 * math.pi * r[:, 0], torch.sqrt(r[:, 1])
    helper = torch.where((n[:, 0].abs() > 0.9)[:, None], torch.tensor([0.0, 1.0, 0.0], device="cuda:0"), torch.tensor([1.0, 0.0, 0.0], device="cuda:0"))
    tx = torch.linalg.cross(n, helper); tx = tx / torch.linalg.norm(tx, dim=1, keepdim=True).clamp_min(1e-20)
    ty = torch.linalg.cross(n, tx)
    w = tx * (s * torch.cos(phi))[:, None] + ty * (s * torch.sin(phi))[:, None] + n * torch.sqrt(1 - r[:, 1])[:, None]
    out = torch.empty_like(rays)
    out[:, 0:3] = o + d * t[:, None] + n * (1e-4 * diagonal); out[:, 3] = 0.25 * diagonal
    out[:, 4:7] = w / torch.linalg.norm(w, dim=1, keepdim=True).clamp_min(1e-20)
    out.view(torch.int32)[:, 7] = (t < 0).to(torch.int32)          # TB_QUERY_RAY_DISABLED where the camera ray hit nothing
    return out


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def main():
    import torch
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ray_query_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_rate.py measures on the GPU: no device found")
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "rays": N, "rounds": ROUNDS, "window_s": WINDOW,
              "unit": "Mrays/s", "scenes": {}}
    for scene in sys.argv[2:] or ["cornell-box", "proc0:870000"]:
        with api.TracerBoy(0) as tb:
            if scene == "cornell-box":
                tb.LoadScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt"))
            else:
                kind, triangles = scene[4:].split(":")
                tb.LoadProcedural(int(kind), int(triangles), 1234)
            info = tb.SceneInfo()
            diagonal = math.dist(info.sceneMin[:], info.sceneMax[:])
            cam = camera_rays(torch, tb.GetCamera(), 1)
            ao = ao_rays(torch, cam, tb.TraceRays(cam, api.RAYS_CLOSEST), diagonal, 2)
            g = torch.Generator(device="cuda:0"); g.manual_seed(3)
            sets = {"camera": cam, "ao": ao, "ao_shuf": ao[torch.randperm(N, generator=g, device="cuda:0")].contiguous()}
            result["scenes"][scene] = {"triangles": info.numTriangles, "bvh_max_depth": info.bvhMaxDepth, "sets": {}}
            for name, rays in sets.items():
                host = rays.cpu().numpy()
                ho, hd = host[:, 0:3].copy(), host[:, 4:7].copy()

                def call(form):
                    if form == "hook_host":
                        return tb.TraceClosest(ho, hd)
                    if DEVICE_FORMS[form] is None:
                        return tb.TraceRays(rays, api.RAYS_CLOSEST)
                    os.environ["TB_RQ_REFILL"] = DEVICE_FORMS[form]
                    try:
                        return tb.TraceRays(rays, api.RAYS_OCCLUDED)
                    finally:
                        os.environ["TB_RQ_REFILL"] = ""

                forms = list(DEVICE_FORMS) + ["hook_host"]
                answers = {f: call(f) for f in forms}               # everything once; and the forms of occluded mode agree
                traced = (rays.view(torch.int32)[:, 7] & 1) == 0
                occluded_share = float(answers["occluded"][traced].float().mean()) if bool(traced.any()) else 0.0
                differ = {f: int((answers[f] != answers["occluded"]).sum()) for f in DEVICE_FORMS if f not in ("closest", "occluded")}
                windows = {f: [] for f in forms}
                for _ in range(ROUNDS):
                    for f in forms:
                        calls, t0 = 0, time.perf_counter()
                        while True:
                            call(f); calls += 1
                            dt = time.perf_counter() - t0
                            if dt >= WINDOW:
                                break
                        windows[f].append(calls * N / dt / 1e6)
                row = {"occluded_share_of_traced": occluded_share, "differ_from_occluded": differ, "forms": {f: stats(v) for f, v in windows.items()}}
                result["scenes"][scene]["sets"][name] = row
                print(scene, name, "occluded %.3f" % occluded_share, "differ", differ, flush=True)
                for f in forms:
                    s = row["forms"][f]
                    print("    %-13s %9.1f  [%9.1f .. %9.1f] Mrays/s" % (f, s["median"], s["min"], s["max"]), flush=True)
                del answers
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
