#!/usr/bin/env python3
"""What a lightmap bake costs on one MI355X: GPU time of its three parts.

    python scripts/bake_rate.py [profiles/bake_rate.json]

Scenes: cornell-box and tb_load_procedural(0, 870 000).  Each is baked REPEATS times into a 1024 x 1024 atlas with 16 samples and 2 fill passes, from
planar-projection UVs (one grid cell per geometry, as tests/bake_cases.py builds them) that live in a device tensor, into a device tensor.  Recorded per
scene, as the median, the fastest and the slowest of the repeats after one bake that is not counted: the options last_bake_raster_us (tile counts,
scan, coverage, texel records), last_bake_trace_us (the radiance query) and last_bake_finish_us (resolve + fill passes) -- HIP events, microseconds --
the covered texels, and raster + finish as a share of the trace.
The skewed set: one quad over the whole atlas plus 1000 sub-texel triangles, written as a scene file of its own and baked with 1 sample and no bounce,
so that the raster time is what the number is about -- the case in which one triangle's box is the whole atlas and a distribution by triangles would
make it one wave's loop; the same 1000 small triangles WITHOUT the quad beside it, for scale.  No time here is a gate."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE, SAMPLES, DILATE, REPEATS = 1024, 16, 2, 7
SMALL, SKEW_SEED = 1000, 6
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def planar_atlas(positions, ranges, seed=23, margin=0.08):
    """tests/bake_cases.py planar_atlas: geometry g projected along its thinnest axis into cell g of a square grid."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(positions, np.float64).reshape(-1, 3)
    cols = int(np.ceil(np.sqrt(max(len(ranges), 1))))
    uv = np.zeros((len(pos), 2), np.float64)
    for g, (first, count) in enumerate(ranges):
        flip = rng.random() < 0.5
        if not count:
            continue
        p = pos[first:first + count]
        ext = p.max(0) - p.min(0)
        axes = np.argsort(-ext, kind="stable")[:2]
        if flip:
            axes = axes[::-1]
        q = (p[:, axes] - p.min(0)[axes]) / np.maximum(ext[axes], 1e-30)
        uv[first:first + count] = (np.array([g % cols, g // cols], np.float64) + margin + q * (1 - 2 * margin)) / cols
    return uv.astype(np.float32)


def skewed_scene(path, with_quad):
    """A scene file of SMALL sub-texel triangles (for a SIDE x SIDE atlas) and, with_quad, two triangles over the whole atlas after them."""
    rng = np.random.default_rng(SKEW_SEED)
    c = rng.uniform(0, 1, (SMALL, 1, 2)) * SIDE
    uv = (c + rng.uniform(-0.3, 0.3, (SMALL, 3, 2))) / SIDE
    if with_quad:
        uv = np.concatenate([uv, [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]]])
    uv = uv.reshape(-1, 2)
    pos = np.stack([uv[:, 0] * 2 - 1, uv[:, 1] * 2, np.zeros(len(uv))], 1)
    fmt = lambda a: " ".join("%.9g" % x for x in np.asarray(a).reshape(-1))
    with open(path, "w") as f:
        f.write('LookAt 0 1 4  0 1 0  0 1 0\nCamera "perspective" "float fov" [45]\nFilm "image" "integer xresolution" [32] "integer yresolution" [24]\nWorldBegin\n'
                'MakeNamedMaterial "A" "string type" ["matte"] "rgb Kd" [0.7 0.6 0.5]\nNamedMaterial "A"\n')
        f.write('Shape "trianglemesh" "integer indices" [%s] "point P" [%s] "float uv" [%s]\nWorldEnd\n' % (" ".join(str(i) for i in range(len(uv))), fmt(pos), fmt(uv)))


def timed_bakes(tb, settings, samples, dilate, uv, out):
    rows = {"raster_us": [], "trace_us": [], "finish_us": []}
    for i in range(REPEATS + 1):
        tb.BakeLightmap(SIDE, SIDE, samples, uv=uv, dilate=dilate, settings=settings, out=out)
        if i:
            for k in rows:
                rows[k].append(tb.GetOption("last_bake_" + k))
    r = {k: stats(v) for k, v in rows.items()}
    r["covered"] = tb.GetOption("last_bake_covered")
    return r


def main():
    import torch
    from tracerboy_amd import api, build
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bake_rate.json")
    if not torch.cuda.is_available():
        raise SystemExit("bake_rate.py measures on the GPU: no device found")
    settings = api.GetDefaultOutputSettings()
    result = {"device": torch.cuda.get_device_name(0), "kernel_digest": build.kernel_digest(), "atlas": [SIDE, SIDE], "samples": SAMPLES, "dilate": DILATE,
              "repeats": REPEATS, "unit": "microseconds of GPU time (HIP events)", "scenes": {}, "skewed": {}}
    out = torch.empty((SIDE, SIDE, 4), dtype=torch.float32, device="cuda:0")
    with api.TracerBoy(0) as tb:
        for name in ("cornell-box", "proc0:870000"):
            if name == "cornell-box":
                tb.LoadScene(CORNELL); hs = api.HostScene(CORNELL)
            else:
                tb.LoadProcedural(0, 870000, 1234); hs = api.HostScene(procedural=(0, 870000, 1234))
            view = tb.HostSceneView()
            ranges = [tb.GeometryVertexRange(g) for g in range(view.numHitGroups)]
            uv = torch.from_numpy(planar_atlas(hs.triangles()["positions"], ranges)).to("cuda:0")
            hs.close()
            r = timed_bakes(tb, settings, SAMPLES, DILATE, uv, out)
            r["triangles"] = tb.SceneInfo().numTriangles
            r["raster_plus_finish_share_of_trace"] = (r["raster_us"]["median"] + r["finish_us"]["median"]) / max(r["trace_us"]["median"], 1)
            result["scenes"][name] = r
            print(name, json.dumps(r), flush=True)
        dark = api.GetDefaultOutputSettings(); dark.MaxBounces = 0
        with tempfile.TemporaryDirectory() as tmp:
            for name, with_quad in (("quad_and_1000_small", True), ("1000_small_alone", False)):
                path = os.path.join(tmp, name + ".pbrt")
                skewed_scene(path, with_quad)
                tb.LoadScene(path)
                r = timed_bakes(tb, dark, 1, 0, None, out)
                r["triangles"] = tb.SceneInfo().numTriangles
                result["skewed"][name] = r
                print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
