"""What the guide pass of a denoised still costs on one MI355X, against what it replaces: a render with option "aov" on.
cornell-box and Teapot at 1920 x 1080, MaxBounces 3, blue noise off:

    last_guides_us of tb_render_guides over the last K = 1, 8, 32 of 64 frames   (HIP events around the kernel)
    tb_last_render_ms of the 64 frames with option "aov" off                      (the render the guide pass goes with)
    tb_last_render_ms of the same 64 frames with option "aov" on                  (what section 12 needs for the same picture)

    python scripts/still_guides_timing.py [profiles/still_guides.json]

Two contexts per scene (option "aov" resets the history), everything called once before anything is timed; then ROUNDS rounds that alternate
between the scenes and, inside a round, between the five measurements, so that every figure has ROUNDS samples spread over the whole run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = {name: os.path.join(ROOT, "tests", "golden", "scenes", name, "scene.pbrt") for name in ("cornell-box", "Teapot")}
ROUNDS, FRAMES, W, H = 9, 64, 1920, 1080
KS = (1, 8, 32)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    from tracerboy_amd import api, build
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "still_guides.json")
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 3
    ctx, t = {}, {name: {"render_aov_off_ms": [], "render_aov_on_ms": [], **{"guides_us_k%d" % k: [] for k in KS}} for name in SCENES}

    def render(tb):
        tb.InvalidateHistory()
        tb.Render(W, H, FRAMES, s, 0.0)
        return tb.LastRenderMs()

    try:
        for name, path in SCENES.items():
            plain, aov = api.TracerBoy(0), api.TracerBoy(0)
            ctx[name] = (plain, aov)
            aov.SetOption("aov", 1)
            for tb in (plain, aov):
                tb.LoadScene(path)
                render(tb); render(tb)                           # warmed: buffers allocated, kernels loaded, the launch trials past their first calls
            for k in KS:
                plain.RenderGuides(FRAMES - k, k)
        for _ in range(ROUNDS):
            for name, (plain, aov) in ctx.items():
                t[name]["render_aov_off_ms"].append(render(plain))
                t[name]["render_aov_on_ms"].append(render(aov))
                for k in KS:
                    plain.RenderGuides(FRAMES - k, k)
                    t[name]["guides_us_k%d" % k].append(plain.GetOption("last_guides_us"))
        variants = {name: (plain.GetOption("last_variant"), aov.GetOption("last_variant")) for name, (plain, aov) in ctx.items()}
    finally:
        for pair in ctx.values():
            for tb in pair:
                tb.close()
    rows = []
    for name in SCENES:
        v = t[name]
        off, on = median(v["render_aov_off_ms"]), median(v["render_aov_on_ms"])
        row = {"scene": name, "width": W, "height": H, "frames": FRAMES, "variant_aov_off": variants[name][0], "variant_aov_on": variants[name][1],
               "render_aov_off_ms": round(off, 3), "render_aov_on_ms": round(on, 3), "aov_surplus_ms": round(on - off, 3),
               "aov_surplus_ms_per_frame": round((on - off) / FRAMES, 4)}
        for k in KS:
            g = v["guides_us_k%d" % k]
            row["guides_k%d" % k] = {"us": median(g), "us_min": min(g), "us_max": max(g), "us_per_frame": round(median(g) / k, 1),
                                     "plain_render_plus_guides_ms": round(off + median(g) / 1e3, 3),
                                     "cheaper_than_aov_render": bool(off + median(g) / 1e3 < on)}
        row["all"] = {key: [round(x, 3) for x in val] for key, val in v.items()}
        rows.append(row)
    result = {"what": "tb_render_guides on one MI355X against a render with option aov on: %d x %d, %d frames, MaxBounces 3; GPU time from HIP events; "
                      "medians of %d alternating rounds" % (W, H, FRAMES, ROUNDS), "kernel_digest": build.kernel_digest(), "scenes": rows}
    with open(out, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
