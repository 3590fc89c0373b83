"""Is the guide kernel better off held to three waves per SIMD with 4-5 registers in scratch, as built, or left at the two
waves the compiler gives it?  Same-box A/B of two libraries:

    python scripts/build_variant.py guides2 --flags=-DTB_GUIDES_WAVES=0 --tus kernels/guide_kernels.hip
    python scripts/still_guides_waves_ab.py [profiles/still_guides_waves_ab.json]

ROUNDS rounds alternate between the libraries; every measurement is a fresh child process (TB_LIB selects the library) that loads cornell-box and
Teapot, sets the 1920 x 1080 frame, warms the pass and reports the median last_guides_us of three K = 8 passes per scene."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = {name: os.path.join(ROOT, "tests", "golden", "scenes", name, "scene.pbrt") for name in ("cornell-box", "Teapot")}
LIBS = {"waves3_built": os.path.join(ROOT, "tracerboy_amd", "libtracerboy_hip.so"),
        "waves2_unheld": os.path.join(ROOT, "tracerboy_amd", "_sweep", "libtracerboy_hip_guides2.so")}
ROUNDS, W, H, K = 5, 1920, 1080, 8


def median(v):
    return sorted(v)[len(v) // 2]


def child():
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 3
    res = {}
    for name, path in SCENES.items():
        with api.TracerBoy(0) as tb:
            tb.LoadScene(path)
            tb.BeginAccumulation(W, H, s, 0.0, first_frame=0)
            tb.RenderGuides(0, K)
            us = []
            for _ in range(3):
                tb.RenderGuides(0, K); us.append(tb.GetOption("last_guides_us"))
            res[name] = median(us)
    print("AB " + json.dumps(res))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "still_guides_waves_ab.json")
    for lib in LIBS.values():
        if not os.path.exists(lib):
            raise SystemExit("missing %s (see the docstring)" % lib)
    t = {tag: {name: [] for name in SCENES} for tag in LIBS}
    for _ in range(ROUNDS):
        for tag, lib in LIBS.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, TB_LIB=lib), capture_output=True, text=True, timeout=100)
            if r.returncode != 0:
                raise SystemExit("child failed (%s): %s" % (tag, r.stdout + r.stderr))
            got = json.loads([l for l in r.stdout.splitlines() if l.startswith("AB ")][-1][3:])
            for name, us in got.items():
                t[tag][name].append(us)
    result = {"what": "pt_guides, K = %d frames at %d x %d on one MI355X: last_guides_us, medians of %d alternating rounds of fresh processes" % (K, W, H, ROUNDS),
              "scenes": {name: {tag: {"us": median(t[tag][name]), "us_all": t[tag][name]} for tag in LIBS} for name in SCENES}}
    with open(out, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
