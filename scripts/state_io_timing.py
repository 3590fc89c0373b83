"""What render states cost on one MI355X: GPU time of the two streaming kernels of state_kernels.hip from HIP events
(options last_state_digest_us / last_state_add_us), their achieved bytes per second against the HBM peak, and the wall time of a save and a
load, at 1080p and 4K.

    python scripts/state_io_timing.py [profiles/state_io.json]

state_digest reads both surfaces once (2 x W x H x 16 B); state_add reads four and writes two (6 x W x H x 16 B)."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box", "scene.pbrt")
HBM_PEAK = 8.0e12   # bytes per second, MI355X specification
REPEATS = 7


def median(v):
    return sorted(v)[len(v) // 2]


def measure(api, W, H, tmp):
    s = api.GetDefaultOutputSettings(); s.EnableBlueNoise = 0; s.MaxBounces = 2
    a, b = os.path.join(tmp, "a.tbs"), os.path.join(tmp, "b.tbs")
    with api.TracerBoy(0) as tb:
        tb.LoadScene(CORNELL)
        tb.BeginAccumulation(W, H, s, 0.0, first_frame=1); tb.Render(W, H, 1, s, 0.0); tb.SaveState(b)
        tb.InvalidateHistory(); tb.Render(W, H, 1, s, 0.0)
        digest_us = []
        for _ in range(REPEATS):
            tb.AccumDigest(); digest_us.append(tb.GetOption("last_state_digest_us"))
        save_s, load_s, add_us = [], [], []
        for _ in range(3):
            t0 = time.perf_counter(); tb.SaveState(a); save_s.append(time.perf_counter() - t0)
        for _ in range(REPEATS):
            t0 = time.perf_counter(); tb.LoadState(a); load_s.append(time.perf_counter() - t0)
            tb.LoadState(b, add=True); add_us.append(tb.GetOption("last_state_add_us"))
    surface = W * H * 16
    d, p = median(digest_us) * 1e-6, median(add_us) * 1e-6
    return {"width": W, "height": H, "surface_bytes": surface,
            "state_digest_us": median(digest_us), "state_digest_us_all": digest_us, "state_digest_gb_per_s": round(2 * surface / d / 1e9, 1),
            "state_digest_share_of_hbm_peak": round(2 * surface / d / HBM_PEAK, 3),
            "state_add_us": median(add_us), "state_add_us_all": add_us, "state_add_gb_per_s": round(6 * surface / p / 1e9, 1),
            "state_add_share_of_hbm_peak": round(6 * surface / p / HBM_PEAK, 3),
            "save_wall_ms": round(min(save_s) * 1e3, 2), "load_wall_ms": round(min(load_s) * 1e3, 2), "file_bytes": os.path.getsize(a)}


def main():
    from tracerboy_amd import api, build
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "state_io.json")
    with tempfile.TemporaryDirectory() as tmp:
        rows = [measure(api, 1920, 1080, tmp), measure(api, 3840, 2160, tmp)]
    result = {"what": "render-state kernels and file I/O, one MI355X; medians of %d" % REPEATS, "hbm_peak_bytes_per_s": HBM_PEAK,
              "kernel_digest": build.kernel_digest(), "sizes": rows}
    with open(out, "w") as f:
        json.dump(result, f, indent=1); f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
