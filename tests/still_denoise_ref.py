"""NumPy restatement of the denoise of a progressive render (tracerboy_amd/csrc/kernels/dn_kernels.hip): prepare,
prefilter and finish in float32 arrays, operation for operation in the kernels' order; the a-trous passes go through the oracle's DenoiserCS
(oracle_lib.denoise).  Imported by tests/test_still_denoise.py; holds no test itself."""
import numpy as np

F32 = np.float32


def luma(c):
    """ColorToLuma (Tonemap.h:12-15) in float32: (x * 0.212671 + y * 0.715160) + z * 0.072169."""
    c = np.asarray(c, F32)
    return (c[..., 0] * F32(0.212671) + c[..., 1] * F32(0.715160)) + c[..., 2] * F32(0.072169)


def prepare(output, jittered):
    """(mean colour, variance of the mean's luminance from the two halves).  output: sums over all samples, jittered: over the samples whose
    coin fell below 0.5 -- (H, W, 4) float32 (sum rgb * w, sum w)."""
    o, q = np.asarray(output, F32), np.asarray(jittered, F32)
    with np.errstate(all="ignore"):
        n, m = o[..., 3], q[..., 3]
        r = n - m
        c = np.where((n > 0)[..., None], o[..., :3] / n[..., None], F32(0))
        j = q[..., :3] / m[..., None]
        k = (o[..., :3] - q[..., :3]) / r[..., None]
        d = luma(j) - luma(k)
        v = (d * d) * ((m * r) / (n * n))
        v = np.where((m > 0) & (r > 0), v, F32(0))
        v = np.where(np.isfinite(v), v, F32(0))
    out = np.empty(o.shape, F32)
    out[..., :3] = c; out[..., 3] = v
    return out


def prefilter(prepared):
    """3x3 Gaussian over .w, coordinates clamped to the frame; taps dy = -1..1 outer, dx = -1..1 inner; acc = acc + weight * v from 0."""
    p = np.asarray(prepared, F32)
    h, w = p.shape[:2]
    k = (F32(0.5), F32(0.25))
    v = p[..., 3]
    acc = np.zeros((h, w), F32)
    for dy in (-1, 0, 1):
        ys = np.clip(np.arange(h) + dy, 0, h - 1)
        for dx in (-1, 0, 1):
            xs = np.clip(np.arange(w) + dx, 0, w - 1)
            weight = k[abs(dy)] * k[abs(dx)]
            acc = acc + weight * v[ys][:, xs]
    out = p.copy()
    out[..., 3] = acc
    return out


def finish(x):
    out = np.array(x, F32)
    out[..., 3] = F32(1)
    return out


def filter_passes(filtered, normals, positions, samples_rendered, dn):
    """WaveletIterations passes of DenoiserCS as tb_denoise runs them: input = the pass before (filtered for pass 0), undenoised = filtered,
    OffsetMultiplier = 1 << i, GlobalFrameCount = samples_rendered.  Returns the last pass's output, or None when no pass runs."""
    import oracle_lib as ol
    from tracerboy_amd import _ctypes_abi as abi
    h, w = filtered.shape[:2]
    x = None
    for i in range(dn.WaveletIterations if dn.Enabled else 0):
        k = abi.TbDenoiserConstants(w, h, 1 << i, dn.NormalWeightingExponential, dn.IntersectPositionWeightingMultiplier,
                                    dn.LuminanceWeightingMultiplier, samples_rendered)
        x = ol.denoise(k, filtered if x is None else x, normals, positions, filtered)
    return x


def chain(output, jittered, normals, positions, samples_rendered, dn):
    """The whole chain; the stages as tb_read_denoise_stage numbers them: [prepared, filtered, last filter pass or None, final]."""
    prepared = prepare(output, jittered)
    filtered = prefilter(prepared)
    last = filter_passes(filtered, normals, positions, samples_rendered, dn)
    return [prepared, filtered, last, finish(filtered if last is None else last)]


def rel_mse(x, ref):
    """mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01), in float64"""
    x, ref = np.asarray(x, np.float64)[..., :3], np.asarray(ref, np.float64)[..., :3]
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))
