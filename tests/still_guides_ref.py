"""NumPy restatement of the guide pass and its denoise chain (tracerboy_amd/csrc/kernels/guide_kernels.hip and the
dn_*_guides / dn_*_demod / dn_*_remod kernels of dn_kernels.hip): the sums in float32 in frame order, the resolve, the demodulated prepare and
the remodulating finish operation for operation in the kernels' order; prefilter and a-trous passes are section 12's (tests/still_denoise_ref.py).
Imported by tests/test_still_guides.py; holds no test itself."""
import numpy as np

import still_denoise_ref as ref

F32 = np.float32


def oracle_frame(view, pf, width, height, frame, threads=8):
    """(normal, albedo, position) AOVs of one frame from the oracle, each (H, W, 4): position = (world position, distance to the neighbour's hit),
    the world-position target of the frame's parity."""
    import oracle_lib as ol
    r = ol.render(view, pf, width, height, 1, first_frame=frame, threads=threads, aovs=True)
    return r["normals"], r["custom"], r["worldpos1"] if frame % 2 else r["worldpos0"]


def guide_sums(frames):
    """frames: (normal, albedo, position) per frame, in frame order.  Returns the three guide surfaces (albedo, normal, position) as the kernel
    sums them: acc = acc + v from 0, a frame hits where its normal is not all zero, its effective albedo is 1 where its albedo is all zero."""
    h, w = np.asarray(frames[0][0]).shape[:2]
    A, N, P = (np.zeros((h, w, 4), F32) for _ in range(3))
    one = F32(1)
    for normal, albedo, position in frames:
        n, a, p = (np.asarray(v, F32) for v in (normal, albedo, position))
        hit = (n[..., :3] != 0).any(-1)
        lit = (a[..., :3] != 0).any(-1)
        e = np.where(lit[..., None], a[..., :3], one)
        A[..., :3] = A[..., :3] + e
        A[..., 3] = A[..., 3] + one
        N[..., :3] = np.where(hit[..., None], N[..., :3] + n[..., :3], N[..., :3])
        N[..., 3] = np.where(hit, N[..., 3] + one, N[..., 3])
        P[...] = np.where(hit[..., None], P + p, P)
    return A, N, P


def resolve(N, P):
    """(normals, positions) the filter reads: sums / frames that hit, a mean of several normals brought back to length 1; (0, 0, 0, 1) and 0 where
    no frame hit."""
    N, P = np.asarray(N, F32), np.asarray(P, F32)
    hits = N[..., 3]
    some = hits > 0
    with np.errstate(all="ignore"):
        normals = np.where(some[..., None], N / hits[..., None], F32(0)).astype(F32)
        positions = np.where(some[..., None], P / hits[..., None], F32(0)).astype(F32)
        # more than one frame: the mean's direction (DenoiserCS raises dot products of normals to the 128th power), zero where the sum cancels
        x, y, z = normals[..., 0], normals[..., 1], normals[..., 2]
        l = np.sqrt((x * x + y * y) + z * z)
        unit = np.where((l > 0)[..., None], normals[..., :3] / l[..., None], F32(0))
        normals[..., :3] = np.where((hits > 1)[..., None], unit, normals[..., :3])
    normals[..., 3] = F32(1)
    return normals, positions


def demod(A):
    """d = max(mean effective albedo, 0.01) per channel, (H, W, 3)"""
    A = np.asarray(A, F32)
    with np.errstate(all="ignore"):
        a = A[..., :3] / A[..., 3:4]
    return np.where(a > F32(0.01), a, F32(0.01)).astype(F32)


def prepare_demod(output, jittered, A):
    """still_denoise_ref.prepare with the mean colour and both halves' means divided by d"""
    o, q, d = np.asarray(output, F32), np.asarray(jittered, F32), demod(A)
    with np.errstate(all="ignore"):
        n, m = o[..., 3], q[..., 3]
        r = n - m
        c = np.where((n > 0)[..., None], (o[..., :3] / n[..., None]) / d, F32(0))
        j = (q[..., :3] / m[..., None]) / d
        k = ((o[..., :3] - q[..., :3]) / r[..., None]) / d
        dl = ref.luma(j) - ref.luma(k)
        v = (dl * dl) * ((m * r) / (n * n))
        v = np.where((m > 0) & (r > 0), v, F32(0))
        v = np.where(np.isfinite(v), v, F32(0))
    out = np.empty(o.shape, F32)
    out[..., :3] = c; out[..., 3] = v
    return out


def finish_remod(x, A):
    out = np.empty(np.asarray(x).shape, F32)
    out[..., :3] = np.asarray(x, F32)[..., :3] * demod(A)
    out[..., 3] = F32(1)
    return out


def chain(output, jittered, A, N, P, samples_rendered, dn, mode):
    """tb_denoise with option denoise_guides = mode (1 or 2) on the guide surfaces; the stages as tb_read_denoise_stage numbers them:
    [prepared, filtered, last filter pass or None, final].  Mode 2: stages 0-2 in the demodulated domain, stage 3 remodulated."""
    normals, positions = resolve(N, P)
    prepared = prepare_demod(output, jittered, A) if mode == 2 else ref.prepare(output, jittered)
    filtered = ref.prefilter(prepared)
    last = ref.filter_passes(filtered, normals, positions, samples_rendered, dn)
    x = filtered if last is None else last
    return [prepared, filtered, last, finish_remod(x, A) if mode == 2 else ref.finish(x)]
