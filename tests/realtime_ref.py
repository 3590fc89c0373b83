"""NumPy float64 restatement of the real-time chain's three operations (tracerboy_amd/csrc/kernels/rt_kernels.hip): temporal accumulation
(TemporalAccumulationCS: reprojection through the previous camera, world-position history rejection, luminance moments), one a-trous
iteration (DenoiserCS) and the albedo composite (CompositeAlbedoCS).  Written from the shaders' operations, whole-array, in float64 with
libm's exp / power -- not from oracle/rt_ref.cpp, whose fp32 operation order it does not follow: what it shares with the oracle is the
operation, not the arithmetic.  The two choices the shaders leave to the hardware are the project's: a read outside a texture gives 0, the
bilinear CLAMP sample uses exact weights.  Imported by tests/test_realtime_kernels.py; holds no test itself."""
import numpy as np

F64 = np.float64
LUMA = np.array([np.float32(0.212671), np.float32(0.715160), np.float32(0.072169)], F64)   # Tonemap.h:12-15, as fp32 constants
EPSILON = F64(np.float32(0.0001))                                                          # SharedShaderStructs.h:3
KERNEL = np.array([3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0])


def luma(c):
    return np.asarray(c, F64)[..., :3] @ LUMA


def _vec(a):
    return np.array(a[:], F64)


def _norm(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _fetch(tex, ix, iy):
    """tex[iy, ix] with 0 outside the texture"""
    h, w = tex.shape[:2]
    inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    return np.where(inside[..., None], tex[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)], 0.0)


def _bilinear_clamp(tex, u, v):
    h, w = tex.shape[:2]
    fx, fy = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[..., None], (fy - y0)[..., None]
    xa, xb = np.clip(x0, 0, w - 1).astype(int), np.clip(x0 + 1, 0, w - 1).astype(int)
    ya, yb = np.clip(y0, 0, h - 1).astype(int), np.clip(y0 + 1, 0, h - 1).astype(int)
    top = tex[ya, xa] * (1 - tx) + tex[ya, xb] * tx
    bottom = tex[yb, xa] * (1 - tx) + tex[yb, xb] * tx
    return top * (1 - ty) + bottom * ty


def temporal(k, history, current, world_pos, prev_world_pos, moment_history, normals):
    """Returns (out, moments or None, info).  info["decision"]: per pixel, the distance to the nearest point where the operation is
    discontinuous -- u and v against 0 and 1, t against 0, |fx| and |fy| against 0 (int() truncates where frac() floors; at every other
    integer the picked taps and their weights change continuously), each tap's |dist - extent| / extent -- so that a comparison with an
    fp32 evaluation can leave out the pixels where rounding decides.  info["inside"] / ["behind"] / ["taps"]: the reprojection lands in
    [0, 1]^2; t < 0; how many of the four taps pass the world-position test (where inside)."""
    w, h = int(k.ResolutionX), int(k.ResolutionY)
    hist, cur, wp4, pwp, nrm = (np.asarray(a, F64).reshape(h, w, 4) for a in (history, current, world_pos, prev_world_pos, normals))
    wp = wp4[..., :3]
    moments = bool(k.OutputMomentInformation)
    mh = np.asarray(moment_history, F64).reshape(h, w, 4) if moments else None
    ppos, plook, pright, pup = _vec(k.PrevFrameCameraPosition), _vec(k.PrevFrameCameraLookAt), _vec(k.PrevFrameCameraRight), _vec(k.PrevFrameCameraUp)
    lens_h = F64(k.CameraLensHeight); lens_w = lens_h * (F64(w) / F64(h))
    with np.errstate(all="ignore"):
        pdir = _norm(plook - ppos)
        focal = ppos - F64(k.CameraFocalDistance) * pdir
        ray = _norm(wp - focal)
        hit = (nrm[..., :3] != 0).any(-1)
        # extent of the 3x3 neighbourhood's world positions; a neighbour counts only with both coordinates > 0 (as the shader has it)
        nmin, nmax = wp.copy(), wp.copy()
        ys, xs = np.mgrid[0:h, 0:w]
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                cx, cy = xs + dx, ys + dy
                ok = ((cx > 0) & (cy > 0) & (cx < w) & (cy < h))[..., None]
                nb = wp[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
                nmin = np.where(ok, np.fmin(nmin, nb), nmin); nmax = np.where(ok, np.fmax(nmax, nb), nmax)
        extent = np.sqrt(((nmax - nmin) ** 2).sum(-1))
        denom = ray @ pdir
        t = np.where(np.abs(denom) > 0, ((ppos - focal) @ pdir) / denom, -1.0)
        off = focal + ray * t[..., None] - ppos
        u = ((off @ pright) / (lens_w / 2) + 1) / 2
        v = 1 - ((off @ pup) / (lens_h / 2) + 1) / 2
        inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
        enter = inside & (t >= 0) & hit & (not k.IgnoreHistory)
        us, vs = np.where(inside, u, 0.5), np.where(inside, v, 0.5)       # harmless coordinates where the block is not entered
        fx, fy = us * w - 0.5, vs * h - 0.5
        ix0, iy0 = np.trunc(fx).astype(int), np.trunc(fy).astype(int)
        frx, fry = fx - np.floor(fx), fy - np.floor(fy)
        color = np.zeros((h, w, 3)); summed = np.zeros((h, w)); taps = np.zeros((h, w), int)
        decision = np.minimum.reduce([np.abs(u), np.abs(1 - u), np.abs(v), np.abs(1 - v), np.abs(t)])
        decision = np.where(np.isnan(decision), np.inf, decision)
        tap_decision = np.minimum(np.abs(fx), np.abs(fy))
        for x in (0, 1):
            for y in (0, 1):
                ix, iy = ix0 + x, iy0 + y
                dist = np.sqrt(((_fetch(pwp, ix, iy)[..., :3] - wp) ** 2).sum(-1))
                accept = dist < extent
                weight = (frx if x else 1 - frx) * (fry if y else 1 - fry)
                color += np.where(accept[..., None], _fetch(hist, ix, iy)[..., :3] * weight[..., None], 0.0)
                summed += np.where(accept, weight, 0.0); taps += accept
                rel = np.where(extent > 0, np.abs(dist - extent) / extent, np.where(dist > 0, np.inf, 0.0))
                tap_decision = np.minimum(tap_decision, np.where(np.isnan(rel), np.inf, rel))
        decision = np.where(enter, np.minimum(decision, tap_decision), decision)
        valid = enter & (summed > 0)
        prev_color = np.where(valid[..., None], color / summed[..., None], 0.0)
        alpha = np.ones((h, w)); mom = None
        if moments:
            prev_m = np.where(enter[..., None], _bilinear_clamp(mh, us, vs)[..., :3], 0.0)   # replaces the weighted value wherever the block is entered
            lum = luma(cur); count = prev_m[..., 2] + 1
            f = 1 / np.fmin(count, 32.0)
            m1 = prev_m[..., 0] + f * (lum - prev_m[..., 0]); m2 = prev_m[..., 1] + f * (lum * lum - prev_m[..., 1])
            mom = np.stack([m1, m2, count, np.zeros((h, w))], -1)
            alpha = np.fmax(m2 - m1 * m1, 0.0)
        hw = np.where(valid, F64(k.HistoryWeight), 0.0)[..., None]
        out = np.concatenate([cur[..., :3] + hw * (prev_color - cur[..., :3]), alpha[..., None]], -1)
    return out, mom, {"decision": decision, "inside": inside, "behind": t < 0, "taps": np.where(inside, taps, 0), "valid": valid}


def denoise(k, inp, normals, positions, undenoised):
    """One a-trous iteration: 5 x 5 taps dilated by OffsetMultiplier; weight = luminance x position x normal x kernel."""
    w, h = int(k.ResolutionX), int(k.ResolutionY)
    x, nrm, pos, und = (np.asarray(a, F64).reshape(h, w, 4) for a in (inp, normals, positions, undenoised))
    mult = int(k.OffsetMultiplier)
    n, p, footprint = nrm[..., :3], pos[..., :3], pos[..., 3]
    lum = luma(und)
    ys, xs = np.mgrid[0:h, 0:w]
    color = np.zeros((h, w, 3)); variance = np.zeros((h, w)); total = np.zeros((h, w))
    with np.errstate(all="ignore"):
        sigma = np.maximum(F64(k.LumaWeightingMultiplier) * np.sqrt(x[..., 3]), EPSILON)
        for xo in range(-2, 3):
            for yo in range(-2, 3):
                ox, oy = xo * mult, yo * mult
                cx, cy = xs + ox, ys + oy
                ok = (cx >= 0) & (cy >= 0) & (cx < w) & (cy < h)
                cxc, cyc = np.clip(cx, 0, w - 1), np.clip(cy, 0, h - 1)
                luma_w = np.exp(-np.abs(lum[cyc, cxc] - lum) / sigma)
                normal_w = np.power(np.maximum(0.0, (n * n[cyc, cxc]).sum(-1)), F64(k.NormalWeightingExponential))
                dist = np.sqrt(((p[cyc, cxc] - p) ** 2).sum(-1))
                pos_w = np.exp(-dist / (F64(k.IntersectionPositionWeightingMultiplier) * np.abs(ox * footprint + oy * footprint) + EPSILON))
                weight = np.where(ok, luma_w * pos_w * normal_w * KERNEL[abs(xo)] * KERNEL[abs(yo)], 0.0)
                color += weight[..., None] * x[cyc, cxc, :3]; variance += weight * weight * x[cyc, cxc, 3]; total += weight
        valid = (n != 0).any(-1)
        color = np.where(valid[..., None], color, x[..., :3]); variance = np.where(valid, variance, x[..., 3]); total = np.where(valid, total, 1.0)
        return np.concatenate([color / total[..., None], (variance / (total * total))[..., None]], -1)


def composite(albedo, lighting, emissive):
    """albedo * lighting * diffuse + lighting * (1 - diffuse) + emissive, alpha 1 (diffuse = albedo.w)."""
    a, l, e = (np.asarray(v, F64) for v in (albedo, lighting, emissive))
    d = a[..., 3:4]
    out = np.ones(a.shape)
    out[..., :3] = a[..., :3] * l[..., :3] * d + l[..., :3] * (1 - d) + e[..., :3]
    return out
