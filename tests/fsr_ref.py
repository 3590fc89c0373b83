"""FSR 1 in NumPy, fp32 operation by operation: what fsr_kernels.hip has to reproduce bit for bit.

Written from the shader text -- FsrEasuCon / FsrEasuF / FsrEasuSetF / FsrEasuTapF (ffx_fsr1.h:156-202, 239-437), FsrRcasF (ffx_fsr1.h:684-769), the
approximate reciprocals (ffx_a.h:1843-1845) and the tap diagram of ffx_fsr1.h:177-201 -- not from the kernel.  Every value is an np.float32 /
np.uint32 array, every line is one rounded operation (no fused multiply-add), min / max are np.fmin / np.fmax: the other operand where one is NaN,
as DXBC's min / max; where both are zeros the sign is settled the way tb_math.h does it (-0 below +0), which np.fmin / np.fmax leave open.

An image is (H, W, C) with C >= 3, row 0 = top.  R8G8B8A8_UNORM: a load is c / 255, a store (uint32)(saturate(v) * 255 + 0.5), alpha 255;
RGBA32F: alpha 1, no clamp.  Both passes also return the intermediates the tests' branch pre-checks look at."""
import numpy as np

F = np.float32
U = np.uint32


def _f(a):
    return np.ascontiguousarray(a, F)


def _bits(a):
    return _f(a).view(U)


def _float(u):
    return np.ascontiguousarray(u, U).view(F)


def fmin(a, b):
    a, b = np.broadcast_arrays(_f(a), _f(b))
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, _float(_bits(a) | _bits(b)), np.fmin(a, b)).astype(F)


def fmax(a, b):
    a, b = np.broadcast_arrays(_f(a), _f(b))
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, _float(_bits(a) & _bits(b)), np.fmax(a, b)).astype(F)


def saturate(x):
    return fmin(fmax(x, F(0.0)), F(1.0))


def min3(a, b, c):
    return fmin(a, fmin(b, c))


def max3(a, b, c):
    return fmax(a, fmax(b, c))


def rcp_lo(a):      # APrxLoRcpF1
    return _float(U(0x7ef07ebb) - _bits(a))


def rsq_lo(a):      # APrxLoRsqF1
    return _float(U(0x5f347d74) - (_bits(a) >> U(1)))


def rcp_med(a):     # APrxMedRcpF1
    a = _f(a)
    b = _float(U(0x7ef19fff) - _bits(a))
    return b * (-b * a + F(2.0))


def luma2(c):
    return c[2] * F(0.5) + (c[0] * F(0.5) + c[1])


# ---- constants --------------------------------------------------------------------------------------------------------------------------
def easu_constants(in_w, in_h, out_w, out_h):
    """FsrEasuCon(viewport = in, size = in, out): sixteen uint32 words."""
    vx, vy = F(in_w), F(in_h)
    rox, roy, rix, riy = F(1.0) / F(out_w), F(1.0) / F(out_h), F(1.0) / vx, F(1.0) / vy
    k = [vx * rox, vy * roy, F(0.5) * vx * rox - F(0.5), F(0.5) * vy * roy - F(0.5),
         rix, riy, F(1.0) * rix, F(-1.0) * riy,
         F(-1.0) * rix, F(2.0) * riy, F(1.0) * rix, F(2.0) * riy,
         F(0.0) * rix, F(4.0) * riy]
    return np.concatenate([_bits(np.array(k, F)), np.zeros(2, U)])


def half_truncated(x):
    """AU1_AH1_AF1 for a positive normal binary16 result: the exponent rebased, the mantissa cut off."""
    u = int(_bits(np.array([x], F))[0])
    return (((u >> 23) & 0xff) - 112) << 10 | (u & 0x7fffff) >> 13


# ---- surfaces ---------------------------------------------------------------------------------------------------------------------------
def load_unorm8(img):
    return (np.asarray(img, np.uint8)[..., :3].astype(F) / F(255.0)).astype(F)


def store_unorm8(rgb):
    with np.errstate(all="ignore"):
        q = (saturate(rgb) * F(255.0) + F(0.5)).astype(U).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:2] + (1,), 255, np.uint8)], axis=-1)


def store_f32(rgb):
    return np.concatenate([_f(rgb), np.ones(rgb.shape[:2] + (1,), F)], axis=-1)


# ---- EASU -------------------------------------------------------------------------------------------------------------------------------
def _easu_set(acc, w, lA, lB, lC, lD, lE):
    """FsrEasuSetF:   a
                    b c d
                      e      acc = [dir.x, dir.y, len]"""
    dc = lD - lC
    cb = lC - lB
    lenX = rcp_lo(fmax(np.abs(dc), np.abs(cb)))
    dirX = lD - lB
    acc[0] = acc[0] + dirX * w
    lenX = saturate(np.abs(dirX) * lenX)
    lenX = lenX * lenX
    acc[2] = acc[2] + lenX * w
    ec = lE - lC
    ca = lC - lA
    lenY = rcp_lo(fmax(np.abs(ec), np.abs(ca)))
    dirY = lE - lA
    acc[1] = acc[1] + dirY * w
    lenY = saturate(np.abs(dirY) * lenY)
    lenY = lenY * lenY
    acc[2] = acc[2] + lenY * w


def easu(rgb, out_w, out_h, con):
    """rgb: (in_h, in_w, 3) float32 texel values; con: the sixteen words.  Returns ((out_h, out_w, 3) float32, intermediates)."""
    rgb = _f(np.asarray(rgb)[..., :3])
    in_h, in_w = rgb.shape[:2]
    c = _float(np.asarray(con, U)[:4])
    with np.errstate(all="ignore"):
        ipx, ipy = np.meshgrid(np.arange(out_w, dtype=U).astype(F), np.arange(out_h, dtype=U).astype(F))
        ppx = ipx * c[0] + c[2]
        ppy = ipy * c[1] + c[3]
        fpx, fpy = np.floor(ppx), np.floor(ppy)
        ppx = ppx - fpx
        ppy = ppy - fpy
        fx, fy = fpx.astype(np.int64), fpy.astype(np.int64)

        def texel(dx, dy):   # texel (fx + dx, fy + dy) under the CLAMP sampler, as three planes
            t = rgb[np.clip(fy + dy, 0, in_h - 1), np.clip(fx + dx, 0, in_w - 1)]
            return [_f(t[..., 0]), _f(t[..., 1]), _f(t[..., 2])]
        #    b c
        #  e f g h
        #  i j k l
        #    n o
        b, cc = texel(0, -1), texel(1, -1)
        e, f, g, h = texel(-1, 0), texel(0, 0), texel(1, 0), texel(2, 0)
        i, j, k, l = texel(-1, 1), texel(0, 1), texel(1, 1), texel(2, 1)
        n, o = texel(0, 2), texel(1, 2)
        bL, cL, eL, fL, gL, hL = luma2(b), luma2(cc), luma2(e), luma2(f), luma2(g), luma2(h)
        iL, jL, kL, lL, nL, oL = luma2(i), luma2(j), luma2(k), luma2(l), luma2(n), luma2(o)
        acc = [np.zeros_like(ppx), np.zeros_like(ppx), np.zeros_like(ppx)]
        one = F(1.0)
        _easu_set(acc, (one - ppx) * (one - ppy), bL, eL, fL, gL, jL)
        _easu_set(acc, ppx * (one - ppy), cL, fL, gL, hL, kL)
        _easu_set(acc, (one - ppx) * ppy, fL, iL, jL, kL, nL)
        _easu_set(acc, ppx * ppy, gL, jL, kL, lL, oL)
        dirx, diry, ln = acc
        dir2x = dirx * dirx
        dir2y = diry * diry
        dirR = dir2x + dir2y
        zro = dirR < F(1.0 / 32768.0)
        dirR = rsq_lo(dirR)
        dirR = np.where(zro, one, dirR).astype(F)
        dirx = np.where(zro, one, dirx).astype(F)
        dirx = dirx * dirR
        diry = diry * dirR
        ln = ln * F(0.5)
        ln = ln * ln
        stretch = (dirx * dirx + diry * diry) * rcp_lo(fmax(np.abs(dirx), np.abs(diry)))
        len2x = one + (stretch - one) * ln
        len2y = one + F(-0.5) * ln
        lob = F(0.5) + F((1.0 / 4.0 - 0.04) - 0.5) * ln
        clp = rcp_lo(lob)
        mn = [fmin(min3(f[q], g[q], j[q]), k[q]) for q in range(3)]
        mx = [fmax(max3(f[q], g[q], j[q]), k[q]) for q in range(3)]
        aC = [np.zeros_like(ppx), np.zeros_like(ppx), np.zeros_like(ppx)]
        aW = np.zeros_like(ppx)
        cut = np.zeros(ppx.shape, bool)
        for (ox, oy, t) in ((0, -1, b), (1, -1, cc), (-1, 1, i), (0, 1, j), (0, 0, f), (-1, 0, e), (1, 1, k), (2, 1, l), (2, 0, h), (1, 0, g),
                            (1, 2, o), (0, 2, n)):           # the order FsrEasuF accumulates in
            offx = F(ox) - ppx
            offy = F(oy) - ppy
            vx = (offx * dirx) + (offy * diry)
            vy = (offx * (-diry)) + (offy * dirx)
            vx = vx * len2x
            vy = vy * len2y
            d2 = vx * vx + vy * vy
            cut |= d2 > clp
            d2 = fmin(d2, clp)
            wB = F(2.0 / 5.0) * d2 + F(-1.0)
            wA = lob * d2 + F(-1.0)
            wB = wB * wB
            wA = wA * wA
            wB = F(25.0 / 16.0) * wB + F(-(25.0 / 16.0 - 1.0))
            w = wB * wA
            for q in range(3):
                aC[q] = aC[q] + t[q] * w
            aW = aW + w
        rW = one / aW
        pix = [fmin(mx[q], fmax(mn[q], aC[q] * rW)) for q in range(3)]
    out = _f(np.stack(pix, axis=-1))
    return out, dict(zro=zro, fx=fx, fy=fy, cut=cut, lo=_f(np.stack(mn, axis=-1)), hi=_f(np.stack(mx, axis=-1)))


# ---- RCAS -------------------------------------------------------------------------------------------------------------------------------
def rcas(rgb, con_bits):
    """rgb: (h, w, 3) float32; con_bits: rcas[0], the bits of exp2(-sharpness).  Returns ((h, w, 3) float32, intermediates)."""
    rgb = _f(np.asarray(rgb)[..., :3])
    hh, ww = rgb.shape[:2]
    con = _float(np.array([con_bits], U))[0]
    padded = np.zeros((hh + 2, ww + 2, 3), F)          # Texture2D::Load outside the resource is 0
    padded[1:-1, 1:-1] = rgb

    def tap(dx, dy):
        t = padded[1 + dy:1 + dy + hh, 1 + dx:1 + dx + ww]
        return [_f(t[..., 0]), _f(t[..., 1]), _f(t[..., 2])]
    #    b
    #  d e f
    #    h
    b, d, e, f, h = tap(0, -1), tap(-1, 0), tap(0, 0), tap(1, 0), tap(0, 1)
    with np.errstate(all="ignore"):
        lobes, nan_min, nan_max = [], np.zeros((hh, ww), bool), np.zeros((hh, ww), bool)
        for q in range(3):
            mn4 = fmin(min3(b[q], d[q], f[q]), h[q])
            mx4 = fmax(max3(b[q], d[q], f[q]), h[q])
            hitMin = mn4 * (F(1.0) / (F(4.0) * mx4))
            hitMax = (F(1.0) - mx4) * (F(1.0) / (F(4.0) * mn4 + F(-4.0)))
            nan_min |= np.isnan(hitMin)
            nan_max |= np.isnan(hitMax)
            lobes.append(fmax(-hitMin, hitMax))
        widest = max3(lobes[0], lobes[1], lobes[2])
        lobe = fmax(F(-0.1875), fmin(widest, F(0.0))) * con
        rcpL = rcp_med(F(4.0) * lobe + F(1.0))
        pix = [((((lobe * b[q] + lobe * d[q]) + lobe * h[q]) + lobe * f[q]) + e[q]) * rcpL for q in range(3)]
    ys, xs = np.mgrid[0:hh, 0:ww]
    outside = (ys == 0) | (xs == 0) | (ys == hh - 1) | (xs == ww - 1)
    return _f(np.stack(pix, axis=-1)), dict(nan_min=nan_min, nan_max=nan_max, widest=widest, lobe=lobe, con=con, outside=outside)


# ---- the passes on surfaces, and the chain ------------------------------------------------------------------------------------------------
def easu_surface(img, out_w, out_h, con):
    """img: uint8 (R8G8B8A8_UNORM) or float32 (RGBA32F), (H, W, 4) -> the same kind at out_h x out_w."""
    if np.asarray(img).dtype == np.uint8:
        return store_unorm8(easu(load_unorm8(img), out_w, out_h, con)[0])
    return store_f32(easu(img, out_w, out_h, con)[0])


def rcas_surface(img, con_bits):
    if np.asarray(img).dtype == np.uint8:
        return store_unorm8(rcas(load_unorm8(img), con_bits)[0])
    return store_f32(rcas(img, con_bits)[0])


def upscale(img, out_w, out_h, constants):
    """EASU -> RCAS as tb_upscale chains them; constants: the library's TbFsrConstants (easu words, rcas[0] as returned)."""
    h, w = np.asarray(img).shape[:2]
    easu_words = np.array(list(constants.easu), U)
    assert np.array_equal(easu_words, easu_constants(w, h, out_w, out_h)), "the constants are not those of these sizes"
    return rcas_surface(easu_surface(img, out_w, out_h, easu_words), int(constants.rcas[0]))
