/* fsr_kernels.hip -- FSR 1 upscaling for the output stage: the reference's FidelityFXSuperResolutionPass::Run
 * (FidelityFXSuperResolution.cpp:53-111), restated.
 *
 *   fsr_easu_kernel   FidelityFXSuperResolutionCS.hlsl:16-43 over FsrEasuF / FsrEasuSetF / FsrEasuTapF (ffx_fsr1.h:239-437): edge-adaptive
 *                     spatial upsampling, 12 taps around the resolve position, the result clamped to the four nearest texels
 *   fsr_rcas_kernel   FidelityFXSharpenCS.hlsl:15-40 over FsrRcasF (ffx_fsr1.h:684-769): robust contrast-adaptive sharpening, a 5-tap cross;
 *                     FSR_RCAS_DENOISE and FSR_RCAS_PASSTHROUGH_ALPHA off, as in that shader
 *
 * Both are templates on the surface type (tb_abi.h TB_FSR_SURFACE_*): Unorm8 is the reference's R8G8B8A8_UNORM chain (a load is c / 255, a
 * store the conversion of post_process_kernel, alpha 255), F32 is RGBA32F with alpha 1, no clamp and no quantisation.
 *
 * Work shape: one wave64 per 16 x 16 output tile, four pixels per lane (the reference's numthreads(64, 1, 1) + four CurrFilter calls).  Lane l
 * owns column l & 15 of rows (l >> 4) + 4 k: a wave-wide store is four runs of 16 consecutive pixels (256 B each for F32), and the taps of a
 * wave-wide load fall into the few input rows under those runs.  No LDS tile: neighbouring lanes' taps overlap, but they overlap in L1 / L2 -- an
 * input row segment of a tile is read by at most 4 + 3 wave-wide loads.  ARmp8x8 is only a swizzle of the same 256 pixels.
 *
 * The four Gather4 of EASU under the CLAMP sampler are taken in integer form: each gather point is a texel corner ((fx + 1) / w, (fy - 1) / h
 * and its three neighbours, ffx_fsr1.h:177-201, 344-348), half a texel away from any rounding boundary, so the texels are (fx + dx, fy + dy)
 * with every coordinate clamped to the frame.  RCAS loads with Texture2D::Load: a tap outside the frame is (0, 0, 0).
 *
 * fp32 arithmetic is spelled out operation by operation (no contraction, tb_math.h primitives: min / max / saturate return the other operand
 * when one is NaN, as DXBC's do) and mirrored by tests/fsr_ref.py, which the tests compare bit for bit. */
#include <hip/hip_runtime.h>
#include "tb_math.h"
#include "tb_abi.h"
#include "fsr_launch.h"

namespace {

struct P3 { float x, y, z; };
__device__ __forceinline__ P3 p3(float x, float y, float z) { P3 r; r.x = x; r.y = y; r.z = z; return r; }

/* ffx_a.h:1843-1845: unsigned wraparound, no contraction */
__device__ __forceinline__ float rcp_lo(float a) { return tb_u2f(0x7ef07ebbu - tb_f2u(a)); }          /* APrxLoRcpF1 */
__device__ __forceinline__ float rsq_lo(float a) { return tb_u2f(0x5f347d74u - (tb_f2u(a) >> 1)); }   /* APrxLoRsqF1 */
__device__ __forceinline__ float rcp_med(float a) { float b = tb_u2f(0x7ef19fffu - tb_f2u(a)); return b * (-b * a + 2.0f); } /* APrxMedRcpF1 */

__device__ __forceinline__ float luma2(P3 c) { return c.z * 0.5f + (c.x * 0.5f + c.y); }              /* luma times 2, ffx_fsr1.h:363, 731 */
__device__ __forceinline__ float min3(float a, float b, float c) { return tb_min(a, tb_min(b, c)); }  /* AMin3F1, ffx_a.h:1166 */
__device__ __forceinline__ float max3(float a, float b, float c) { return tb_max(a, tb_max(b, c)); }  /* AMax3F1, ffx_a.h:1141 */

/* A surface type: its texel, how a texel becomes three floats and back.  kTable: the workgroup first fills a 256-entry LDS table with c / 255.0f
 * (fill_table) and loads look the channels up in it -- the same correctly rounded quotients, divided once per workgroup instead of 36 times per
 * EASU pixel (an IEEE division is about fifteen instructions here; spelled out per tap they held 230 VGPRs, two waves per SIMD). */
struct Unorm8 {
    typedef uint32_t Texel;
    static constexpr bool kTable = true;
    static __device__ __forceinline__ P3 load(const Texel* s, size_t i, const float* table)
    {
        const uint32_t v = s[i];
        return p3(table[v & 0xffu], table[(v >> 8) & 0xffu], table[(v >> 16) & 0xffu]);
    }
    static __device__ __forceinline__ void store(Texel* d, size_t i, P3 c) /* R8G8B8A8_UNORM store: clamp, scale, + 0.5, truncate (post_process_kernel) */
    {
        const uint32_t r = (uint32_t)(tb_saturate(c.x) * 255.0f + 0.5f), g = (uint32_t)(tb_saturate(c.y) * 255.0f + 0.5f),
            b = (uint32_t)(tb_saturate(c.z) * 255.0f + 0.5f);
        d[i] = r | (g << 8) | (b << 16) | 0xff000000u;
    }
};
struct F32 {
    typedef TbFloat4 Texel;
    static constexpr bool kTable = false;
    static __device__ __forceinline__ P3 load(const Texel* s, size_t i, const float*) { const TbFloat4 v = s[i]; return p3(v.x, v.y, v.z); }
    static __device__ __forceinline__ void store(Texel* d, size_t i, P3 c) { d[i] = TbFloat4{c.x, c.y, c.z, 1.0f}; }
};

/* every lane of the 64-lane workgroup, before any of them leaves */
template <class S> __device__ __forceinline__ void fill_table(float* table)
{
    if (S::kTable) {
        for (uint32_t c = threadIdx.x; c < 256u; c += 64u) table[c] = (float)c / 255.0f;
        __syncthreads();
    }
}

/* FsrEasuSetF, ffx_fsr1.h:275-313: direction and length from the '+' of lumas around one of the four nearest texels, weighted bilinearly
 *    a
 *  b c d
 *    e   */
__device__ __forceinline__ void easu_set(float& dirX, float& dirY, float& len, float w, float lA, float lB, float lC, float lD, float lE)
{
    const float dc = lD - lC, cb = lC - lB;
    float lenX = rcp_lo(tb_max(tb_abs(dc), tb_abs(cb)));
    const float dX = lD - lB;
    dirX = dirX + dX * w;
    lenX = tb_saturate(tb_abs(dX) * lenX);
    lenX = lenX * lenX;
    len = len + lenX * w;
    const float ec = lE - lC, ca = lC - lA;
    float lenY = rcp_lo(tb_max(tb_abs(ec), tb_abs(ca)));
    const float dY = lE - lA;
    dirY = dirY + dY * w;
    lenY = tb_saturate(tb_abs(dY) * lenY);
    lenY = lenY * lenY;
    len = len + lenY * w;
}

/* FsrEasuTapF, ffx_fsr1.h:239-272: the tap's offset rotated into the edge direction, stretched, weighted by the lanczos-2 approximation */
__device__ __forceinline__ void easu_tap(P3& aC, float& aW, float offX, float offY, float dirX, float dirY, float lenX, float lenY, float lob, float clp, P3 c)
{
    float vx = (offX * dirX) + (offY * dirY);
    float vy = (offX * (-dirY)) + (offY * dirX);
    vx = vx * lenX; vy = vy * lenY;
    float d2 = vx * vx + vy * vy;
    d2 = tb_min(d2, clp);
    float wB = (float)(2.0 / 5.0) * d2 + (-1.0f);
    float wA = lob * d2 + (-1.0f);
    wB = wB * wB;
    wA = wA * wA;
    wB = (float)(25.0 / 16.0) * wB + (float)(-(25.0 / 16.0 - 1.0));
    const float w = wB * wA;
    aC = p3(aC.x + c.x * w, aC.y + c.y * w, aC.z + c.z * w);
    aW = aW + w;
}

struct EasuArgs { uint32_t inW, inH, outW, outH; float con0[4]; };

/* FsrEasuF, ffx_fsr1.h:315-437 */
template <class S> __device__ __forceinline__ P3 easu_pixel(const EasuArgs& a, const typename S::Texel* in, const float* table, uint32_t ix, uint32_t iy)
{
    float ppx = (float)ix * a.con0[0] + a.con0[2], ppy = (float)iy * a.con0[1] + a.con0[3];
    const float fpx = tb_floor(ppx), fpy = tb_floor(ppy);
    ppx = ppx - fpx; ppy = ppy - fpy;
    /* the twelve texels, every coordinate clamped to the frame (the CLAMP sampler of the four gathers):
     *      b c            (fx, fy - 1) ...
     *    e f g h          (fx - 1, fy) ...
     *    i j k l
     *      n o   */
    const int fx = (int)fpx, fy = (int)fpy, mx = (int)a.inW - 1, my = (int)a.inH - 1;
    const size_t x0 = (size_t)min(max(fx - 1, 0), mx), x1 = (size_t)min(max(fx, 0), mx), x2 = (size_t)min(max(fx + 1, 0), mx), x3 = (size_t)min(max(fx + 2, 0), mx);
    const size_t r0 = (size_t)min(max(fy - 1, 0), my) * a.inW, r1 = (size_t)min(max(fy, 0), my) * a.inW, r2 = (size_t)min(max(fy + 1, 0), my) * a.inW,
        r3 = (size_t)min(max(fy + 2, 0), my) * a.inW;
    const P3 b = S::load(in, r0 + x1, table), c = S::load(in, r0 + x2, table);
    const P3 e = S::load(in, r1 + x0, table), f = S::load(in, r1 + x1, table), g = S::load(in, r1 + x2, table), h = S::load(in, r1 + x3, table);
    const P3 i = S::load(in, r2 + x0, table), j = S::load(in, r2 + x1, table), k = S::load(in, r2 + x2, table), l = S::load(in, r2 + x3, table);
    const P3 n = S::load(in, r3 + x1, table), o = S::load(in, r3 + x2, table);
    const float bL = luma2(b), cL = luma2(c), eL = luma2(e), fL = luma2(f), gL = luma2(g), hL = luma2(h), iL = luma2(i), jL = luma2(j), kL = luma2(k),
        lL = luma2(l), nL = luma2(n), oL = luma2(o);
    float dirX = 0.0f, dirY = 0.0f, len = 0.0f;
    easu_set(dirX, dirY, len, (1.0f - ppx) * (1.0f - ppy), bL, eL, fL, gL, jL);
    easu_set(dirX, dirY, len, ppx * (1.0f - ppy), cL, fL, gL, hL, kL);
    easu_set(dirX, dirY, len, (1.0f - ppx) * ppy, fL, iL, jL, kL, nL);
    easu_set(dirX, dirY, len, ppx * ppy, gL, jL, kL, lL, oL);
    /* normalise with the approximation, clean up close to zero (:389-395) */
    const float dir2x = dirX * dirX, dir2y = dirY * dirY;
    float dirR = dir2x + dir2y;
    const bool zro = dirR < (float)(1.0 / 32768.0);
    dirR = rsq_lo(dirR);
    dirR = zro ? 1.0f : dirR;
    dirX = zro ? 1.0f : dirX;
    dirX = dirX * dirR; dirY = dirY * dirR;
    len = len * 0.5f;
    len = len * len;
    const float stretch = (dirX * dirX + dirY * dirY) * rcp_lo(tb_max(tb_abs(dirX), tb_abs(dirY)));
    const float lenX = 1.0f + (stretch - 1.0f) * len, lenY = 1.0f + (-0.5f) * len;
    const float lob = 0.5f + (float)((1.0 / 4.0 - 0.04) - 0.5) * len;
    const float clp = rcp_lo(lob);
    const P3 mn = p3(tb_min(min3(f.x, g.x, j.x), k.x), tb_min(min3(f.y, g.y, j.y), k.y), tb_min(min3(f.z, g.z, j.z), k.z));
    const P3 mxc = p3(tb_max(max3(f.x, g.x, j.x), k.x), tb_max(max3(f.y, g.y, j.y), k.y), tb_max(max3(f.z, g.z, j.z), k.z));
    P3 aC = p3(0.0f, 0.0f, 0.0f); float aW = 0.0f;
    easu_tap(aC, aW, 0.0f - ppx, -1.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, b);
    easu_tap(aC, aW, 1.0f - ppx, -1.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, c);
    easu_tap(aC, aW, -1.0f - ppx, 1.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, i);
    easu_tap(aC, aW, 0.0f - ppx, 1.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, j);
    easu_tap(aC, aW, 0.0f - ppx, 0.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, f);
    easu_tap(aC, aW, -1.0f - ppx, 0.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, e);
    easu_tap(aC, aW, 1.0f - ppx, 1.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, k);
    easu_tap(aC, aW, 2.0f - ppx, 1.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, l);
    easu_tap(aC, aW, 2.0f - ppx, 0.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, h);
    easu_tap(aC, aW, 1.0f - ppx, 0.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, g);
    easu_tap(aC, aW, 1.0f - ppx, 2.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, o);
    easu_tap(aC, aW, 0.0f - ppx, 2.0f - ppy, dirX, dirY, lenX, lenY, lob, clp, n);
    /* normalise and dering (:437) */
    const float rW = 1.0f / aW;
    return p3(tb_min(mxc.x, tb_max(mn.x, aC.x * rW)), tb_min(mxc.y, tb_max(mn.y, aC.y * rW)), tb_min(mxc.z, tb_max(mn.z, aC.z * rW)));
}

template <class S> __global__ __launch_bounds__(64) void fsr_easu_kernel(EasuArgs a, const typename S::Texel* in, typename S::Texel* out)
{
    __shared__ float table[S::kTable ? 256 : 1];
    fill_table<S>(table);
    const uint32_t tilesX = (a.outW + 15u) / 16u;
    const uint32_t x = (blockIdx.x % tilesX) * 16u + (threadIdx.x & 15u), y0 = (blockIdx.x / tilesX) * 16u + (threadIdx.x >> 4);
    if (x >= a.outW) return;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t y = y0 + 4u * k;
        if (y >= a.outH) return;
        S::store(out, (size_t)y * a.outW + x, easu_pixel<S>(a, in, table, x, y));
    }
}

/* FsrRcasF, ffx_fsr1.h:684-769 */
template <class S> __device__ __forceinline__ P3 rcas_tap(const typename S::Texel* in, const float* table, uint32_t W, uint32_t H, int x, int y)
{
    if (x < 0 || y < 0 || x >= (int)W || y >= (int)H) return p3(0.0f, 0.0f, 0.0f); /* Texture2D::Load outside the resource */
    return S::load(in, (size_t)y * W + (size_t)x, table);
}
__device__ __forceinline__ float rcas_lobe(float b, float d, float f, float h) /* one channel's limiter (:741-758) */
{
    const float mn4 = tb_min(min3(b, d, f), h), mx4 = tb_max(max3(b, d, f), h);
    const float hitMin = mn4 * (1.0f / (4.0f * mx4));
    const float hitMax = (1.0f - mx4) * (1.0f / (4.0f * mn4 + (-4.0f)));
    return tb_max(-hitMin, hitMax);
}
template <class S> __device__ __forceinline__ P3 rcas_pixel(const typename S::Texel* in, const float* table, uint32_t W, uint32_t H, float con, int x, int y)
{
    /*    b
     *  d e f
     *    h   */
    const P3 b = rcas_tap<S>(in, table, W, H, x, y - 1), d = rcas_tap<S>(in, table, W, H, x - 1, y), e = rcas_tap<S>(in, table, W, H, x, y), f = rcas_tap<S>(in, table, W, H, x + 1, y),
        h = rcas_tap<S>(in, table, W, H, x, y + 1);
    const float lobeR = rcas_lobe(b.x, d.x, f.x, h.x), lobeG = rcas_lobe(b.y, d.y, f.y, h.y), lobeB = rcas_lobe(b.z, d.z, f.z, h.z);
    const float lobe = tb_max(-0.1875f /* FSR_RCAS_LIMIT = 0.25 - 1 / 16, ffx_fsr1.h:654 */, tb_min(max3(lobeR, lobeG, lobeB), 0.0f)) * con;
    const float rcpL = rcp_med(4.0f * lobe + 1.0f);
    return p3(((((lobe * b.x + lobe * d.x) + lobe * h.x) + lobe * f.x) + e.x) * rcpL, ((((lobe * b.y + lobe * d.y) + lobe * h.y) + lobe * f.y) + e.y) * rcpL,
              ((((lobe * b.z + lobe * d.z) + lobe * h.z) + lobe * f.z) + e.z) * rcpL);
}

template <class S> __global__ __launch_bounds__(64) void fsr_rcas_kernel(uint32_t W, uint32_t H, float con, const typename S::Texel* in, typename S::Texel* out)
{
    __shared__ float table[S::kTable ? 256 : 1];
    fill_table<S>(table);
    const uint32_t tilesX = (W + 15u) / 16u;
    const uint32_t x = (blockIdx.x % tilesX) * 16u + (threadIdx.x & 15u), y0 = (blockIdx.x / tilesX) * 16u + (threadIdx.x >> 4);
    if (x >= W) return;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t y = y0 + 4u * k;
        if (y >= H) return;
        S::store(out, (size_t)y * W + x, rcas_pixel<S>(in, table, W, H, con, (int)x, (int)y));
    }
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool sizesOk(uint32_t w, uint32_t h) { return w && h && (uint64_t)w * h <= (1ull << 24); }

} // namespace

extern "C" hipError_t fsr_launch_easu(hipStream_t stream, uint32_t surface, const uint32_t con0[4], uint32_t inW, uint32_t inH, uint32_t outW, uint32_t outH,
                                      const void* in, void* out)
{
    if (!con0 || !in || !out || in == out || !sizesOk(inW, inH) || !sizesOk(outW, outH)) return hipErrorInvalidValue;
    EasuArgs a; a.inW = inW; a.inH = inH; a.outW = outW; a.outH = outH;
    for (int i = 0; i < 4; i++) a.con0[i] = tb_u2f(con0[i]);
    const uint32_t tiles = ((outW + 15u) / 16u) * ((outH + 15u) / 16u);
    if (surface == TB_FSR_SURFACE_UNORM8) {
        if (!aligned(in, 4) || !aligned(out, 4)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(fsr_easu_kernel<Unorm8>, dim3(tiles), dim3(64), 0, stream, a, (const uint32_t*)in, (uint32_t*)out);
    } else if (surface == TB_FSR_SURFACE_F32) {
        if (!aligned(in, 16) || !aligned(out, 16)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(fsr_easu_kernel<F32>, dim3(tiles), dim3(64), 0, stream, a, (const TbFloat4*)in, (TbFloat4*)out);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" hipError_t fsr_launch_rcas(hipStream_t stream, uint32_t surface, uint32_t con, uint32_t W, uint32_t H, const void* in, void* out)
{
    if (!in || !out || in == out || !sizesOk(W, H)) return hipErrorInvalidValue;
    const uint32_t tiles = ((W + 15u) / 16u) * ((H + 15u) / 16u);
    if (surface == TB_FSR_SURFACE_UNORM8) {
        if (!aligned(in, 4) || !aligned(out, 4)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(fsr_rcas_kernel<Unorm8>, dim3(tiles), dim3(64), 0, stream, W, H, tb_u2f(con), (const uint32_t*)in, (uint32_t*)out);
    } else if (surface == TB_FSR_SURFACE_F32) {
        if (!aligned(in, 16) || !aligned(out, 16)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(fsr_rcas_kernel<F32>, dim3(tiles), dim3(64), 0, stream, W, H, tb_u2f(con), (const TbFloat4*)in, (TbFloat4*)out);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}
