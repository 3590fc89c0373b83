/* probe_launch.h -- the launchers of probe_kernels.hip and the arithmetic they share with the host: light probes around the two queries (DESIGN.md
 * section 25; include/tracerboy_hip.h tb_bake_probes, tb_sample_probes).
 *   probe_launch_rays     per (probe, texel of its M x M octahedral map) the ray record of the radiance query and that of the ray query
 *   probe_launch_project  per probe the TbProbe record: the rays' sums projected onto nine SH basis functions, the hits' statistics; one wave a probe
 *   probe_launch_sample   per point and normal the irradiance of a probe grid: eight corners, the invalid ones left out, the weights renormalised
 * Every pointer is a device pointer; ray records, sums, hit records and probe records are 16-B aligned.  2 <= M <= 64.  The launchers know neither
 * contexts nor options.  The functions marked PROBE_HD are the text the kernels and the host entry points (tb_probe_directions,
 * tb_sh9_irradiance: host_api.cpp, which includes no HIP header) both compile.
 *
 * THE ARITHMETIC IS THE CONTRACT (tests/probe_cases.py restates it in numpy).  Every operation below is one rounded binary32 + - x / sqrt, unfused,
 * in the order written; abs, negation, min, max, floor, the products with +-1 and the conversions of whole numbers below 2^24 are exact.
 *
 *   Directions.  A probe looks along the centres of an M x M octahedral map; texel t = y * M + x is ray t of the probe.
 *     h = 2.0f / (float)M;  u = ((x + 0.5f) * h) - 1;  v = ((y + 0.5f) * h) - 1;  z = (1 - |u|) - |v|
 *     where z < 0:  px = (1 - |v|) * sgn(u), py = (1 - |u|) * sgn(v), sgn(a) = (a < 0 ? -1 : +1);  else px = u, py = v
 *     len2 = ((px * px) + (py * py)) + z * z;  len = sqrt(len2);  direction = (px / len, py / len, z / len);  solid angle w = (h * h) / (len2 * len)
 *   (d omega = du dv / |p|^3 on the octahedron |x| + |y| + |z| = 1.)  The directions are not jittered: samples vary the paths.
 *
 *   Rays.  Probe i of a call (position P, number N = first_probe_number + i), ray t: the radiance record {Origin P, SeedX (float)N, Direction,
 *   SeedY (float)t}, the distance record {Origin P, TMax +inf, Direction, Flags 0}.  A probe with a coordinate that is not finite: both records all
 *   zero for every t -- neither query traces such a ray.
 *
 *   Basis, of a unit vector (x, y, z), each constant rounded to binary32:
 *     Y0 = c0                 c0 = 0.28209479177387814
 *     Y1 = c1 * y, Y2 = c1 * z, Y3 = c1 * x               c1 = 0.4886025119029199
 *     Y4 = c2 * (x * y), Y5 = c2 * (y * z)                 c2 = 1.0925484305920792
 *     Y6 = c3 * ((3 * (z * z)) - 1)                       c3 = 0.31539156525252005
 *     Y7 = c2 * (x * z)
 *     Y8 = c4 * ((x * x) - (y * y))                       c4 = 0.5462742152960396
 *
 *   Projection.  Lane l of the probe's wave takes the rays t = l, l + 64, ... in ascending order, starting from acc[j][c] = W = D = H = B = 0,
 *   Dmin = +inf.  With the radiance query's (sr, sg, sb, a) of the ray and the hit record (T, Normal) of the ray query:
 *     iff a > 0:   L_c = s_c / a;  q_c = L_c * w;  acc[j][c] = acc[j][c] + (q_c * Y_j) for j = 0 .. 8, c = r, g, b;  W = W + w
 *     iff T >= 0:  D = D + T;  H = H + 1;  Dmin = min(Dmin, T);  B = B + 1 where ((N.x * d.x) + (N.y * d.y)) + N.z * d.z > 0, d the direction
 *   Then the lanes are combined by six butterfly steps at lane distances 32, 16, 8, 4, 2, 1: v = v + (lane ^ distance's v) for the 27 acc, W, D, H
 *   and B, v = min(v, the other's) for Dmin.  Addition is commutative, so every lane ends with the same bits.  The record:
 *     SH[j * 3 + c] = (FOUR_PI * acc[j][c]) / W, FOUR_PI = 4 * 3.1415926535f; all 0 where W == 0
 *     Weight = W, Hits = H, Backfaces = B, MinDistance = Dmin, MeanDistance = D / H; both distances -1 where H == 0
 *   A probe with a coordinate that is not finite: 27 zeros, Weight = Hits = Backfaces = 0, both distances -1, whatever its rays' answers hold.
 *
 *   Irradiance of a record at the unit normal n, per channel c, with s_j = SH[j * 3 + c] and Y_j = Y_j(n) (probe_sh9_channel):
 *     E = (((A0 * s0) * Y0) + (A1 * (((s1 * Y1) + (s2 * Y2)) + (s3 * Y3))))
 *         + (A2 * (((((s4 * Y4) + (s5 * Y5)) + (s6 * Y6)) + (s7 * Y7)) + (s8 * Y8)))
 *     A0 = 3.1415926535f, A1 = 2.0943951f, A2 = 0.7853982f
 *
 *   Sampling a grid {origin, spacing, count} at the point P with the unit normal n.  Per axis a:
 *     g = (P[a] - origin[a]) / spacing[a];  g = min(max(g, 0), (float)(count[a] - 1))  (fmaxf, fminf: a NaN becomes 0)
 *     i0 = count[a] == 1 ? 0 : min((int)floor(g), count[a] - 2);  f = g - (float)i0
 *   Corner c = dz * 4 + dy * 2 + dx, c = 0 .. 7 in ascending order: the probe (min(i0x + dx, count[0] - 1), min(i0y + dy, count[1] - 1),
 *   min(i0z + dz, count[2] - 1)) -- the clamp only meets corners of weight 0, on an axis of one probe --, its weight
 *   wc = ((dx ? fx : 1 - fx) * (dy ? fy : 1 - fy)) * (dz ? fz : 1 - fz).  The corner counts iff its Weight > 0 and its
 *   Backfaces <= backface_limit * (float)(M * M); then S[k] = S[k] + (wc * SH[k]) for k = 0 .. 26 and Wsum = Wsum + wc, both from 0.
 *   Output: (E_r, E_g, E_b, Wsum) with E of the record S[k] / Wsum; (0, 0, 0, 0) where Wsum == 0 -- no valid probe was near. */
#pragma once
#include <math.h>
#include <stdint.h>
#include "tb_abi.h"

#if defined(__HIPCC__)
#define PROBE_HD __host__ __device__ static inline
#else
#define PROBE_HD static inline
#endif

#define PROBE_MIN_RES 2u
#define PROBE_MAX_RES 64u
#define PROBE_FOUR_PI (4.0f * 3.1415926535f)
#define PROBE_A0 3.1415926535f
#define PROBE_A1 2.0943951f
#define PROBE_A2 0.7853982f

/* ray t = y * M + x of an M x M map: the unit direction and its solid angle */
PROBE_HD void probe_direction(uint32_t M, uint32_t x, uint32_t y, float d[3], float* w)
{
    const float h = 2.0f / (float)M;
    const float u = (((float)x + 0.5f) * h) - 1.0f, v = (((float)y + 0.5f) * h) - 1.0f;
    const float au = fabsf(u), av = fabsf(v);
    const float z = (1.0f - au) - av;
    float px = u, py = v;
    if (z < 0.0f) { px = (1.0f - av) * (u < 0.0f ? -1.0f : 1.0f); py = (1.0f - au) * (v < 0.0f ? -1.0f : 1.0f); }
    const float len2 = ((px * px) + (py * py)) + z * z;
    const float len = sqrtf(len2);
    d[0] = px / len; d[1] = py / len; d[2] = z / len;
    *w = (h * h) / (len2 * len);
}

PROBE_HD void probe_basis(float x, float y, float z, float Y[9])
{
    const float c0 = 0.28209479177387814f, c1 = 0.4886025119029199f, c2 = 1.0925484305920792f, c3 = 0.31539156525252005f, c4 = 0.5462742152960396f;
    Y[0] = c0; Y[1] = c1 * y; Y[2] = c1 * z; Y[3] = c1 * x;
    Y[4] = c2 * (x * y); Y[5] = c2 * (y * z); Y[6] = c3 * ((3.0f * (z * z)) - 1.0f); Y[7] = c2 * (x * z); Y[8] = c4 * ((x * x) - (y * y));
}

/* the irradiance of one channel: s[j * stride] is coefficient j */
PROBE_HD float probe_sh9_channel(const float* s, int stride, const float Y[9])
{
    return (((PROBE_A0 * s[0]) * Y[0]) + (PROBE_A1 * (((s[1 * stride] * Y[1]) + (s[2 * stride] * Y[2])) + (s[3 * stride] * Y[3]))))
        + (PROBE_A2 * (((((s[4 * stride] * Y[4]) + (s[5 * stride] * Y[5])) + (s[6 * stride] * Y[6])) + (s[7 * stride] * Y[7])) + (s[8 * stride] * Y[8])));
}

PROBE_HD bool probe_finite(float x) { return fabsf(x) < INFINITY; } /* false for a NaN */

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
extern "C" {
/* positions: 3 floats per probe; n probes numbered from firstNumber; n * M * M records each, n * M * M <= 2^31 */
hipError_t probe_launch_rays(hipStream_t stream, const float* positions, uint32_t n, uint32_t M, uint32_t firstNumber, TbRadianceRay* radianceRays,
                             TbQueryRay* queryRays);
/* sums, hits: n * M * M answers of the two queries in the rays' order; probes: n records */
hipError_t probe_launch_project(hipStream_t stream, const float* positions, uint32_t n, uint32_t M, const TbFloat4* sums, const TbQueryHit* hits,
                                TbProbe* probes);
/* probes: count[0] * count[1] * count[2] records (at most 2^24, so that every index is an exact float); points, normals: 3 floats per point; out: n x (E_r, E_g, E_b, Wsum) */
hipError_t probe_launch_sample(hipStream_t stream, const tb_probe_grid* grid, uint32_t M, float backfaceLimit, const TbProbe* probes, uint32_t n,
                               const float* points, const float* normals, TbFloat4* out);
}
#endif
