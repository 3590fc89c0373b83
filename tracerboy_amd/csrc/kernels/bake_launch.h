/* bake_launch.h -- the launchers of bake_kernels.hip: lightmap baking around the radiance query (include/tracerboy_hip.h
 * tb_bake_lightmap).
 *   bake_launch_raster   which texel of a W x H atlas belongs to which triangle (bake_cover), then per texel a ray record of section 22 and a
 *                        TbBakeTexel (bake_texels); counts the texels that have a triangle
 *   bake_launch_resolve  sums of a hemisphere query -> irradiance, alpha 1 on covered texels
 *   bake_launch_dilate   one 3 x 3 fill pass
 * Every pointer is a device pointer unless it says otherwise; rays, texels, sums and pictures are 16-B aligned.  1 <= W, H <= BAKE_MAX_SIDE.  The
 * launchers know neither contexts nor options.
 *
 * THE ARITHMETIC IS THE CONTRACT (tests/bake_cases.py restates it in numpy).  Every operation below is one rounded binary32 + - x / sqrt, unfused,
 * in the order written; min, max, floor, abs, negation and the products with 0.5 are exact.
 *
 *   Coverage.  Vertex k of triangle t has the lightmap UV (u, v); its texel-space point is p = (u * W, v * H).  Texel (x, y) has the centre
 *   c = (x + 0.5, y + 0.5).  E(a, b, q) = (b.x - a.x) * (q.y - a.y) - (b.y - a.y) * (q.x - a.x).  A = E(p0, p1, p2).  A triangle is skipped when
 *   A == 0, when A or a coordinate of a p is not finite, or when a vertex number is not below the vertex count.  Where A < 0, vertices 1 and 2
 *   change places with all that belongs to them (p, position, normal) and A is E of the new order (its negation, exactly).  The candidates of a
 *   triangle are the texels x in [max(floor(min p.x), 0), min(floor(max p.x), W - 1)], y likewise: the box clipped to the atlas, no wrap.  (Every
 *   candidate's square meets the box: the issue's second condition of class 1 holds by construction.)  With e0 = E(p1, p2, c), e1 = E(p2, p0, c),
 *   e2 = E(p0, p1, c):
 *     class 0   e0 >= 0 && e1 >= 0 && e2 >= 0                                                       (the centre is covered)
 *     class 1   not class 0, and for each edge (a, b) of the three  e >= -(0.5 * (|b.x - a.x| + |b.y - a.y|))   (the conservative offset)
 *   A texel keeps the smallest key (class << 32) | t of the triangles that claim it, by a 64-bit atomic minimum on a word that starts as all
 *   ones: a centre hit beats an edge hit, the lower index wins among equals, and no schedule changes the result.
 *
 *   Texel records.  No key: an all-zero ray (section 22 does not trace it) and the texel {0xffffffff, 0, 0, 0}.  Else, with the key's triangle in
 *   the rasteriser's order: w0 = e0 / A, w1 = e1 / A, w2 = (1 - w0) - w1; class 1: each w becomes (w > 0 ? w : 0), then s = (w0 + w1) + w2 and
 *   each w becomes w / s.  Origin = ((P0 * w0) + (P1 * w1)) + (P2 * w2) per component; n the same blend of the three normals;
 *   len2 = ((n.x * n.x) + (n.y * n.y)) + n.z * n.z; Direction = n / sqrt(len2) where len2 is finite and > 0, else g / sqrt(len2 of g) with
 *   g = cross(Q1 - Q0, Q2 - Q0) of the positions in the CALLER's order, cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z,
 *   a.x * b.y - a.y * b.x); if that len2 fails too, or a component of Origin or Direction is not finite, the texel counts as having no key.
 *   SeedX = (float)x, SeedY = (float)y.  The texel record holds the triangle, the class and the weights of the caller's vertices 0 and 1 (where
 *   1 and 2 changed places, w1 of the record is the rasteriser's w2).
 *
 *   Resolve.  A texel with a triangle whose accepted count a3 = sum.w is > 0: rgb = (PI * sum) / a3 with PI = 3.1415926535f, alpha 1; every other
 *   texel (0, 0, 0, 0).
 *
 *   Dilate, pass p = 1, 2, ...: a texel with alpha > 0 is copied.  Any other looks at its 3 x 3 neighbours inside the atlas in row-major order (dy
 *   -1 .. 1 outer, dx -1 .. 1 inner), sums the rgb of those with alpha > 0 from 0, one addition per neighbour, counts them as m, and where m > 0
 *   becomes (sum / (float)m, 2^-p); else it is copied. */
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "tb_abi.h"

#define BAKE_MAX_SIDE 8192u
#define BAKE_TILE 8u /* a work item of bake_cover is one triangle's share of one BAKE_TILE x BAKE_TILE texel tile of the atlas: one wave, a lane per texel */

/* the mesh a bake reads: positions 3 floats per vertex; normals and uv at a stride in floats (3 and 2 for plain arrays; 8 and 8 with uv = the
 * vertex buffer + 3 for the scene's 32-B vertex records); triVerts 3 vertex numbers per triangle */
typedef struct BakeMesh {
    const float* positions; const float* normals; const float* uv; const uint32_t* triVerts;
    uint32_t normalStride, uvStride, numTris, numVertices;
} BakeMesh;

extern "C" {
/* bytes of scratch bake_launch_raster needs for numTris triangles on a W x H atlas: the keys, the tile counts, their scan, rocPRIM's own */
size_t bake_raster_scratch_bytes(uint32_t numTris, uint32_t W, uint32_t H);
/* covered: one device word, receives the number of texels with a triangle.  Waits for the stream once (the number of work items comes back). */
hipError_t bake_launch_raster(hipStream_t stream, const BakeMesh* mesh, uint32_t W, uint32_t H, void* scratch, size_t scratchBytes, TbRadianceRay* rays,
                              TbBakeTexel* texels, uint32_t* covered);
hipError_t bake_launch_resolve(hipStream_t stream, uint64_t n, const TbBakeTexel* texels, const TbFloat4* sums, TbFloat4* rgba);
/* pass: 1 .. 16; in and out are different surfaces */
hipError_t bake_launch_dilate(hipStream_t stream, uint32_t W, uint32_t H, uint32_t pass, const TbFloat4* in, TbFloat4* out);
}
