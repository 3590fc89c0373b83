/* bake_kernels.hip -- lightmap baking around the radiance query (include/tracerboy_hip.h tb_bake_lightmap): the rasteriser of a
 * UV atlas, the texels' ray records, the resolve of the traced sums and the gutter fill.  bake_launch.h states the arithmetic, which is the contract.
 *
 *   bake_tiles     one lane per triangle: how many BAKE_TILE x BAKE_TILE tiles of the atlas its clipped box touches
 *   (rocPRIM)      exclusive scan of those counts: where each triangle's work items begin
 *   bake_cover     one wave per work item = (triangle, tile), one lane per texel of the tile: the two coverage classes, a 64-bit atomic minimum
 *                  per claimed texel.  The item's triangle is found by a bisection of the scanned counts, the same in all 64 lanes.
 *   bake_texels    one lane per texel: barycentrics, origin, direction, the two records; counts the texels that kept a triangle
 *   bake_resolve   one lane per texel: pi * sum / count
 *   bake_dilate    one lane per texel: one 3 x 3 fill pass
 * Work is handed out by tiles, not by triangles: a quad that spans the atlas is 2^20 items of one wave each at 8192 x 8192, not one lane's loop.
 * Every index a kernel forms is below a count it was given: texels below W x H, triangles below numTris, vertices below numVertices (a triangle
 * that names a vertex past the count is skipped). */
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "tb_abi.h"
#include "bake_launch.h"

namespace {

constexpr int BLOCK = 256;
constexpr float BAKE_PI = 3.1415926535f; /* pt_device.hpp PI */
constexpr unsigned long long NO_KEY = ~0ull;
#define BAKE_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

__device__ __forceinline__ bool finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); } /* false for a NaN */
__device__ __forceinline__ float edge(float ax, float ay, float bx, float by, float qx, float qy) { return (bx - ax) * (qy - ay) - (by - ay) * (qx - ax); }
__device__ __forceinline__ float offset(float ax, float ay, float bx, float by) { return -(0.5f * (__builtin_fabsf(bx - ax) + __builtin_fabsf(by - ay))); }

/* a triangle in the rasteriser's order: the vertex numbers, the texel-space points, A > 0, the clipped box */
struct Setup { uint32_t v[3]; float px[3], py[3], A; bool swapped; int x0, y0, x1, y1; };

__device__ __forceinline__ bool bake_setup(const BakeMesh& m, uint32_t W, uint32_t H, uint32_t t, Setup& s)
{
    const float fw = (float)W, fh = (float)H;
    for (int k = 0; k < 3; k++) {
        s.v[k] = m.triVerts[3ull * t + k];
        if (s.v[k] >= m.numVertices) return false;
        s.px[k] = m.uv[(size_t)m.uvStride * s.v[k]] * fw; s.py[k] = m.uv[(size_t)m.uvStride * s.v[k] + 1] * fh;
        if (!finite(s.px[k]) || !finite(s.py[k])) return false;
    }
    s.A = edge(s.px[0], s.py[0], s.px[1], s.py[1], s.px[2], s.py[2]);
    if (!finite(s.A) || s.A == 0.0f) return false;
    s.swapped = s.A < 0.0f;
    if (s.swapped) {
        const uint32_t v = s.v[1]; s.v[1] = s.v[2]; s.v[2] = v;
        const float x = s.px[1]; s.px[1] = s.px[2]; s.px[2] = x;
        const float y = s.py[1]; s.py[1] = s.py[2]; s.py[2] = y;
        s.A = edge(s.px[0], s.py[0], s.px[1], s.py[1], s.px[2], s.py[2]);
    }
    const float lox = floorf(fminf(fminf(s.px[0], s.px[1]), s.px[2])), hix = floorf(fmaxf(fmaxf(s.px[0], s.px[1]), s.px[2]));
    const float loy = floorf(fminf(fminf(s.py[0], s.py[1]), s.py[2])), hiy = floorf(fmaxf(fmaxf(s.py[0], s.py[1]), s.py[2]));
    if (hix < 0.0f || hiy < 0.0f || lox > fw - 1.0f || loy > fh - 1.0f) return false;
    s.x0 = (int)fmaxf(lox, 0.0f); s.x1 = (int)fminf(hix, fw - 1.0f); s.y0 = (int)fmaxf(loy, 0.0f); s.y1 = (int)fminf(hiy, fh - 1.0f);
    return true;
}

__global__ __launch_bounds__(BLOCK) void bake_tiles(BakeMesh m, uint32_t W, uint32_t H, unsigned long long* __restrict__ counts)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t > m.numTris) return;
    unsigned long long n = 0; /* entry numTris stays 0: the scan's last output is the total */
    Setup s;
    if (t < m.numTris && bake_setup(m, W, H, t, s))
        n = (unsigned long long)((s.x1 / (int)BAKE_TILE) - (s.x0 / (int)BAKE_TILE) + 1) * (unsigned long long)((s.y1 / (int)BAKE_TILE) - (s.y0 / (int)BAKE_TILE) + 1);
    counts[t] = n;
}

/* first: numTris + 1 scanned counts; the items [itemBase, itemEnd) of this launch, one per wave */
__global__ __launch_bounds__(BLOCK) void bake_cover(BakeMesh m, uint32_t W, uint32_t H, const unsigned long long* __restrict__ first,
    unsigned long long itemBase, unsigned long long itemEnd, unsigned long long* __restrict__ keys)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const unsigned long long item = itemBase + (unsigned long long)blockIdx.x * (BLOCK / 64) + wave;
    if (item >= itemEnd) return;
    uint32_t lo = 0, hi = m.numTris; /* the last t with first[t] <= item: first[0] = 0 <= item < first[numTris] */
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (first[mid] <= item) lo = mid; else hi = mid; }
    const uint32_t t = lo;
    Setup s;
    if (!bake_setup(m, W, H, t, s)) return; /* (not reached: such a triangle has no items) */
    const uint32_t local = (uint32_t)(item - first[t]);
    const uint32_t tilesX = (uint32_t)(s.x1 / (int)BAKE_TILE - s.x0 / (int)BAKE_TILE + 1);
    const int x = (s.x0 / (int)BAKE_TILE + (int)(local % tilesX)) * (int)BAKE_TILE + (int)(lane & 7u);
    const int y = (s.y0 / (int)BAKE_TILE + (int)(local / tilesX)) * (int)BAKE_TILE + (int)(lane >> 3);
    if (x < s.x0 || x > s.x1 || y < s.y0 || y > s.y1) return;
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const float e0 = edge(s.px[1], s.py[1], s.px[2], s.py[2], cx, cy), e1 = edge(s.px[2], s.py[2], s.px[0], s.py[0], cx, cy),
                e2 = edge(s.px[0], s.py[0], s.px[1], s.py[1], cx, cy);
    uint32_t cls;
    if (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) cls = 0u;
    else if (e0 >= offset(s.px[1], s.py[1], s.px[2], s.py[2]) && e1 >= offset(s.px[2], s.py[2], s.px[0], s.py[0]) &&
             e2 >= offset(s.px[0], s.py[0], s.px[1], s.py[1])) cls = 1u;
    else return;
    const unsigned long long key = ((unsigned long long)cls << 32) | t;
    unsigned long long* at = keys + (size_t)y * W + (uint32_t)x;
    /* a key only ever falls: one that is already no larger than ours makes the atomic pointless */
    if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) (void)atomicMin(at, key);
}

__device__ __forceinline__ float blend(float a, float b, float c, float w0, float w1, float w2) { return ((a * w0) + (b * w1)) + (c * w2); }
__device__ __forceinline__ float len2of(float x, float y, float z) { return ((x * x) + (y * y)) + z * z; }

__global__ __launch_bounds__(BLOCK) void bake_texels(BakeMesh m, uint32_t W, uint32_t H, const unsigned long long* __restrict__ keys,
    TbRadianceRay* __restrict__ rays, TbBakeTexel* __restrict__ texels, uint32_t* covered)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, n = W * H;
    bool has = false;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f}, rw0 = 0.0f, rw1 = 0.0f;
    uint32_t tri = 0xffffffffu, cls = 0u;
    const uint32_t x = i < n ? i % W : 0u, y = i < n ? i / W : 0u;
    const unsigned long long key = i < n ? keys[i] : NO_KEY;
    Setup s;
    if (key != NO_KEY && bake_setup(m, W, H, (uint32_t)key, s)) {
        const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
        const float e0 = edge(s.px[1], s.py[1], s.px[2], s.py[2], cx, cy), e1 = edge(s.px[2], s.py[2], s.px[0], s.py[0], cx, cy);
        float w0 = e0 / s.A, w1 = e1 / s.A, w2 = (1.0f - w0) - w1;
        if ((uint32_t)(key >> 32)) {
            w0 = w0 > 0.0f ? w0 : 0.0f; w1 = w1 > 0.0f ? w1 : 0.0f; w2 = w2 > 0.0f ? w2 : 0.0f;
            const float sum = (w0 + w1) + w2;
            w0 = w0 / sum; w1 = w1 / sum; w2 = w2 / sum;
        }
        const float* P[3]; const float* N[3];
        for (int k = 0; k < 3; k++) { P[k] = m.positions + 3ull * s.v[k]; N[k] = m.normals + (size_t)m.normalStride * s.v[k]; }
        float nn[3];
        for (int k = 0; k < 3; k++) { o[k] = blend(P[0][k], P[1][k], P[2][k], w0, w1, w2); nn[k] = blend(N[0][k], N[1][k], N[2][k], w0, w1, w2); }
        float len2 = len2of(nn[0], nn[1], nn[2]);
        if (!(finite(len2) && len2 > 0.0f)) { /* the geometric normal, in the caller's winding */
            const float* Q1 = s.swapped ? P[2] : P[1]; const float* Q2 = s.swapped ? P[1] : P[2];
            const float ax = Q1[0] - P[0][0], ay = Q1[1] - P[0][1], az = Q1[2] - P[0][2], bx = Q2[0] - P[0][0], by = Q2[1] - P[0][1], bz = Q2[2] - P[0][2];
            nn[0] = ay * bz - az * by; nn[1] = az * bx - ax * bz; nn[2] = ax * by - ay * bx;
            len2 = len2of(nn[0], nn[1], nn[2]);
        }
        if (finite(len2) && len2 > 0.0f) {
            const float len = sqrtf(len2);
            for (int k = 0; k < 3; k++) d[k] = nn[k] / len;
            has = finite(o[0]) && finite(o[1]) && finite(o[2]) && finite(d[0]) && finite(d[1]) && finite(d[2]);
        }
        if (has) { tri = (uint32_t)key; cls = (uint32_t)(key >> 32); rw0 = w0; rw1 = s.swapped ? w2 : w1; }
    }
    if (i < n) {
        float4* r = (float4*)(rays + i);
        r[0] = has ? make_float4(o[0], o[1], o[2], (float)x) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        r[1] = has ? make_float4(d[0], d[1], d[2], (float)y) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        *(uint4*)(texels + i) = make_uint4(tri, cls, __float_as_uint(rw0), __float_as_uint(rw1));
    }
    const unsigned long long got = __ballot(has);
    if ((threadIdx.x & 63u) == 0u && got) (void)atomicAdd(covered, (uint32_t)__popcll(got));
}

__global__ __launch_bounds__(BLOCK) void bake_resolve(uint32_t n, const TbBakeTexel* __restrict__ texels, const TbFloat4* __restrict__ sums,
    TbFloat4* __restrict__ rgba)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const TbFloat4 s = sums[i];
    TbFloat4 out = {0.0f, 0.0f, 0.0f, 0.0f};
    if (texels[i].triangle != 0xffffffffu && s.w > 0.0f) { out.x = (BAKE_PI * s.x) / s.w; out.y = (BAKE_PI * s.y) / s.w; out.z = (BAKE_PI * s.z) / s.w; out.w = 1.0f; }
    rgba[i] = out;
}

__global__ __launch_bounds__(BLOCK) void bake_dilate(uint32_t W, uint32_t H, float alpha, const TbFloat4* __restrict__ in, TbFloat4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= W * H) return;
    const int x = (int)(i % W), y = (int)(i / W);
    TbFloat4 v = in[i];
    if (!(v.w > 0.0f)) {
        float r = 0.0f, g = 0.0f, b = 0.0f; uint32_t m = 0;
        for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
            const TbFloat4 q = in[(size_t)qy * W + (uint32_t)qx];
            if (q.w > 0.0f) { r = r + q.x; g = g + q.y; b = b + q.z; m++; }
        }
        if (m) { const float fm = (float)m; v.x = r / fm; v.y = g / fm; v.z = b / fm; v.w = alpha; }
    }
    out[i] = v;
}

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t scanBytes(uint32_t entries)
{
    size_t tmp = 0;
    unsigned long long* none = nullptr;
    (void)rocprim::exclusive_scan(nullptr, tmp, none, none, 0ull, (size_t)entries, rocprim::plus<unsigned long long>(), (hipStream_t)0);
    return tmp;
}

} // namespace

extern "C" size_t bake_raster_scratch_bytes(uint32_t numTris, uint32_t W, uint32_t H)
{
    return round256(8ull * W * H) + 2 * round256(8ull * ((size_t)numTris + 1)) + round256(scanBytes(numTris + 1u)) + 256;
}

extern "C" hipError_t bake_launch_raster(hipStream_t stream, const BakeMesh* mesh, uint32_t W, uint32_t H, void* scratch, size_t scratchBytes,
    TbRadianceRay* rays, TbBakeTexel* texels, uint32_t* covered)
{
    if (!mesh || !W || !H || W > BAKE_MAX_SIDE || H > BAKE_MAX_SIDE || !scratch || !rays || !texels || !covered) return hipErrorInvalidValue;
    if (scratchBytes < bake_raster_scratch_bytes(mesh->numTris, W, H)) return hipErrorInvalidValue;
    const uint32_t n = W * H, T = mesh->numTris;
    uint8_t* at = (uint8_t*)scratch;
    auto take = [&](size_t bytes) { uint8_t* p = at; at += round256(bytes); return p; };
    unsigned long long* keys = (unsigned long long*)take(8ull * n);
    unsigned long long* counts = (unsigned long long*)take(8ull * ((size_t)T + 1));
    unsigned long long* first = (unsigned long long*)take(8ull * ((size_t)T + 1));
    size_t tmpBytes = scanBytes(T + 1u);
    void* tmp = take(tmpBytes);
    BAKE_TRY(hipMemsetAsync(keys, 0xff, 8ull * n, stream));
    BAKE_TRY(hipMemsetAsync(covered, 0, 4, stream));
    unsigned long long items = 0;
    if (T) {
        hipLaunchKernelGGL(bake_tiles, dim3(T / BLOCK + 1u), dim3(BLOCK), 0, stream, *mesh, W, H, counts);
        BAKE_TRY(rocprim::exclusive_scan(tmp, tmpBytes, counts, first, 0ull, (size_t)T + 1, rocprim::plus<unsigned long long>(), stream));
        BAKE_TRY(hipMemcpyAsync(&items, first + T, 8, hipMemcpyDeviceToHost, stream));
        BAKE_TRY(hipStreamSynchronize(stream));
    }
    const unsigned long long perLaunch = 1ull << 30; /* items of one launch: 2^28 workgroups */
    for (unsigned long long base = 0; base < items; base += perLaunch) {
        const unsigned long long end = base + perLaunch < items ? base + perLaunch : items;
        const uint32_t blocks = (uint32_t)((end - base + (BLOCK / 64) - 1) / (BLOCK / 64));
        hipLaunchKernelGGL(bake_cover, dim3(blocks), dim3(BLOCK), 0, stream, *mesh, W, H, (const unsigned long long*)first, base, end, keys);
    }
    hipLaunchKernelGGL(bake_texels, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, *mesh, W, H, (const unsigned long long*)keys, rays, texels, covered);
    return hipGetLastError();
}

extern "C" hipError_t bake_launch_resolve(hipStream_t stream, uint64_t n, const TbBakeTexel* texels, const TbFloat4* sums, TbFloat4* rgba)
{
    if (!n) return hipSuccess;
    if (n > (1ull << 26) || !texels || !sums || !rgba) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bake_resolve, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, (uint32_t)n, texels, sums, rgba);
    return hipGetLastError();
}

extern "C" hipError_t bake_launch_dilate(hipStream_t stream, uint32_t W, uint32_t H, uint32_t pass, const TbFloat4* in, TbFloat4* out)
{
    if (!W || !H || W > BAKE_MAX_SIDE || H > BAKE_MAX_SIDE || pass < 1 || pass > 16 || !in || !out || in == out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bake_dilate, dim3((W * H + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, W, H, ldexpf(1.0f, -(int)pass), in, out);
    return hipGetLastError();
}
