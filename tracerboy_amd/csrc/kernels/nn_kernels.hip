/* nn_kernels.hip -- what the neural networks run besides their convolution (nn_convk_kernels.hip); launchers in nn_launch.h:
 *   nn_maxpool2x2_kernel     2 x 2 max-pool, stride 2, on the rounded values: the still denoiser's U-Net
 *   nn_pack_input_kernel     three RGBA32F surfaces -> a network's zero-extended NHWC binary16 input (the U-Net and the super-resolution)
 *   nn_unpack_output_kernel  the U-Net's 3-channel result -> RGBA32F (r, g, b, 1), cropped
 *   nn_resolve_aux_kernel    the guide sums -> the albedo and normals the U-Net reads
 *   nn_to_rgba8_kernel       the output stage's 8-bit store (both stages)
 * No lane reads or writes outside a tensor's padded extent. */
#include "nn_launch.h"
#include "tb_math.h"

#define NN_THREADS 256u

namespace {

typedef _Float16 nn_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 nn_half4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ _Float16 nn_max(_Float16 a, _Float16 b) { return (a > b || a != a) ? a : b; } /* a NaN on either side wins */

__global__ __launch_bounds__(NN_THREADS) void nn_maxpool2x2_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, uint32_t width, uint32_t channels,
    uint64_t items /* output pixels * channels / 8 */)
{
    const uint64_t i = (uint64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= items) return;
    const uint32_t groups = channels / 8u, g = (uint32_t)(i % groups), ow = width / 2u;
    const uint64_t pixel = i / groups; const uint32_t ox = (uint32_t)(pixel % ow); const uint64_t oy = pixel / ow;
    const uint16_t* s = in + ((oy * 2u) * width + ox * 2u) * channels + g * 8u;
    const size_t row = (size_t)width * channels;
    const nn_half8 a = *(const nn_half8*)s, b = *(const nn_half8*)(s + channels), c = *(const nn_half8*)(s + row), d = *(const nn_half8*)(s + row + channels);
    nn_half8 m;
    for (int j = 0; j < 8; j++) m[j] = nn_max(nn_max(a[j], b[j]), nn_max(c[j], d[j]));
    *(nn_half8*)(out + pixel * channels + g * 8u) = m;
}

/* post_kernels.hip's R8G8B8A8_UNORM store of one channel: clamp (NaN -> 0), scale, + 0.5, truncate */
__device__ __forceinline__ uint32_t nn_unorm8(float x) { return (uint32_t)(tb_saturate(x) * 255.0f + 0.5f); }

/* a lane writes 8 channels of one pixel: group 0 = channels 0-7, group 1 = channel 8 and zeros, groups 2 and 3 zeros.  unormColor: the colour goes
 * through the 8-bit store and back, k / 255 in fp32, before its one rounding to binary16 -- what a network reads from an R8G8B8A8_UNORM picture */
__global__ __launch_bounds__(NN_THREADS) void nn_pack_input_kernel(const TbFloat4* __restrict__ color, const TbFloat4* __restrict__ albedo,
    const TbFloat4* __restrict__ normal, uint16_t* __restrict__ out, uint32_t width, uint32_t height, uint32_t paddedW, uint32_t items, uint32_t unormColor)
{
    const uint32_t i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= items) return;
    const uint32_t g = i & 3u, pixel = i >> 2, x = pixel % paddedW, y = pixel / paddedW;
    nn_half8 h = {0, 0, 0, 0, 0, 0, 0, 0};
    if (x < width && y < height && g < 2u) {
        const size_t s = (size_t)y * width + x;
        if (g == 0u) {
            TbFloat4 c = color[s];
            if (unormColor) { c.x = (float)nn_unorm8(c.x) / 255.0f; c.y = (float)nn_unorm8(c.y) / 255.0f; c.z = (float)nn_unorm8(c.z) / 255.0f; }
            h[0] = (_Float16)c.x; h[1] = (_Float16)c.y; h[2] = (_Float16)c.z;
            if (albedo) { const TbFloat4 a = albedo[s], n = normal[s]; h[3] = (_Float16)a.x; h[4] = (_Float16)a.y; h[5] = (_Float16)a.z; h[6] = (_Float16)n.x; h[7] = (_Float16)n.y; }
        } else if (albedo) h[0] = (_Float16)normal[s].z;
    }
    *(nn_half8*)(out + (size_t)i * 8u) = h;
}

__global__ __launch_bounds__(NN_THREADS) void nn_unpack_output_kernel(const uint16_t* __restrict__ in, TbFloat4* __restrict__ out, uint32_t width, uint32_t paddedW,
    uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const uint32_t x = i % width, y = i / width;
    const nn_half4 h = *(const nn_half4*)(in + ((size_t)y * paddedW + x) * 32u);
    out[i] = TbFloat4{(float)h[0], (float)h[1], (float)h[2], 1.0f};
}

__global__ __launch_bounds__(NN_THREADS) void nn_resolve_aux_kernel(const TbFloat4* __restrict__ gAlbedo, const TbFloat4* __restrict__ gNormal,
    TbFloat4* __restrict__ albedo, TbFloat4* __restrict__ normal, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const TbFloat4 a = gAlbedo[i], n = gNormal[i];
    albedo[i] = TbFloat4{a.x / a.w, a.y / a.w, a.z / a.w, 1.0f};
    const float hits = n.w; /* as dn_resolve_guides_kernel (dn_kernels.hip) resolves the filter's normals */
    TbFloat4 on{0.0f, 0.0f, 0.0f, 1.0f};
    if (hits > 0.0f) { on.x = n.x / hits; on.y = n.y / hits; on.z = n.z / hits; }
    if (hits > 1.0f) {
        const float l = tb_sqrt((on.x * on.x + on.y * on.y) + on.z * on.z);
        if (l > 0.0f) { on.x = on.x / l; on.y = on.y / l; on.z = on.z / l; } else { on.x = 0.0f; on.y = 0.0f; on.z = 0.0f; }
    }
    normal[i] = on;
}

__global__ __launch_bounds__(NN_THREADS) void nn_to_rgba8_kernel(const TbFloat4* __restrict__ in, uint32_t* __restrict__ out, uint32_t nPixels)
{
    const uint32_t i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= nPixels) return;
    const TbFloat4 o = in[i]; /* post_kernels.hip's R8G8B8A8_UNORM store */
    const uint32_t r = nn_unorm8(o.x), g = nn_unorm8(o.y), b = nn_unorm8(o.z);
    out[i] = r | (g << 8) | (b << 16) | 0xff000000u;
}

uint32_t nn_groups(uint64_t items) { return (uint32_t)((items + NN_THREADS - 1u) / NN_THREADS); }

} // namespace

extern "C" hipError_t nn_launch_maxpool2x2(hipStream_t stream, uint32_t width, uint32_t height, uint32_t channels, const uint16_t* in, uint16_t* out)
{
    if (!nn_frame(width, height) || ((width | height) & 1u) || !channels || channels % 32u || channels > 512u || !nn_tensor(in) || !nn_tensor(out) || in == out)
        return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)(width / 2u) * (height / 2u) * (channels / 8u);
    hipLaunchKernelGGL(nn_maxpool2x2_kernel, dim3(nn_groups(items)), dim3(NN_THREADS), 0, stream, in, out, width, channels, items);
    return hipGetLastError();
}

extern "C" hipError_t nn_launch_pack_input(hipStream_t stream, uint32_t width, uint32_t height, uint32_t paddedW, uint32_t paddedH, const TbFloat4* color,
    const TbFloat4* albedo, const TbFloat4* normal, uint32_t unormColor, uint16_t* out)
{
    if (!nn_frame(width, height) || paddedW < width || paddedH < height || !nn_frame(paddedW, paddedH) || !nn_tensor(color) || !nn_tensor(out))
        return hipErrorInvalidValue;
    if ((albedo != nullptr) != (normal != nullptr) || (albedo && (!nn_tensor(albedo) || !nn_tensor(normal)))) return hipErrorInvalidValue;
    const uint32_t items = paddedW * paddedH * 4u; /* <= 2^26 */
    hipLaunchKernelGGL(nn_pack_input_kernel, dim3(nn_groups(items)), dim3(NN_THREADS), 0, stream, color, albedo, normal, out, width, height, paddedW, items, unormColor ? 1u : 0u);
    return hipGetLastError();
}

extern "C" hipError_t nn_launch_unpack_output(hipStream_t stream, uint32_t width, uint32_t height, uint32_t paddedW, const uint16_t* in, TbFloat4* out)
{
    if (!nn_frame(width, height) || paddedW < width || !nn_tensor(in) || !nn_tensor(out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_unpack_output_kernel, dim3(nn_groups((uint64_t)width * height)), dim3(NN_THREADS), 0, stream, in, out, width, paddedW, width * height);
    return hipGetLastError();
}

extern "C" hipError_t nn_launch_resolve_aux(hipStream_t stream, uint32_t width, uint32_t height, const TbFloat4* gAlbedo, const TbFloat4* gNormal, TbFloat4* albedo,
    TbFloat4* normal)
{
    if (!nn_frame(width, height) || !nn_tensor(gAlbedo) || !nn_tensor(gNormal) || !nn_tensor(albedo) || !nn_tensor(normal)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_resolve_aux_kernel, dim3(nn_groups((uint64_t)width * height)), dim3(NN_THREADS), 0, stream, gAlbedo, gNormal, albedo, normal, width * height);
    return hipGetLastError();
}

extern "C" hipError_t nn_launch_to_rgba8(hipStream_t stream, uint32_t width, uint32_t height, const TbFloat4* in, uint32_t* out)
{
    if (!nn_frame(width, height) || !nn_tensor(in) || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_to_rgba8_kernel, dim3(nn_groups((uint64_t)width * height)), dim3(NN_THREADS), 0, stream, in, out, width * height);
    return hipGetLastError();
}
