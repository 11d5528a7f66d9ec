// ycbcr10_in.hip -- 10-bit Y'CbCr (P010, yuv420p10le, yuv422p10le) -> RGB on the GPU (gfx950), the stand-alone kernels.
//
//  ycbcr10_to_rgb10       planes -> u16 HWC R, G, B codes 0..1023: the rule on its own, the anchor the fused staging step of pre_fused
//                         (prepost.hip) and the fp32 unpack below are held to by the tests.
//  pre_unpack_ycbcr10_f32 planes -> fp32 planar RGB, float(code) * fp32(1/1023), for the fp32 preset (cond_resize_f32 follows).
//
// The arithmetic is ycc_in.h's rule at 10 bits.  Both kernels work on pixel pairs (2i, 2i + 1) of one row (ycc_pair; the fp32 unpack is
// ycc_unpack_f32<10>, its body).  Plane reads are u16 loads (pointers and pitches are two-byte aligned, no more); neighbouring lanes read
// neighbouring samples.  Built, as every file here except fp32_ops.hip, without the SLP / loop vectorisers.
#include "ycc_in.h"

namespace {

// One lane = one pair = six u16 = 12 bytes of the destination.  A4: the destination is 4-byte aligned, and the pair goes out as three
// dword stores.
template <bool A4>
__global__ __launch_bounds__(256) void ycbcr10_to_rgb10_kernel(const Ycc10Src src, int H, int W, uint16_t *__restrict__ rgb)
{
    const size_t npair = (size_t)H * W / 2;
    const int Wc = W >> 1;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < npair; t += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / (size_t)Wc), i = (int)(t - (size_t)y * Wc);
        uint32_t r[2], g[2], b[2];
        ycc_pair(src, H, W, y, i, r, g, b);
        uint16_t *d = rgb + t * 6;
        if (A4) {
            uint32_t *d2 = reinterpret_cast<uint32_t *>(d);
            d2[0] = r[0] | (g[0] << 16);
            d2[1] = b[0] | (r[1] << 16);
            d2[2] = g[1] | (b[1] << 16);
        } else {
            d[0] = (uint16_t)r[0]; d[1] = (uint16_t)g[0]; d[2] = (uint16_t)b[0];
            d[3] = (uint16_t)r[1]; d[4] = (uint16_t)g[1]; d[5] = (uint16_t)b[1];
        }
    }
}

__global__ __launch_bounds__(256) void pre_unpack_ycbcr10_f32_kernel(const Ycc10Src src, int H, int W, float *__restrict__ out)
{
    ycc_unpack_f32(src, H, W, out);
}

}  // namespace

hipError_t ycbcr10_to_rgb10_launch(const Ycc10Src &src, int H, int W, uint16_t *rgb, hipStream_t s)
{
    if (!ycc_ok(src, H, W) || !rgb) return hipErrorInvalidValue;
    const dim3 g(ycc_grid((size_t)H * W / 2)), b(256);
    if (((uintptr_t)rgb & 3) == 0) hipLaunchKernelGGL(ycbcr10_to_rgb10_kernel<true>, g, b, 0, s, src, H, W, rgb);
    else hipLaunchKernelGGL(ycbcr10_to_rgb10_kernel<false>, g, b, 0, s, src, H, W, rgb);
    return hipGetLastError();
}

hipError_t pre_unpack_ycbcr10_f32_launch(const Ycc10Src &src, int H, int W, float *rgb, hipStream_t s)
{
    if (!ycc_ok(src, H, W) || !rgb) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pre_unpack_ycbcr10_f32_kernel, dim3(ycc_grid((size_t)H * W / 2)), dim3(256), 0, s, src, H, W, rgb);
    return hipGetLastError();
}
