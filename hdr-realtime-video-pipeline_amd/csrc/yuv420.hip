// yuv420.hip -- 8-bit 4:2:0 Y'CbCr (I420, NV12) -> the frame the BGR entry points read, on the GPU (gfx950).
//
//  yuv420_to_bgr       planes -> u8 HWC BGR: 1.5 B in, 3 B out per pixel.  The first half of the letterboxed YUV route
//                      (hdrtv_letterbox_u8 reads its output) and the device oracle of the tests.
//  pre_unpack_yuv_f32  planes -> fp32 planar RGB, float(u8) * fp32(1/255): pre_unpack_f32 (fp32_ops.hip) of the converted frame,
//                      for the fp32 preset (cond_resize_f32 follows).
//
// The arithmetic is ycc_in.h's rule at 8 bits.  Both kernels work on pixel pairs (2i, 2i + 1) of one row (ycc_pair; the fp32 unpack
// is ycc_unpack_f32<8>, its body).  Plane reads are byte loads (no pointer or pitch is aligned);
// neighbouring lanes read neighbouring bytes, so each wave load still touches few cache lines.  Built, as every file here except
// fp32_ops.hip, without the SLP / loop vectorisers.
#include "ycc_in.h"

namespace {

// One lane = 8 consecutive pixels of the frame in raster order (four pairs; a group may span rows when W % 8 != 0).  A8: the
// destination is 8-byte aligned, and a full group's 24 bytes go out as three 8-byte stores.
template <bool A8>
__global__ __launch_bounds__(256) void yuv420_to_bgr_kernel(const Yuv420Src src, int H, int W, uint8_t *__restrict__ bgr)
{
    const size_t npix = (size_t)H * W, ngrp = (npix + 7) / 8;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += (size_t)gridDim.x * blockDim.x) {
        const size_t p0 = g * 8;
        int y = (int)(p0 / (size_t)W), x = (int)(p0 - (size_t)y * W);
        const int np = npix - p0 >= 8 ? 4 : (int)((npix - p0) / 2);      // pairs in this group
        uint32_t w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < np) {
                uint32_t r[2], gg[2], b[2];
                ycc_pair(src, H, W, y, x >> 1, r, gg, b);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int o = (2 * q + h) * 3;
                    w[o >> 2] |= b[h] << ((o & 3) * 8);
                    w[(o + 1) >> 2] |= gg[h] << (((o + 1) & 3) * 8);
                    w[(o + 2) >> 2] |= r[h] << (((o + 2) & 3) * 8);
                }
                x += 2;
                if (x == W) { x = 0; ++y; }
            }
        }
        uint8_t *d = bgr + p0 * 3;
        if (A8 && np == 4) {
            uint2 *d2 = reinterpret_cast<uint2 *>(d);
            d2[0] = make_uint2(w[0], w[1]);
            d2[1] = make_uint2(w[2], w[3]);
            d2[2] = make_uint2(w[4], w[5]);
        } else {
            for (int k = 0; k < 6 * np; ++k) d[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

__global__ __launch_bounds__(256) void pre_unpack_yuv_f32_kernel(const Yuv420Src src, int H, int W, float *__restrict__ out)
{
    ycc_unpack_f32(src, H, W, out);
}

}  // namespace

hipError_t yuv420_to_bgr_launch(const Yuv420Src &src, int H, int W, uint8_t *bgr, hipStream_t s)
{
    if (!ycc_ok(src, H, W) || !bgr) return hipErrorInvalidValue;
    const dim3 g(ycc_grid(((size_t)H * W + 7) / 8)), b(256);
    if (((uintptr_t)bgr & 7) == 0) hipLaunchKernelGGL(yuv420_to_bgr_kernel<true>, g, b, 0, s, src, H, W, bgr);
    else hipLaunchKernelGGL(yuv420_to_bgr_kernel<false>, g, b, 0, s, src, H, W, bgr);
    return hipGetLastError();
}

hipError_t pre_unpack_yuv_f32_launch(const Yuv420Src &src, int H, int W, float *rgb, hipStream_t s)
{
    if (!ycc_ok(src, H, W) || !rgb) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pre_unpack_yuv_f32_kernel, dim3(ycc_grid((size_t)H * W / 2)), dim3(256), 0, s, src, H, W, rgb);
    return hipGetLastError();
}
