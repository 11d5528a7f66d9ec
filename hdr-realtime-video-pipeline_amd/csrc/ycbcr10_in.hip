// ycbcr10_in.hip -- 10-bit Y'CbCr (P010, yuv420p10le, yuv422p10le) -> RGB on the GPU (gfx950), the stand-alone kernels.
//
//  ycbcr10_to_rgb10       planes -> u16 HWC R, G, B codes 0..1023: the rule on its own, the anchor the fused staging step of pre_fused
//                         (prepost.hip) and the fp32 unpack below are held to by the tests.
//  pre_unpack_ycbcr10_f32 planes -> fp32 planar RGB, float(code) * fp32(1/1023), for the fp32 preset (cond_resize_f32 follows).
//
// The arithmetic is ycbcr10_in.h's rule.  Both kernels work on pixel pairs (2i, 2i + 1) of one row, as yuv420.hip: the pair shares its
// chroma column i.  Plane reads are u16 loads (pointers and pitches are two-byte aligned, no more); neighbouring lanes read
// neighbouring samples.  Built, as every file here except fp32_ops.hip, without the SLP / loop vectorisers.
#include "launchers.h"
#include "ycbcr10_in.h"

namespace {

__device__ __forceinline__ const uint16_t *row_of(const uint16_t *p, int row, int pitch_bytes)
{
    return reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(p) + (size_t)row * pitch_bytes);
}

// ten-bit R, G, B of the two pixels of pair i (luma columns 2i, 2i + 1) of row y
__device__ __forceinline__ void ycc10_pair(const Ycc10Src &s, int H, int W, int y, int i, uint32_t (&r)[2], uint32_t (&g)[2],
                                           uint32_t (&b)[2])
{
    const int Wc = W >> 1, i2 = min(i + 1, Wc - 1);
    int j = y, n = y;                                     // 4:2:2: 3 C[y] + C[y] = 4 C[y]
    if (s.fmt != YCC10_YUV422P10) {
        const int Hc = H >> 1;
        j = y >> 1;
        n = (y & 1) ? min(j + 1, Hc - 1) : max(j - 1, 0);
    }
    const int sh = s.fmt == YCC10_P010 ? 6 : 0;
    const uint16_t *yr = row_of(s.y, y, s.y_pitch) + 2 * i;
    int u4a, u4b, v4a, v4b;
    if (s.fmt == YCC10_P010) {
        const uint16_t *cj = row_of(s.u, j, s.c_pitch), *cn = row_of(s.u, n, s.c_pitch);
        u4a = 3 * ycc10_sample(cj[2 * i], sh) + ycc10_sample(cn[2 * i], sh);
        v4a = 3 * ycc10_sample(cj[2 * i + 1], sh) + ycc10_sample(cn[2 * i + 1], sh);
        u4b = 3 * ycc10_sample(cj[2 * i2], sh) + ycc10_sample(cn[2 * i2], sh);
        v4b = 3 * ycc10_sample(cj[2 * i2 + 1], sh) + ycc10_sample(cn[2 * i2 + 1], sh);
    } else {
        const uint16_t *uj = row_of(s.u, j, s.c_pitch), *un = row_of(s.u, n, s.c_pitch);
        const uint16_t *vj = row_of(s.v, j, s.c_pitch), *vn = row_of(s.v, n, s.c_pitch);
        u4a = 3 * ycc10_sample(uj[i], sh) + ycc10_sample(un[i], sh);
        v4a = 3 * ycc10_sample(vj[i], sh) + ycc10_sample(vn[i], sh);
        u4b = 3 * ycc10_sample(uj[i2], sh) + ycc10_sample(un[i2], sh);
        v4b = 3 * ycc10_sample(vj[i2], sh) + ycc10_sample(vn[i2], sh);
    }
    ycc10_rule(ycc10_sample(yr[0], sh), 2 * u4a, 2 * v4a, s.k, r[0], g[0], b[0]);
    ycc10_rule(ycc10_sample(yr[1], sh), u4a + u4b, v4a + v4b, s.k, r[1], g[1], b[1]);
}

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
        ycc10_pair(src, H, W, y, i, r, g, b);
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
    const float k1023 = (float)(1.0 / 1023.0);
    const size_t npix = (size_t)H * W, npair = npix / 2;
    const int Wc = W >> 1;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < npair; t += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / (size_t)Wc), i = (int)(t - (size_t)y * Wc);
        uint32_t r[2], g[2], b[2];
        ycc10_pair(src, H, W, y, i, r, g, b);
        const size_t o = (size_t)y * W + 2 * i;
        out[o] = __fmul_rn((float)r[0], k1023);
        out[o + 1] = __fmul_rn((float)r[1], k1023);
        out[npix + o] = __fmul_rn((float)g[0], k1023);
        out[npix + o + 1] = __fmul_rn((float)g[1], k1023);
        out[2 * npix + o] = __fmul_rn((float)b[0], k1023);
        out[2 * npix + o + 1] = __fmul_rn((float)b[1], k1023);
    }
}

inline int ycc10_grid(size_t n)
{
    size_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;   // 256 CUs x 8 blocks, grid-stride beyond (as yuv420.hip's yuv_grid)
    return (int)(g < 1 ? 1 : g);
}

bool ycc10_ok(const Ycc10Src &s, int H, int W)
{
    return ycc10_check(s.y, s.y_pitch, s.u, s.v, s.c_pitch, s.fmt, H, W) == nullptr;
}

}  // namespace

hipError_t ycbcr10_to_rgb10_launch(const Ycc10Src &src, int H, int W, uint16_t *rgb, hipStream_t s)
{
    if (!ycc10_ok(src, H, W) || !rgb) return hipErrorInvalidValue;
    const dim3 g(ycc10_grid((size_t)H * W / 2)), b(256);
    if (((uintptr_t)rgb & 3) == 0) hipLaunchKernelGGL(ycbcr10_to_rgb10_kernel<true>, g, b, 0, s, src, H, W, rgb);
    else hipLaunchKernelGGL(ycbcr10_to_rgb10_kernel<false>, g, b, 0, s, src, H, W, rgb);
    return hipGetLastError();
}

hipError_t pre_unpack_ycbcr10_f32_launch(const Ycc10Src &src, int H, int W, float *rgb, hipStream_t s)
{
    if (!ycc10_ok(src, H, W) || !rgb) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pre_unpack_ycbcr10_f32_kernel, dim3(ycc10_grid((size_t)H * W / 2)), dim3(256), 0, s, src, H, W, rgb);
    return hipGetLastError();
}
