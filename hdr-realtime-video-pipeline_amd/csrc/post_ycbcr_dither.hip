// post_ycbcr_dither.hip -- the 10-bit Y'CbCr conversions of post_ycbcr.hip with the ordered dither of include/hdrtv_mi355x.h
// (hdrtv_post_ycbcr10_ex / hdrtv_rgb48_to_ycbcr10_ex with dither = HDRTV_DITHER_ORDERED) on the device (gfx950).  The same tile code
// (post_ycbcr_tile.h: tile, lanes' jobs, LDS layout and bank reasoning as post_ycbcr.hip describes them) with MODE = YC_ORDERED: the
// rounding constant of every luma and chroma sample is (2 M + 1) scaled to the sample's shift, M the 16 x 16 Bayer index computed
// from the sample's own coordinates -- a bit reverse, two shifts and masks per nibble, no table and no memory access.
// The instances live in their own file, under their own names, so that post_ycbcr.hip keeps exactly the kernels it had.
#include "post_ycbcr_tile.h"

namespace {

template <typename T, bool PQ, int FMT>
__global__ __launch_bounds__(256) void post_ycc10_dither_kernel(Ycbcr10Params p)
{
    const TensorSrc<T, PQ> src{static_cast<const T *>(p.in), (size_t)p.H * p.W, p.W, p.peak, p.pq_bnd};
    ycbcr_tile<TensorSrc<T, PQ>, FMT, YC_ORDERED>(src, p);
}

template <int FMT>
__global__ __launch_bounds__(256) void rgb48_ycc10_dither_kernel(Ycbcr10Params p)
{
    const Rgb48Src src{static_cast<const uint16_t *>(p.in), p.W};
    ycbcr_tile<Rgb48Src, FMT, YC_ORDERED>(src, p);
}

template <typename T, bool PQ>
void launch_fmt(const Ycbcr10Params &p, dim3 g, hipStream_t s)
{
    if (p.fmt == HDRTV_YCC_P010) hipLaunchKernelGGL((post_ycc10_dither_kernel<T, PQ, HDRTV_YCC_P010>), g, dim3(256), 0, s, p);
    else if (p.fmt == HDRTV_YCC_YUV420P10) hipLaunchKernelGGL((post_ycc10_dither_kernel<T, PQ, HDRTV_YCC_YUV420P10>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((post_ycc10_dither_kernel<T, PQ, HDRTV_YCC_YUV422P10>), g, dim3(256), 0, s, p);
}

}  // namespace

// the argument rules of post_ycbcr10_launch / rgb48_to_ycbcr10_launch
hipError_t post_ycbcr10_dither_launch(const Ycbcr10Params &p, int is_f32, int pq, hipStream_t s)
{
    if (!ycbcr_params_ok(p) || (pq && !p.pq_bnd)) return hipErrorInvalidValue;
    const dim3 g((p.W + YC_TW - 1) / YC_TW, (p.H + YC_TH - 1) / YC_TH);
    if (is_f32) {
        if (pq) launch_fmt<float, true>(p, g, s);
        else launch_fmt<float, false>(p, g, s);
    } else {
        if (pq) launch_fmt<f16, true>(p, g, s);
        else launch_fmt<f16, false>(p, g, s);
    }
    return hipGetLastError();
}

hipError_t rgb48_to_ycbcr10_dither_launch(const Ycbcr10Params &p, hipStream_t s)
{
    if (!ycbcr_params_ok(p)) return hipErrorInvalidValue;
    const dim3 g((p.W + YC_TW - 1) / YC_TW, (p.H + YC_TH - 1) / YC_TH);
    if (p.fmt == HDRTV_YCC_P010) hipLaunchKernelGGL((rgb48_ycc10_dither_kernel<HDRTV_YCC_P010>), g, dim3(256), 0, s, p);
    else if (p.fmt == HDRTV_YCC_YUV420P10) hipLaunchKernelGGL((rgb48_ycc10_dither_kernel<HDRTV_YCC_YUV420P10>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((rgb48_ycc10_dither_kernel<HDRTV_YCC_YUV422P10>), g, dim3(256), 0, s, p);
    return hipGetLastError();
}
