// post_ycbcr.hip -- 10-bit limited-range BT.2020nc Y'CbCr (P010, yuv420p10le, yuv422p10le) on the device (gfx950): what an encoder
// takes (hdrtv_post_ycbcr10 / hdrtv_rgb48_to_ycbcr10; include/hdrtv_mi355x.h states the integer rule).  The fused kernel goes from the
// model's planar f16 / f32 tensor straight to the planes: post_rgb48 + a conversion kernel would write and re-read 6 bytes per
// pixel for a 3-byte result.  The second kernel applies the same rule to RGB48 codes already in device memory (a scaled frame).
//
// A workgroup of 256 lanes owns YC_TH x YC_TW = 16 x 128 luma pixels:
//   1. stage   a lane takes eight neighbouring pixels of a row: one 16-byte load per plane (f16; two for f32; three for RGB48
//              codes), each pixel quantised ONCE with post_quant.h's quantisers (plain or PQ), its luma computed from the registers and
//              written as one 16-byte store, its codes kept as u16 `codes[ch][row][col]` (one 16-byte LDS store per plane).  The
//              chroma taps reach one column left of the tile (2i - 1) and, with top-left siting, one row above it (2j - 1): wave 2
//              stages that column, wave 1 that row (frame-edge indices clamped here, so step 2 never clamps).  W even and H even
//              (4:2:0) keep every other tap inside the tile and the frame.
//   2. chroma  a lane owns four neighbouring chroma samples: per plane and tap row one u16 (the column left of its group) and one
//              16-byte LDS read, the vertical weights, then 1 2 1 across -- sums of codes, at most 16 x 65535 -- and the matrix once
//              per sample in int64 (the rule is linear, so sum(w * u) = UR * sum(w * R) + ...).  P010: eight u16 Cb Cr Cb Cr ..
//              as one 16-byte store; planar: 8 bytes to each plane.  4:2:0 has 8 x 16 such groups per tile (half the lanes),
//              4:2:2 16 x 16.
// A group whose global address is not aligned to its access (odd pitches / plane starts in units of 16 bytes, W not a multiple of 8)
// or that crosses the right edge loads and stores its valid elements one by one.
// LDS banks (MI355X_MICROARCH.md): rows are 272 bytes = 68 dwords apart; a ds_write_b128 group of 8 lanes covers 128 contiguous
// bytes of one row, a ds_read_b128 group of 16 lanes whole 256-byte rows or two half rows 8 (4:2:0: 16) dwords apart in bank.
// 3 x 17 x 136 u16 = 13.5 KiB of LDS; the 32 waves of a CU (eight workgroups) fit while a kernel stays within 64 VGPRs.
// The tile code itself lives in post_ycbcr_tile.h, which post_ycbcr_dither.hip instantiates with the ordered dither.
#include "post_ycbcr_tile.h"

namespace {

template <typename T, bool PQ, int FMT>
__global__ __launch_bounds__(256) void post_ycbcr10_kernel(Ycbcr10Params p)
{
    const TensorSrc<T, PQ> src{static_cast<const T *>(p.in), (size_t)p.H * p.W, p.W, p.peak, p.pq_bnd};
    ycbcr_tile<TensorSrc<T, PQ>, FMT, YC_ROUND>(src, p);
}

template <int FMT>
__global__ __launch_bounds__(256) void rgb48_ycbcr10_kernel(Ycbcr10Params p)
{
    const Rgb48Src src{static_cast<const uint16_t *>(p.in), p.W};
    ycbcr_tile<Rgb48Src, FMT, YC_ROUND>(src, p);
}

template <typename T, bool PQ>
void launch_fmt(const Ycbcr10Params &p, dim3 g, hipStream_t s)
{
    if (p.fmt == HDRTV_YCC_P010) hipLaunchKernelGGL((post_ycbcr10_kernel<T, PQ, HDRTV_YCC_P010>), g, dim3(256), 0, s, p);
    else if (p.fmt == HDRTV_YCC_YUV420P10) hipLaunchKernelGGL((post_ycbcr10_kernel<T, PQ, HDRTV_YCC_YUV420P10>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((post_ycbcr10_kernel<T, PQ, HDRTV_YCC_YUV422P10>), g, dim3(256), 0, s, p);
}

}  // namespace

// pitches in u16 elements.  The bounds every store rests on (W even, H even for 4:2:0, pitches >= the row) are checked here too.
hipError_t post_ycbcr10_launch(const Ycbcr10Params &p, int is_f32, int pq, hipStream_t s)
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

hipError_t rgb48_to_ycbcr10_launch(const Ycbcr10Params &p, hipStream_t s)
{
    if (!ycbcr_params_ok(p)) return hipErrorInvalidValue;
    const dim3 g((p.W + YC_TW - 1) / YC_TW, (p.H + YC_TH - 1) / YC_TH);
    if (p.fmt == HDRTV_YCC_P010) hipLaunchKernelGGL((rgb48_ycbcr10_kernel<HDRTV_YCC_P010>), g, dim3(256), 0, s, p);
    else if (p.fmt == HDRTV_YCC_YUV420P10) hipLaunchKernelGGL((rgb48_ycbcr10_kernel<HDRTV_YCC_YUV420P10>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((rgb48_ycbcr10_kernel<HDRTV_YCC_YUV422P10>), g, dim3(256), 0, s, p);
    return hipGetLastError();
}
