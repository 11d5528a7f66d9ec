// post_quant.h -- the pixel rule of the output kernels, "one pixel of the model's tensor -> three u16 codes" (quant_rgb, plain or
// PQ), shared by prepost.hip (post_rgb48 / post_pq_rgb48), post_scale.hip (the same codes, then the Lanczos upscale) and
// post_ycbcr.hip (the same codes, then the Y'CbCr matrix): one definition, so the scaled and the Y'CbCr entry points start from
// exactly the integers the unscaled one writes.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float clamp01(float v)
{
    // torch.clamp semantics incl. NaN propagation
    return v != v ? v : fminf(fmaxf(v, 0.f), 1.f);
}

__device__ __forceinline__ uint32_t quant_u16(float x)
{
    return (uint32_t)(int)__fadd_rn(__fmul_rn(clamp01(x), 65535.f), 0.5f) & 0xffff;
}

// Exact u16 code of a PQ level: code(y) = floor(pq(y) * 65535 + 0.5) with the OETF in double precision, as an integer
// function of the fp32 argument y.  bnd[v] (v = 1..65535) is the smallest fp32 y whose code is >= v (built on the host in
// double, hdrtv_api.hip pq_boundaries; 256 KiB, L2-resident); the fp32 evaluation lands within a few codes of the answer
// and two compares against the table settle it.  The result does not depend on any device math-library rounding.
// First guess without transcendental functions: lut[i] (appended to bnd at PQ_LUT_OFF) is the exact code at the fp32 value whose
// bit pattern is (PQ_LUT_BASE + i) << 17 -- 64 steps per binary octave from 2^-27 to 1, the curve's own near-logarithmic
// spacing -- and the code in between is interpolated on the low 17 mantissa bits (within 2 codes of the truth everywhere).
constexpr int PQ_LUT_BASE = (127 - 27) << 6, PQ_LUT_N = 27 * 64 + 2, PQ_LUT_OFF = 65536;
// pq_code_level: the code of a level y with 1.0 = 10000 nits, clamped to [0, 1] here (the oracle's orc_pq_code; post_tonemap.hip
// calls it on a scaled table entry).  pq_code: the code of a linear value with 1.0 = `peak` nits -- the same walk behind its scaling.
__device__ __forceinline__ uint32_t pq_code_level(float y, const float *__restrict__ bnd)
{
    y = fminf(fmaxf(y, 0.f), 1.f);
    const uint32_t bits = __float_as_uint(y);
    int c = 0;
    if ((int)(bits >> 17) >= PQ_LUT_BASE) {
        const int i = (int)(bits >> 17) - PQ_LUT_BASE;
        const int c0 = (int)bnd[PQ_LUT_OFF + i], c1 = (int)bnd[PQ_LUT_OFF + i + 1];
        c = c0 + (int)(((uint32_t)(c1 - c0) * (bits & 0x1ffffu)) >> 17);
    }
    while (c < 65535 && y >= bnd[c + 1]) ++c;
    while (c > 0 && y < bnd[c]) --c;
    return (uint32_t)c;
}
__device__ __forceinline__ uint32_t pq_code(float lin, float peak, const float *__restrict__ bnd)
{
    return pq_code_level(__fdiv_rn(__fmul_rn(lin, peak), 10000.f), bnd);
}
__device__ __forceinline__ float gamut_row(float m0, float m1, float m2, float r, float g, float b)
{
    return __fmaf_rn(m2, b, __fmaf_rn(m1, g, __fmul_rn(m0, r)));      // the oracle's rounding sequence
}

// One pixel (cr, cg, cb) of the model's output -> its three u16 codes.  PQ: ITU-R BT.2087 BT.709 -> BT.2020 (linear light), the
// [0, 1] clamp and the exact PQ code at `peak` nits; otherwise the plain rounding of the clamped value.
template <bool PQ>
__device__ __forceinline__ void quant_rgb(float cr, float cg, float cb, float peak, const float *__restrict__ bnd, uint32_t &q0,
                                          uint32_t &q1, uint32_t &q2)
{
    if (PQ) {
        const float xr = gamut_row(0.6274f, 0.3293f, 0.0433f, cr, cg, cb);
        const float xg = gamut_row(0.0691f, 0.9195f, 0.0114f, cr, cg, cb);
        const float xb = gamut_row(0.0164f, 0.0880f, 0.8956f, cr, cg, cb);
        q0 = pq_code(fminf(fmaxf(xr, 0.f), 1.f), peak, bnd);
        q1 = pq_code(fminf(fmaxf(xg, 0.f), 1.f), peak, bnd);
        q2 = pq_code(fminf(fmaxf(xb, 0.f), 1.f), peak, bnd);
    } else {
        q0 = quant_u16(cr);
        q1 = quant_u16(cg);
        q2 = quant_u16(cb);
    }
}

}  // namespace
