// film_grain.h -- the pixel rule of the film grain (gfx950), "position and seed -> the grain value g" and "u16 code and I * g -> the
// grained u16 code", shared by film_grain.hip (codes -> codes, and tensor -> quant_rgb -> grain in one launch), post_scale_grain.hip
// (the Lanczos tile with the staged codes grained) and post_fsr_grain.hip (the FSR tile with the final codes grained): one
// definition, so that every fused form writes exactly the integers of its twin followed by hdrtv_rgb48_film_grain.
// include/hdrtv_mi355x.h states the rule, tests/film_grain_ref.py restates it in NumPy; the device is held to that bit for bit, so
// every float operation below is one rounded float32 operation -- __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn and floorf, no
// fused multiply-add (the files that include this are built with -ffp-contract=off on top: hipcc's default contraction fuses in
// the backend), no reciprocal-multiply for a division.  No intermediate of the rule is denormal and den >= 0.011, so the
// denormal mode does not enter.  g is computed once per pixel: the three channels of a pixel take the same I * g.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float fg_fract(float v) { return __fsub_rn(v, floorf(v)); }

// permute(v) = fract(((34 v + 1) v) / 289) * 289
__device__ __forceinline__ float fg_permute(float v)
{
    const float t = __fmul_rn(__fadd_rn(__fmul_rn(34.f, v), 1.f), v);
    return __fmul_rn(fg_fract(__fdiv_rn(t, 289.f)), 289.f);
}

// The rule splits by what each part depends on, so that a kernel that walks a column or a row computes the shared part once:
//   grain_col(x, W) = permute(mx), grain_row(y, H) = my, grain_at(col, row, seed) = g.  Two of the rule's five divisions lie in grain_col.
__device__ __forceinline__ float grain_col(int x, int W)
{
    const float px = __fdiv_rn(__fadd_rn((float)x, 0.5f), (float)W);
    return fg_permute(__fadd_rn(px, 1.f));
}

__device__ __forceinline__ float grain_row(int y, int H)
{
    const float py = __fdiv_rn(__fadd_rn((float)y, 0.5f), (float)H);
    return __fadd_rn(py, 1.f);
}

__device__ __forceinline__ float grain_at(float col, float row, float seed)
{
    const float mz = __fadd_rn(seed, 1.f);
    float state = __fadd_rn(fg_permute(__fadd_rn(col, row)), mz);
    state = fg_permute(state);
    const float rnd = fg_fract(__fdiv_rn(state, 41.f));
    const float p = __fadd_rn(__fmul_rn(0.95f, rnd), 0.025f);
    const float q = __fsub_rn(p, 0.5f);
    const float r = __fmul_rn(q, q);
    // the shader's rational approximation of the inverse normal distribution, each constant rounded once to float32
    const float num = __fadd_rn(__fmul_rn(-0.5303572634357367f, r), 0.151015505647689f);
    const float den = __fadd_rn(__fadd_rn(__fmul_rn(r, r), __fmul_rn(-0.7607324991323768f, r)), 0.132089632343748f);
    const float g = __fmul_rn(q, __fadd_rn(1.365020122861334f, __fdiv_rn(num, den)));
    return __fmul_rn(g, 0.255121822830526f);
}

// g of grain position (x, y) of a W x H frame for the per-frame seed in [0, 1): |g| <= 0.50000006
__device__ __forceinline__ float grain_value(int x, int y, int W, int H, float seed)
{
    return grain_at(grain_col(x, W), grain_row(y, H), seed);
}

// the grained code of the u16 code c: s = c / 65535, v = sat(s + Ig), G = (int)(v * 65535 + 0.5) -- quant_u16's rounding.  s is the
// correctly rounded quotient without a division: q = c * r, e = fma(-q, 65535, c), s = fma(e, r, q) with r = float32(1 / 65535), one
// Newton step on the residual, equal to float32(c) / 65535 for every one of the 65536 codes (post_fsr.hip's sample, which
// tests/test_rgb48_fsr_host.py shows in exact arithmetic; tests/test_gpu_film_grain.py runs every code through it).  These two are
// the only fused operations of the rule's code, and they are written as such.
__device__ __forceinline__ uint32_t grain_code(uint32_t c, float Ig)
{
    constexpr float r = (float)(1.0 / 65535.0);
    const float x = (float)c;
    const float q = __fmul_rn(x, r);
    const float s = __fmaf_rn(__fmaf_rn(-q, 65535.f, x), r, q);
    const float v = fminf(fmaxf(__fadd_rn(s, Ig), 0.f), 1.f);
    return (uint32_t)(int)__fadd_rn(__fmul_rn(v, 65535.f), 0.5f);
}

// I * g of a position: what grain_code takes for each of the pixel's three codes
__device__ __forceinline__ float grain_term(float intensity, int x, int y, int W, int H, float seed)
{
    return __fmul_rn(intensity, grain_value(x, y, W, H, seed));
}

}  // namespace
