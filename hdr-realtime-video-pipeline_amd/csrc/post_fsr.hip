// post_fsr.hip -- hdrtv_post_rgb48_fsr (gfx950): quantise + FSR upscale of the RGB48 output in one kernel, the fused form of
// post_scale_tile.h with the reference's default display scaler in place of the Lanczos passes: EASU (edge-adaptive spatial
// upsampling, twelve taps, direction and length from four luma analyses) and, optionally, RCAS (contrast-adaptive sharpening with
// the denoise term) on the float32 EASU image.  include/hdrtv_mi355x.h states the rule, tests/rgb48_fsr_ref.py restates it in
// NumPy; the device is held to that bit for bit, so every float operation below is one rounded float32 operation: __fmul_rn /
// __fadd_rn / __fsub_rn / __fdiv_rn, no fused multiply-add (the file is built with -ffp-contract=off on top: hipcc's default
// contraction fuses in the backend), no fast reciprocal or root -- the rule's two approximations are integer subtractions on the
// bit pattern --, denormals kept.
//
// A workgroup of 256 lanes owns PS_TH x PS_TW = 32 x 64 output pixels:
//   1. stage   the source footprint of the tile -- with RCAS, of the tile and its one-pixel ring -- is read from HBM once, quantised
//              once (quant_rgb, plain or PQ) and kept as u16 codes `codes[ch][row][col]`: source rows fp(ya) - 1 .. fp(yb) + 2 for
//              the first and last output row ya, yb (clamped to the image), columns alike; indices outside the frame read the
//              clamped pixel, so the taps never clamp.  fp rises by at most one per output pixel (dH >= H, dW >= W), so the
//              footprint is at most 35 x 67 (37 x 69 with the ring).
//   2. EASU    RCAS off: a lane owns four neighbouring pixels of an output row (and of the row 16 below), computes them one after
//              the other, quantises and stores with post_rgb48_kernel's packing.  RCAS on: lanes walk the 34 x 66 pixels of tile +
//              ring in row-major order (a ring pixel outside the image holds the value at its clamped position) and write the
//              float32 results to `easu[ch][row][col]`.
//   3. RCAS    from `easu`: a lane owns the same four neighbouring pixels, reads their cross-shaped neighbourhoods (14 values per
//              channel), sharpens, quantises, stores.
// A sample is s = c / 65535 correctly rounded.  The kernel gets it without a division: q = c * r, e = fma(-q, 65535, c),
// s = fma(e, r, q) with r = float32(1 / 65535) -- one Newton step on the residual, which tests/test_rgb48_fsr_host.py shows equal to
// the correctly rounded quotient for every one of the 65536 codes (in exact arithmetic).  These two are the only fused operations
// in the file, and they are written as such.
// LDS: codes 3 x 35 x 68 x 2 = 14,280 bytes without RCAS; 3 x 37 x 70 x 2 + 3 x 34 x 66 x 4 = 15,540 + 26,928 = 42,468 bytes with
// it: three workgroups per CU either way.  Banks (MI355X_MICROARCH.md): in the row-major EASU walk the twelve u16 reads of a wave
// are 64 addresses that rise by at most one element per lane (same dword = broadcast), except where the walk wraps to the next
// row; its `easu` writes are consecutive dwords.  Where a lane owns four neighbouring pixels (RCAS's reads of `easu`, EASU's reads of
// `codes` without RCAS) the 16 lanes of a row step by four floats / two to four codes and two rows share a 32-lane group: two-way
// conflicts at worst, against some 700 vector instructions per EASU pixel.
// The kernel's body is post_fsr_body.h, included into the __global__ function below and into post_fsr_grain.hip's, which grains the
// final codes (hdrtv_post_rgb48_fsr_grain) and includes this file for the functions in front of the kernel.
#include "launchers.h"
#include "post_quant.h"
#include "film_grain.h"

namespace {

__device__ __forceinline__ float fm(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fa(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float fs(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float fd(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float sat(float a) { return fminf(fmaxf(a, 0.f), 1.f); }

// the rule's two low-precision functions: integer subtractions on the u32 pattern of the float32
__device__ __forceinline__ float aprx_rcp(float a) { return __uint_as_float(0x7ef07ebbu - __float_as_uint(a)); }
__device__ __forceinline__ float aprx_rsq(float a) { return __uint_as_float(0x5f347d74u - (__float_as_uint(a) >> 1)); }

// u16 code -> float32(c / 65535), correctly rounded for every code (see above)
__device__ __forceinline__ float fsr_sample(uint32_t c)
{
    constexpr float r = (float)(1.0 / 65535.0);
    const float x = (float)c;
    const float q = __fmul_rn(x, r);
    return __fmaf_rn(__fmaf_rn(-q, 65535.f, x), r, q);
}

// one of the four analyses: luma cross lA / lB lC lD / lE, bilinear weight w
__device__ __forceinline__ void fsr_set(float &dirx, float &diry, float &len, float w, float lA, float lB, float lC, float lD, float lE)
{
    const float dc = fs(lD, lC), cb = fs(lC, lB), dx = fs(lD, lB);
    float lenx = sat(fm(fabsf(dx), aprx_rcp(fmaxf(fabsf(dc), fabsf(cb)))));
    lenx = fm(lenx, lenx);
    const float ec = fs(lE, lC), ca = fs(lC, lA), dy = fs(lE, lA);
    float leny = sat(fm(fabsf(dy), aprx_rcp(fmaxf(fabsf(ec), fabsf(ca)))));
    leny = fm(leny, leny);
    dirx = fa(dirx, fm(dx, w));
    diry = fa(diry, fm(dy, w));
    len = fa(len, fa(fm(w, lenx), fm(w, leny)));
}

// the twelve taps b c / e f g h / i j k l / n o as offsets from f
enum { TB, TC, TE, TF, TG, TH, TI, TJ, TK, TL, TN, TO };
constexpr int FSR_OX[12] = {0, 1, -1, 0, 1, 2, -1, 0, 1, 2, 0, 1};
constexpr int FSR_OY[12] = {-1, -1, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2};
constexpr int FSR_ORDER[12] = {TB, TC, TI, TJ, TF, TE, TK, TL, TH, TG, TO, TN};      // the order the weights accumulate in

// EASU of one output pixel.  t = the code of tap (-1, -1) of channel 0: tap (ox, oy) of channel ch lies at
// t[ch * PLANE + (oy + 1) * PITCH + ox + 1]; ppx, ppy = the position inside the source pixel f.
template <int PITCH, int PLANE>
__device__ __forceinline__ void fsr_easu(const uint16_t *t, const float ppx, const float ppy, float (&out)[3])
{
    float s[12][3], l[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) s[k][ch] = fsr_sample(t[ch * PLANE + (FSR_OY[k] + 1) * PITCH + FSR_OX[k] + 1]);
        l[k] = fa(fa(fm(0.2126f, s[k][0]), fm(0.7152f, s[k][1])), fm(0.0722f, s[k][2]));
    }
    const float omx = fs(1.f, ppx), omy = fs(1.f, ppy);
    float dirx = 0.f, diry = 0.f, len = 0.f;
    fsr_set(dirx, diry, len, fm(omx, omy), l[TB], l[TE], l[TF], l[TG], l[TJ]);
    fsr_set(dirx, diry, len, fm(ppx, omy), l[TC], l[TF], l[TG], l[TH], l[TK]);
    fsr_set(dirx, diry, len, fm(omx, ppy), l[TF], l[TI], l[TJ], l[TK], l[TN]);
    fsr_set(dirx, diry, len, fm(ppx, ppy), l[TG], l[TJ], l[TK], l[TL], l[TO]);

    float dirr = fa(fm(dirx, dirx), fm(diry, diry));
    const bool zro = dirr < (1.f / 32768.f);
    dirr = zro ? 1.f : aprx_rsq(dirr);
    dirx = zro ? 1.f : dirx;
    dirx = fm(dirx, dirr);
    diry = fm(diry, dirr);
    len = fm(len, 0.5f);
    len = fm(len, len);
    const float stretch = fm(fa(fm(dirx, dirx), fm(diry, diry)), aprx_rcp(fmaxf(fabsf(dirx), fabsf(diry))));
    const float len2x = fa(1.f, fm(fs(stretch, 1.f), len)), len2y = fa(1.f, fm(-0.5f, len));
    const float lob = fa(0.5f, fm((float)((0.25 - 0.04) - 0.5), len));
    const float clp = aprx_rcp(lob);

    float ac[3] = {0.f, 0.f, 0.f}, aw = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const int k = FSR_ORDER[i];
        const float offx = fs((float)FSR_OX[k], ppx), offy = fs((float)FSR_OY[k], ppy);
        const float vx = fm(fa(fm(offx, dirx), fm(offy, diry)), len2x);
        const float vy = fm(fa(fm(offx, -diry), fm(offy, dirx)), len2y);
        const float d2 = fminf(fa(fm(vx, vx), fm(vy, vy)), clp);
        float wb = fa(fm(0.4f, d2), -1.f), wa = fa(fm(lob, d2), -1.f);
        wb = fm(wb, wb);
        wa = fm(wa, wa);
        wb = fa(fm(1.5625f, wb), -0.5625f);
        const float w = fm(wb, wa);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) ac[ch] = fa(ac[ch], fm(s[k][ch], w));
        aw = fa(aw, w);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float mn = fminf(fminf(s[TF][ch], fminf(s[TG][ch], s[TJ][ch])), s[TK][ch]);
        const float mx = fmaxf(fmaxf(s[TF][ch], fmaxf(s[TG][ch], s[TJ][ch])), s[TK][ch]);
        out[ch] = sat(fminf(fmaxf(fd(ac[ch], aw), mn), mx));
    }
}

// RCAS of one pixel e with the neighbours b (above) d (left) f (right) h (below); sharp = float32(2^-sharpness)
__device__ __forceinline__ void fsr_rcas(const float (&b)[3], const float (&d)[3], const float (&e)[3], const float (&f)[3],
                                         const float (&h)[3], const float sharp, float (&out)[3])
{
    float lobe[3], nz[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float mn1 = fminf(fminf(b[ch], fminf(d[ch], f[ch])), h[ch]), mx1 = fmaxf(fmaxf(b[ch], fmaxf(d[ch], f[ch])), h[ch]);
        const float lo = fminf(mn1, e[ch]), hi = fmaxf(mx1, e[ch]);
        const float hit_min = fd(lo, fmaxf(fm(4.f, mx1), 1e-6f));
        const float hit_max = fd(fs(1.f, hi), fminf(fs(fm(4.f, mn1), 4.f), -1e-6f));
        lobe[ch] = fm(fmaxf(-0.1875f, fminf(fmaxf(-hit_min, hit_max), 0.f)), sharp);
        nz[ch] = fd(fabsf(fs(fm(0.25f, fa(fa(fa(b[ch], d[ch]), f[ch]), h[ch])), e[ch])), fmaxf(fs(hi, lo), 1e-6f));
    }
    const float k = fa(fm(-0.5f, sat(fmaxf(nz[0], fmaxf(nz[1], nz[2])))), 1.f);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float lb = fm(lobe[ch], k);
        const float rcp = fd(1.f, fa(fm(4.f, lb), 1.f));
        out[ch] = sat(fm(fa(fa(fa(fa(fm(lb, b[ch]), fm(lb, d[ch])), fm(lb, h[ch])), fm(lb, f[ch])), e[ch]), rcp));
    }
}

// twelve codes of four neighbouring pixels, o[ch] = the codes of channel ch with pixel j in bits 16 j .. 16 j + 15: 24 bytes as three
// 8-byte stores where the address allows, code by code otherwise (post_scale_tile.h's store)
__device__ __forceinline__ void fsr_store(const PostFsrParams &p, int dy, int dx, const uint64_t (&o)[3])
{
    uint16_t *d = p.dst + ((size_t)dy * p.dW + dx) * 3;
    uint32_t c[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[ch][j] = (uint32_t)(o[ch] >> (16 * j)) & 0xffffu;
    }
    if (dx + 3 < p.dW && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
        uint2 *d2 = reinterpret_cast<uint2 *>(d);
        d2[0] = make_uint2(c[0][0] | (c[1][0] << 16), c[2][0] | (c[0][1] << 16));
        d2[1] = make_uint2(c[1][1] | (c[2][1] << 16), c[0][2] | (c[1][2] << 16));
        d2[2] = make_uint2(c[2][2] | (c[0][3] << 16), c[1][3] | (c[2][3] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (dx + j < p.dW) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) d[j * 3 + ch] = (uint16_t)c[ch][j];
            }
        }
    }
}

template <typename T, bool PQ, bool RCAS>
__global__ __launch_bounds__(256) void post_fsr_kernel(const PostFsrParams p, const float sharp)
{
    constexpr bool GRAIN = false;
    [[maybe_unused]] constexpr float intensity = 0.f, seed = 0.f;
#include "post_fsr_body.h"
}

}  // namespace

#ifndef POST_FSR_HELPERS_ONLY          // post_fsr_grain.hip includes this file for everything above and launches its own kernels
namespace {

template <typename T, bool PQ>
void launch(const PostFsrParams &p, int rcas, float sharp, dim3 g, hipStream_t s)
{
    if (rcas) hipLaunchKernelGGL((post_fsr_kernel<T, PQ, true>), g, dim3(256), 0, s, p, sharp);
    else hipLaunchKernelGGL((post_fsr_kernel<T, PQ, false>), g, dim3(256), 0, s, p, 0.f);
}

}  // namespace

hipError_t post_fsr_launch(const PostFsrParams &p, int rcas, float sharp, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || p.dH > 2 * (long long)p.H || p.dW > 2 * (long long)p.W || (pq && !p.pq_bnd) ||
        (rcas && !(sharp >= 0.25f && sharp <= 1.f)))
        return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH);
    if (is_f32) {
        if (pq) launch<float, true>(p, rcas, sharp, g, s);
        else launch<float, false>(p, rcas, sharp, g, s);
    } else {
        if (pq) launch<f16, true>(p, rcas, sharp, g, s);
        else launch<f16, false>(p, rcas, sharp, g, s);
    }
    return hipGetLastError();
}
#endif
