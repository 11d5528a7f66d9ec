// ycbcr10_in.h -- 10-bit Y'CbCr input (P010, yuv420p10le, yuv422p10le): the conversion rule include/hdrtv_mi355x.h states, as one
// device helper, and the launchers of the kernels that apply it (ycbcr10_in.hip; pre_fused's 10-bit instantiation in prepost.hip).
//
// The rule is yuv420.h's at ten bits.  Samples are little-endian u16: P010 carries the value in the high ten bits (v = word >> 6),
// the planar layouts in the low ten (v = word & 0x3ff).  Per luma pixel (x, y) of an H x W frame (W even; H even for 4:2:0), chroma
// planes Hc rows (H / 2, or H for 4:2:2) by Wc = W / 2 samples:
//   vertical   4:2:0: j = y >> 1, n = y odd ? min(j + 1, Hc - 1) : max(j - 1, 0), V4[i] = 3 C[j][i] + C[n][i]
//              4:2:2: V4[i] = 4 C[y][i]                                            (the 4:2:0 line with n = j = y)
//   horizontal i = x >> 1, i2 = x odd ? min(i + 1, Wc - 1) : i,            C8 = V4[i] + V4[i2]     (8 x chroma)
//   offsets    y' = Y - 64 (limited) or Y (full), cb = C8_U - 4096, cr = C8_V - 4096
//   matrix     R = (A y' + RV cr + 32768) >> 16, G = (A y' - GU cb - GV cr + 32768) >> 16, B = (A y' + BU cb + 32768) >> 16,
//              int32, arithmetic shifts, each clamped to [0, 1023]
// Every intermediate stays below 2^28.  tests/ycbcr10_in_ref.py is the numpy restatement the tests hold the kernels to.
#pragma once
#include "common.h"
#include <math.h>

enum { YCC10_P010 = 0, YCC10_YUV420P10 = 1, YCC10_YUV422P10 = 2 };      // = HDRTV_YCC_P010 / _YUV420P10 / _YUV422P10

struct Ycc10Coef {
    int A, RV, GU, GV, BU, yoff;
};

// yuv_coef (yuv420.h) with the ten-bit ranges: sY = 1023/876, sC = 1023/896 (limited), 1 and 1 (full).
inline bool ycc10_coef(int matrix, int full_range, Ycc10Coef *k)
{
    double kr, kb;
    if (matrix == 601) { kr = 0.299; kb = 0.114; }
    else if (matrix == 709) { kr = 0.2126; kb = 0.0722; }
    else if (matrix == 2020) { kr = 0.2627; kb = 0.0593; }
    else return false;
    if (full_range != 0 && full_range != 1) return false;
    const double kg = 1.0 - kr - kb;
    const double sy = full_range ? 1.0 : 1023.0 / 876.0, sc = full_range ? 1.0 : 1023.0 / 896.0;
    auto rnd = [](double v) { return (int)floor(v + 0.5); };
    k->A = rnd(sy * 65536.0);
    k->RV = rnd(2.0 * (1.0 - kr) * sc * 8192.0);
    k->GU = rnd(2.0 * (1.0 - kb) * kb / kg * sc * 8192.0);
    k->GV = rnd(2.0 * (1.0 - kr) * kr / kg * sc * 8192.0);
    k->BU = rnd(2.0 * (1.0 - kb) * sc * 8192.0);
    k->yoff = full_range ? 0 : 64;
    return true;
}

// A frame in device memory; pitches in bytes, even.  Planar: u = Cb plane, v = Cr plane, c_pitch >= W.  P010: u = the interleaved
// CbCr plane (Cb at u16 2i, Cr at 2i + 1), v unused, c_pitch >= 2 W.  Pointers and pitches are two-byte aligned, no more.
struct Ycc10Src {
    const uint16_t *y, *u, *v;
    int y_pitch, c_pitch, fmt;
    Ycc10Coef k;
};

// The argument rule of the header, for the API and the launchers alike (one statement of it; a host function a stand-alone program
// can call).  0 when the planes describe a frame, else a message.
inline const char *ycc10_check(const void *y, int y_pitch, const void *u, const void *v, int c_pitch, int fmt, int H, int W)
{
    if (!y || !u) return "null plane";
    if (fmt != YCC10_P010 && fmt != YCC10_YUV420P10 && fmt != YCC10_YUV422P10) return "unknown fmt";
    if (fmt == YCC10_P010 ? v != nullptr : v == nullptr) return "dev_v must be NULL for P010 and given for the planar layouts";
    if (H <= 0 || W <= 0 || (W & 1) || (fmt != YCC10_YUV422P10 && (H & 1))) return "frame size is not positive and even";
    if ((y_pitch & 1) || (long long)y_pitch < 2LL * W) return "luma pitch is odd or below 2 W bytes";
    if ((c_pitch & 1) || (long long)c_pitch < (fmt == YCC10_P010 ? 2LL * W : (long long)W)) return "chroma pitch is odd or short";
    return nullptr;
}

// the ten-bit value of a sample word: shift 6 for P010, 0 for the planar layouts
__device__ __forceinline__ int ycc10_sample(uint32_t word, int shift) { return (int)((word >> shift) & 0x3ffu); }

// clamp(s >> 16, 0, 1023), the clamp applied before the shift (as yuv_sat_u8, and for its reason)
__device__ __forceinline__ uint32_t ycc10_sat(int s)
{
    return (uint32_t)(s < 0 ? 0 : (s > 0x3ffffff ? 0x3ffffff : s)) >> 16;
}

// The matrix step of the rule: luma value Y and the two 8 x chroma sums -> ten-bit R, G, B.
__device__ __forceinline__ void ycc10_rule(int Y, int c8u, int c8v, const Ycc10Coef &k, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int ay = k.A * (Y - k.yoff), cb = c8u - 4096, cr = c8v - 4096;
    r = ycc10_sat(ay + k.RV * cr + 32768);
    g = ycc10_sat(ay - k.GU * cb - k.GV * cr + 32768);
    b = ycc10_sat(ay + k.BU * cb + 32768);
}

// ycbcr10_in.hip
hipError_t ycbcr10_to_rgb10_launch(const Ycc10Src &src, int H, int W, uint16_t *rgb, hipStream_t s);
hipError_t pre_unpack_ycbcr10_f32_launch(const Ycc10Src &src, int H, int W, float *rgb, hipStream_t s);
// letterbox10.hip: planes at the source size p.sh x p.sw -> the letterboxed frame p.dh x p.dw (p: letterbox_setup's geometry and tables;
// its src / dst are not read), converted and resampled in one launch.  store: u16 [dh][dw][3] codes, or the f16 / f32 [3][dh][dw]
// tensor of those codes.  hipErrorInvalidValue, nothing enqueued, for planes ycc10_check refuses at the source size, a null dst or a
// shrink beyond LB10_MAX_SHRINK on an axis (letterbox10_size_ok).
enum { LB10_U16_HWC = 0, LB10_F16_CHW = 1, LB10_F32_CHW = 2 };
constexpr int LB10_MAX_SHRINK = 4;
bool letterbox10_size_ok(const LetterboxParams &p);
hipError_t letterbox10_launch(const Ycc10Src &src, const LetterboxParams &p, int store, void *dst, hipStream_t s);
// ... and the 0.25x condition map of an f16 tensor [3][H][W] in condition modes 1 and 2 (mode 0: cond_resize_launch)
hipError_t cond_quarter_f16_launch(const f16 *in, f16 *out, int H, int W, int mode, hipStream_t s);
// prepost.hip: pre_fused with the 10-bit staging step (same tables, modes and outputs as pre_fused_launch)
hipError_t pre_fused_ycbcr10_launch(const Ycc10Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const float *wx,
                                    const int *xmn, const int *xns, const float *wy, const int *ymn, const int *yns, int mode,
                                    hipStream_t s);
