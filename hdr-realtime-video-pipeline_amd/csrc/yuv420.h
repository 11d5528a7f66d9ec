// yuv420.h -- 8-bit 4:2:0 Y'CbCr input (I420, NV12): the conversion rule include/hdrtv_mi355x.h states, as one device helper,
// and the launchers of the kernels that apply it (yuv420.hip; pre_fused's YUV instantiation in prepost.hip).
//
// The rule, per luma pixel (x, y) of an even-sized H x W frame, chroma planes Hc = H / 2 rows by Wc = W / 2 samples:
//   vertical   j = y >> 1, n = y odd ? min(j + 1, Hc - 1) : max(j - 1, 0), V4[i] = 3 C[j][i] + C[n][i]
//   horizontal i = x >> 1, i2 = x odd ? min(i + 1, Wc - 1) : i,            C8 = V4[i] + V4[i2]     (8 x chroma)
//   offsets    y' = Y - 16 (limited) or Y (full), cb = C8_U - 1024, cr = C8_V - 1024
//   matrix     R = (A y' + RV cr + 32768) >> 16, G = (A y' - GU cb - GV cr + 32768) >> 16, B = (A y' + BU cb + 32768) >> 16,
//              int32, arithmetic shifts, each clamped to [0, 255]
// Every intermediate stays below 2^26.  tests/yuv420_ref.py is the numpy restatement the tests hold the kernels to.
#pragma once
#include "common.h"
#include <math.h>

enum { YUV_I420 = 0, YUV_NV12 = 1 };      // = HDRTV_YUV_I420 / HDRTV_YUV_NV12

struct YuvCoef {
    int A, RV, GU, GV, BU, yoff;
};

// (Kr, Kb) of BT.601 / BT.709 / BT.2020 (non-constant luminance); false for any other matrix or range.  rnd(v) = floor(v + 0.5)
// in double; A = rnd(sY 2^16), the chroma terms are scaled by 2^13 because C8 carries 8 x chroma.
inline bool yuv_coef(int matrix, int full_range, YuvCoef *k)
{
    double kr, kb;
    if (matrix == 601) { kr = 0.299; kb = 0.114; }
    else if (matrix == 709) { kr = 0.2126; kb = 0.0722; }
    else if (matrix == 2020) { kr = 0.2627; kb = 0.0593; }
    else return false;
    if (full_range != 0 && full_range != 1) return false;
    const double kg = 1.0 - kr - kb;
    const double sy = full_range ? 1.0 : 255.0 / 219.0, sc = full_range ? 1.0 : 255.0 / 224.0;
    auto rnd = [](double v) { return (int)floor(v + 0.5); };
    k->A = rnd(sy * 65536.0);
    k->RV = rnd(2.0 * (1.0 - kr) * sc * 8192.0);
    k->GU = rnd(2.0 * (1.0 - kb) * kb / kg * sc * 8192.0);
    k->GV = rnd(2.0 * (1.0 - kr) * kr / kg * sc * 8192.0);
    k->BU = rnd(2.0 * (1.0 - kb) * sc * 8192.0);
    k->yoff = full_range ? 0 : 16;
    return true;
}

// A frame in device memory.  I420: u = Cb plane, v = Cr plane, c_pitch >= W / 2.  NV12: u = the interleaved CbCr plane (Cb at
// byte 2i, Cr at 2i + 1), v unused, c_pitch >= W.  No pointer or pitch needs any alignment.
struct Yuv420Src {
    const uint8_t *y, *u, *v;
    int y_pitch, c_pitch, layout;
    YuvCoef k;
};

// clamp(s >> 16, 0, 255), with the clamp applied to s before the shift (the same value: the shift is monotonic).  The
// shift-then-clamp form lets hipcc pair two results into v_ashr_pk_u8_i32, whose packed result it then ORs into a byte
// word as if its upper 16 bits were zero; they are not (bytes 2 and 3 of the BGR words came out wrong).
__device__ __forceinline__ uint32_t yuv_sat_u8(int s)
{
    return (uint32_t)(s < 0 ? 0 : (s > 0xffffff ? 0xffffff : s)) >> 16;
}

// The matrix step of the rule: luma byte Y and the two 8 x chroma sums -> u8 R, G, B.
__device__ __forceinline__ void yuv_rule(int Y, int c8u, int c8v, const YuvCoef &k, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int ay = k.A * (Y - k.yoff), cb = c8u - 1024, cr = c8v - 1024;
    r = yuv_sat_u8(ay + k.RV * cr + 32768);
    g = yuv_sat_u8(ay - k.GU * cb - k.GV * cr + 32768);
    b = yuv_sat_u8(ay + k.BU * cb + 32768);
}

// yuv420.hip
hipError_t yuv420_to_bgr_launch(const Yuv420Src &src, int H, int W, uint8_t *bgr, hipStream_t s);
hipError_t pre_unpack_yuv_f32_launch(const Yuv420Src &src, int H, int W, float *rgb, hipStream_t s);
// prepost.hip: pre_fused with the YUV staging step (same tables, modes and outputs as pre_fused_launch)
hipError_t pre_fused_yuv_launch(const Yuv420Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const float *wx,
                                const int *xmn, const int *xns, const float *wy, const int *ymn, const int *yns, int mode,
                                hipStream_t s);
// fp32_ops.hip: the condition-map half of pre_f32_launch on its own (planar fp32 RGB -> cond)
hipError_t cond_resize_f32_launch(const float *rgb, float *cond, int H, int W, int Ho, int Wo, const float *wx, const int *xmn,
                                  const int *xns, const float *wy, const int *ymn, const int *yns, int mode, hipStream_t s);
