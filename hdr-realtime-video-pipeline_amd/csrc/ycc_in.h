// ycc_in.h -- Y'CbCr input at 8 bits (I420, NV12) and 10 bits (P010, yuv420p10le, yuv422p10le): the one statement of the conversion
// rule include/hdrtv_mi355x.h gives, for every kernel that applies it (yuv420.hip, ycbcr10_in.hip, pre_fused's plane instantiations in
// prepost.hip, letterbox10.hip), and the launchers of those kernels.  The host half is plain C++17 (no HIP header, no HIP call): a
// stand-alone program can call it (tests/test_ycc_in_host.py); the device half and the launchers follow under __HIPCC__.
//
// The rule at BITS = 8 | 10, top = 2^BITS - 1.  8-bit samples are bytes.  10-bit samples are little-endian u16: P010 carries the value
// in the high ten bits (v = word >> 6), the planar layouts in the low ten (v = word & 0x3ff).  Per luma pixel (x, y) of an H x W frame
// (W even; H even for 4:2:0), chroma planes Hc rows (H / 2, or H for 4:2:2) by Wc = W / 2 samples:
//   vertical   4:2:0: j = y >> 1, n = y odd ? min(j + 1, Hc - 1) : max(j - 1, 0), V4[i] = 3 C[j][i] + C[n][i]
//              4:2:2: V4[i] = 4 C[y][i]                                            (the 4:2:0 line with n = j = y)
//   horizontal i = x >> 1, i2 = x odd ? min(i + 1, Wc - 1) : i,            C8 = V4[i] + V4[i2]     (8 x chroma)
//   offsets    y' = Y - (16 << (BITS - 8)) (limited) or Y (full), cb = C8_U - (4 << BITS), cr = C8_V - (4 << BITS)
//   matrix     R = (A y' + RV cr + 32768) >> 16, G = (A y' - GU cb - GV cr + 32768) >> 16, B = (A y' + BU cb + 32768) >> 16,
//              int32, arithmetic shifts, each clamped to [0, top]
// Every intermediate stays below 2^26 at 8 bits and 2^28 at 10.  tests/yuv420_ref.py and tests/ycbcr10_in_ref.py are the numpy
// restatements the tests hold the kernels to.
#pragma once
#include <math.h>
#include <stdint.h>

#include <type_traits>

enum { YUV_I420 = 0, YUV_NV12 = 1 };                                    // = HDRTV_YUV_I420 / HDRTV_YUV_NV12
enum { YCC10_P010 = 0, YCC10_YUV420P10 = 1, YCC10_YUV422P10 = 2 };      // = HDRTV_YCC_P010 / _YUV420P10 / _YUV422P10

// A layout value means what the entry points of its depth say it means: which one interleaves CbCr in one plane, which one is 4:2:2.
constexpr bool ycc_interleaved(int bits, int layout) { return bits == 8 ? layout == YUV_NV12 : layout == YCC10_P010; }
constexpr bool ycc_is422(int bits, int layout) { return bits == 10 && layout == YCC10_YUV422P10; }

struct YccCoef {
    int A, RV, GU, GV, BU, yoff;
};

// (Kr, Kb) of BT.601 / BT.709 / BT.2020 (non-constant luminance); false for any other matrix or range.  rnd(v) = floor(v + 0.5) in
// double; limited range: sY = top / (219 << (bits - 8)), sC = top / (224 << (bits - 8)); A = rnd(sY 2^16), the chroma terms are
// scaled by 2^13 because C8 carries 8 x chroma.
inline bool ycc_coef(int bits, int matrix, int full_range, YccCoef *k)
{
    double kr, kb;
    if (matrix == 601) { kr = 0.299; kb = 0.114; }
    else if (matrix == 709) { kr = 0.2126; kb = 0.0722; }
    else if (matrix == 2020) { kr = 0.2627; kb = 0.0593; }
    else return false;
    if (full_range != 0 && full_range != 1) return false;
    const double kg = 1.0 - kr - kb;
    const double top = (double)((1 << bits) - 1), step = (double)(1 << (bits - 8));      // 255 / 219 / 224, or 1023 / 876 / 896
    const double sy = full_range ? 1.0 : top / (219.0 * step), sc = full_range ? 1.0 : top / (224.0 * step);
    auto rnd = [](double v) { return (int)floor(v + 0.5); };
    k->A = rnd(sy * 65536.0);
    k->RV = rnd(2.0 * (1.0 - kr) * sc * 8192.0);
    k->GU = rnd(2.0 * (1.0 - kb) * kb / kg * sc * 8192.0);
    k->GV = rnd(2.0 * (1.0 - kr) * kr / kg * sc * 8192.0);
    k->BU = rnd(2.0 * (1.0 - kb) * sc * 8192.0);
    k->yoff = full_range ? 0 : 16 << (bits - 8);
    return true;
}

// The argument rule of the header, for the API and the launchers alike.  0 when the planes describe a frame, else what is wrong with
// them, the first of these in this order.  Pitches are in bytes; at ten bits they are even.  A luma row holds W samples, a chroma row
// W / 2 per plane, or W in the interleaved plane.
inline const char *ycc_check(int bits, const void *y, int y_pitch, const void *u, const void *v, int c_pitch, int layout, int H, int W)
{
    const int bps = bits == 8 ? 1 : 2;
    if (!y || !u) return "null plane";
    if (layout < 0 || layout > (bits == 8 ? (int)YUV_NV12 : (int)YCC10_YUV422P10)) return "unknown layout";
    if (ycc_interleaved(bits, layout) ? v != nullptr : v == nullptr) return "dev_v must be NULL for NV12 / P010 and given for the planar layouts";
    if (H <= 0 || W <= 0 || (W & 1) || (!ycc_is422(bits, layout) && (H & 1))) return "frame size is not positive and even";
    if ((y_pitch & (bps - 1)) || (long long)y_pitch < (long long)bps * W) return "luma pitch is odd or below a row of samples";
    if ((c_pitch & (bps - 1)) || (long long)c_pitch < (long long)bps * (ycc_interleaved(bits, layout) ? W : W / 2)) return "chroma pitch is odd or short";
    return nullptr;
}

// A frame in device memory; pitches in bytes.  Planar: u = Cb plane, v = Cr plane.  Interleaved (NV12, P010): u = the CbCr plane (Cb
// at sample 2i, Cr at 2i + 1), v unused.  Pointers and pitches are aligned to the sample (one byte, or two), no more.
template <int BITS>
struct YccSrc {
    using sample = std::conditional_t<BITS == 8, uint8_t, uint16_t>;
    const sample *y, *u, *v;
    int y_pitch, c_pitch, layout;
    YccCoef k;
};
// the two depths under the names their kernels' symbols carry (pre_fused_kernel<Yuv420Src>, <Ycc10Src>: profiles and ISA tests read them)
struct Yuv420Src : YccSrc<8> {};
struct Ycc10Src : YccSrc<10> {};

template <int BITS>
inline bool ycc_ok(const YccSrc<BITS> &s, int H, int W)
{
    return ycc_check(BITS, s.y, s.y_pitch, s.u, s.v, s.c_pitch, s.layout, H, W) == nullptr;
}

#ifdef __HIPCC__
#include "launchers.h"

// the value of a sample word: the byte itself at 8 bits; at 10 bits shift 6 for P010, 0 for the planar layouts
template <int BITS>
__device__ __forceinline__ int ycc_sample(uint32_t word, int shift)
{
    return BITS == 8 ? (int)word : (int)((word >> shift) & 0x3ffu);
}

// clamp(s >> 16, 0, top), with the clamp applied to s before the shift (the same value: the shift is monotonic).  The
// shift-then-clamp form lets hipcc pair two results into v_ashr_pk_u8_i32, whose packed result it then ORs into a byte
// word as if its upper 16 bits were zero; they are not (bytes 2 and 3 of the BGR words came out wrong).
template <int BITS>
__device__ __forceinline__ uint32_t ycc_sat(int s)
{
    constexpr int top = (1 << (BITS + 16)) - 1;
    return (uint32_t)(s < 0 ? 0 : (s > top ? top : s)) >> 16;
}

// The matrix step of the rule: luma value Y and the two 8 x chroma sums -> R, G, B in [0, 2^BITS - 1].
template <int BITS>
__device__ __forceinline__ void ycc_rule(int Y, int c8u, int c8v, const YccCoef &k, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int ay = k.A * (Y - k.yoff), cb = c8u - (4 << BITS), cr = c8v - (4 << BITS);
    r = ycc_sat<BITS>(ay + k.RV * cr + 32768);
    g = ycc_sat<BITS>(ay - k.GU * cb - k.GV * cr + 32768);
    b = ycc_sat<BITS>(ay + k.BU * cb + 32768);
}

// The vertical line of the rule: chroma rows j (weight 3) and n (weight 1) of luma row y; c422: n = j = y.
__device__ __forceinline__ void ycc_rows(int y, int Hc, bool c422, int &j, int &n)
{
    j = c422 ? y : y >> 1;
    n = c422 ? y : (y & 1) ? min(j + 1, Hc - 1) : max(j - 1, 0);
}

// The horizontal line: the right neighbour i2 of chroma column i.  last = Wc - 1 for a kernel that reads the planes; a kernel that stages
// columns ilo .. ihi passes last = ihi (<= Wc - 1), so that it never reads a column it did not stage.  That bound is deliberate and part
// of every staged walk; it binds only on a column whose odd pixel lies outside the patch and is not written, so no result depends on it.
__device__ __forceinline__ int ycc_col2(int i, int last) { return min(i + 1, last); }

// The chroma walk of the pair of pixels that shares chroma column i: the V4 sums 3 C[j] + C[n] of Cb and Cr at column i (a) and at its
// right neighbour i2 (b).  The pair's 8 x chroma is then 2 u4a for the even pixel and u4a + u4b for the odd one.  ka / kb are the
// positions of columns i / i2 in the rows the caller hands over, by its own stride and offset:
//   ycc_walk(uj, un, vj, vn, ...)   rows j / n of Cb and of Cr: the planes themselves (planar: ka = i; interleaved: vj = uj + 1, ka = 2 i)
//   ycc_walk(cj, cn, ..., co, ...)  staged rows j / n that hold Cb at k and Cr at k + co (planar: ka = i - ilo, co = the row's half;
//                                   interleaved: ka = 2 (i - ilo), co = 1)
template <int BITS>
__device__ __forceinline__ int ycc_v4(uint32_t cj, uint32_t cn, int shift) { return 3 * ycc_sample<BITS>(cj, shift) + ycc_sample<BITS>(cn, shift); }

template <int BITS, typename P>
__device__ __forceinline__ void ycc_walk(const P *uj, const P *un, const P *vj, const P *vn, int ka, int kb, int shift, int &u4a, int &u4b,
                                         int &v4a, int &v4b)
{
    u4a = ycc_v4<BITS>(uj[ka], un[ka], shift);
    v4a = ycc_v4<BITS>(vj[ka], vn[ka], shift);
    u4b = ycc_v4<BITS>(uj[kb], un[kb], shift);
    v4b = ycc_v4<BITS>(vj[kb], vn[kb], shift);
}

template <int BITS, typename P>
__device__ __forceinline__ void ycc_walk(const P *cj, const P *cn, int ka, int kb, int co, int shift, int &u4a, int &u4b, int &v4a, int &v4b)
{
    u4a = ycc_v4<BITS>(cj[ka], cn[ka], shift);
    u4b = ycc_v4<BITS>(cj[kb], cn[kb], shift);
    v4a = ycc_v4<BITS>(cj[ka + co], cn[ka + co], shift);
    v4b = ycc_v4<BITS>(cj[kb + co], cn[kb + co], shift);
}

template <typename T>
__device__ __forceinline__ const T *row_of(const T *p, int row, int pitch_bytes)
{
    return reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(p) + (size_t)row * pitch_bytes);
}

// The 10-bit plane stager.  Planes and pitches are two-byte aligned and no more, so a row segment [seg, seg + 2 len) is read as the
// whole aligned dwords that hold at least one of its samples, never a dword past its last byte.  ycc10_load: dword d of the segment
// (seg null: nothing), rel = the sample index of its low half (-1 or even; -1000: not loaded).  ycc10_keep: each half of the dword is
// kept or dropped.  D is the staging area's element (a may_alias u16 where the same LDS is f16 elsewhere, or the u32 patch word).
__device__ __forceinline__ void ycc10_load(const uint16_t *seg, int len, int d, uint32_t &word, int &rel)
{
    const uintptr_t a = ((uintptr_t)seg & ~(uintptr_t)3) + 4 * (uintptr_t)d;
    const bool ok = seg != nullptr && a < (uintptr_t)seg + 2 * (uintptr_t)len;
    rel = ok ? (int)((long)a - (long)(uintptr_t)seg) >> 1 : -1000;
    word = ok ? *reinterpret_cast<const uint32_t *>(a) : 0u;
}

template <typename D>
__device__ __forceinline__ void ycc10_keep(D *dst, int len, uint32_t word, int rel)
{
    if (rel >= 0 && rel < len) dst[rel] = (D)(word & 0xffffu);
    if (rel + 1 >= 0 && rel + 1 < len) dst[rel + 1] = (D)(word >> 16);
}

// Rows [row0, row0 + nrows) x samples [col0, col0 + len) of a plane -> dst[r * dst_pitch + k], by a 256-thread workgroup: four loads
// in flight per thread before the first is unpacked.
template <typename D>
__device__ __forceinline__ void ycc10_stage(const uint16_t *plane, int pitch_bytes, int row0, int nrows, int col0, int len, D *dst,
                                            int dst_pitch, int tid)
{
    const int ndw = len / 2 + 1, n = nrows * ndw;             // ceil((2 len + 2) / 4) dwords cover a segment at either alignment
    for (int e0 = tid; e0 < n; e0 += 4 * 256) {
        uint32_t word[4];
        int rel[4], row[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + 256 * i;
            rel[i] = -1000; row[i] = 0; word[i] = 0u;
            if (e < n) {                                      // ycc10_load's rule with the row kept beside it, in nested form: as one
                const int r = e / ndw, d = e - r * ndw;       // select per value it cost letterbox10_kernel 2 - 4 % (profiles/input_refactor_timing.txt)
                const uint16_t *seg = row_of(plane, row0 + r, pitch_bytes) + col0;
                const uintptr_t a = ((uintptr_t)seg & ~(uintptr_t)3) + 4 * (uintptr_t)d;
                if (a < (uintptr_t)seg + 2 * (uintptr_t)len) {
                    rel[i] = (int)((long)a - (long)(uintptr_t)seg) >> 1;
                    row[i] = r;
                    word[i] = *reinterpret_cast<const uint32_t *>(a);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ycc10_keep(dst + row[i] * dst_pitch, len, word[i], rel[i]);
    }
}

// R, G, B of the two pixels of pair i (luma columns 2i, 2i + 1) of row y, read from the planes.  W is even, so a pair never straddles
// two rows, and it shares its chroma column i.
template <int BITS>
__device__ __forceinline__ void ycc_pair(const YccSrc<BITS> &s, int H, int W, int y, int i, uint32_t (&r)[2], uint32_t (&g)[2],
                                         uint32_t (&b)[2])
{
    using T = typename YccSrc<BITS>::sample;
    const bool il = ycc_interleaved(BITS, s.layout);
    const int sh = BITS == 10 && il ? 6 : 0, i2 = ycc_col2(i, (W >> 1) - 1);
    int j, n;
    ycc_rows(y, H >> 1, ycc_is422(BITS, s.layout), j, n);
    const T *yr = row_of(s.y, y, s.y_pitch) + 2 * i;
    int u4a, u4b, v4a, v4b;
    if (il) {
        const T *cj = row_of(s.u, j, s.c_pitch), *cn = row_of(s.u, n, s.c_pitch);
        ycc_walk<BITS>(cj, cn, cj + 1, cn + 1, 2 * i, 2 * i2, sh, u4a, u4b, v4a, v4b);
    } else {
        ycc_walk<BITS>(row_of(s.u, j, s.c_pitch), row_of(s.u, n, s.c_pitch), row_of(s.v, j, s.c_pitch), row_of(s.v, n, s.c_pitch), i, i2, sh,
                       u4a, u4b, v4a, v4b);
    }
    ycc_rule<BITS>(ycc_sample<BITS>(yr[0], sh), 2 * u4a, 2 * v4a, s.k, r[0], g[0], b[0]);
    ycc_rule<BITS>(ycc_sample<BITS>(yr[1], sh), u4a + u4b, v4a + v4b, s.k, r[1], g[1], b[1]);
}

// planes -> fp32 planar RGB, float(code) * fp32(1 / top): pre_unpack_f32 (fp32_ops.hip) of the converted frame, for the fp32 preset
// (cond_resize_f32 follows).  One lane = one pair.  The body of pre_unpack_yuv_f32_kernel (yuv420.hip) and
// pre_unpack_ycbcr10_f32_kernel (ycbcr10_in.hip).
template <int BITS>
__device__ __forceinline__ void ycc_unpack_f32(const YccSrc<BITS> &src, int H, int W, float *__restrict__ out)
{
    const float k = (float)(1.0 / ((1 << BITS) - 1));
    const size_t npix = (size_t)H * W, npair = npix / 2;
    const int Wc = W >> 1;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < npair; t += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(t / (size_t)Wc), i = (int)(t - (size_t)y * Wc);
        uint32_t r[2], g[2], b[2];
        ycc_pair(src, H, W, y, i, r, g, b);
        const size_t o = (size_t)y * W + 2 * i;
        out[o] = __fmul_rn((float)r[0], k);
        out[o + 1] = __fmul_rn((float)r[1], k);
        out[npix + o] = __fmul_rn((float)g[0], k);
        out[npix + o + 1] = __fmul_rn((float)g[1], k);
        out[2 * npix + o] = __fmul_rn((float)b[0], k);
        out[2 * npix + o + 1] = __fmul_rn((float)b[1], k);
    }
}

// the capped grid of the element-wise kernels: 256 CUs x 8 blocks, grid-stride beyond (as prepost.hip's ew_grid)
inline int ycc_grid(size_t n)
{
    size_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    return (int)(g < 1 ? 1 : g);
}

// ---- launchers
// prepost.hip: pre_fused with the plane staging step (same tables, modes and outputs as pre_fused_launch)
hipError_t pre_fused_yuv_launch(const Yuv420Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s);
hipError_t pre_fused_ycbcr10_launch(const Ycc10Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s);
// yuv420.hip, ycbcr10_in.hip
hipError_t yuv420_to_bgr_launch(const Yuv420Src &src, int H, int W, uint8_t *bgr, hipStream_t s);
hipError_t ycbcr10_to_rgb10_launch(const Ycc10Src &src, int H, int W, uint16_t *rgb, hipStream_t s);
hipError_t pre_unpack_yuv_f32_launch(const Yuv420Src &src, int H, int W, float *rgb, hipStream_t s);
hipError_t pre_unpack_ycbcr10_f32_launch(const Ycc10Src &src, int H, int W, float *rgb, hipStream_t s);
// letterbox10.hip: planes at the source size p.sh x p.sw -> the letterboxed frame p.dh x p.dw (p: letterbox_setup's geometry and tables;
// its src / dst are not read), converted and resampled in one launch.  store: u16 [dh][dw][3] codes, or the f16 / f32 [3][dh][dw]
// tensor of those codes.  hipErrorInvalidValue, nothing enqueued, for planes ycc_check refuses at the source size, a null dst or a
// shrink beyond LB10_MAX_SHRINK on an axis (letterbox10_size_ok).
enum { LB10_U16_HWC = 0, LB10_F16_CHW = 1, LB10_F32_CHW = 2 };
constexpr int LB10_MAX_SHRINK = 4;
bool letterbox10_size_ok(const LetterboxParams &p);
hipError_t letterbox10_launch(const Ycc10Src &src, const LetterboxParams &p, int store, void *dst, hipStream_t s);
// ... and the 0.25x condition map of an f16 tensor [3][H][W] in condition modes 1 and 2 (mode 0: cond_resize_launch)
hipError_t cond_quarter_f16_launch(const f16 *in, f16 *out, int H, int W, int mode, hipStream_t s);
#endif
