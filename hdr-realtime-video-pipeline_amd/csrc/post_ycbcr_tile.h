// post_ycbcr_tile.h -- the tile code of the 10-bit Y'CbCr conversion (include/hdrtv_mi355x.h states the integer rule), shared by
// post_ycbcr.hip (MODE = YC_ROUND: the rule's own rounding constants), post_ycbcr_dither.hip (YC_ORDERED: the 16 x 16 Bayer threshold
// in their place) and post_ycbcr_fs.hip (YC_FS_SAMPLES: the samples in 1/4096 code as int32, for the error diffusion that follows):
// the two sources, the luma / staging pass and the chroma pass.  post_ycbcr.hip's header comment describes the tile, the
// lanes' jobs and the LDS layout; the dither adds a handful of integer operations per sample and no memory access.
#pragma once
#include "launchers.h"
#include "post_quant.h"
#include "../../include/hdrtv_mi355x.h"

namespace {

constexpr int YC_LR = YC_TH + 1;        // LDS rows: [0] the row above the tile (top-left siting), [1 ..] the tile's
constexpr int YC_C0 = 8;                // LDS column of the tile's first pixel; [YC_C0 - 1] the column left of it
constexpr int YC_RS = YC_TW + YC_C0;    // row stride in u16: 272 bytes, 16-byte groups stay aligned
constexpr int YC_GW = YC_TW / 8;        // eight-pixel groups per tile row
static_assert(YC_GW == 16 && YC_TH * YC_GW == 256 && YC_LR <= 64, "one stage job per lane; the halo column fits one wave");

// rnd(K * 2^20 * 876 / 65535) and rnd(K' * 2^20 * 896 / 65535), green the remainder (the header derives them)
// what a sample becomes: rounded to ten bits, rounded against the Bayer threshold, or kept in 1/4096 code (u of the header's
// Floyd-Steinberg rule) and written as int32 -- then p.dst_y / dst_u / dst_v are int32 planes (Y', Cb, Cr; P010 is not interleaved
// here) and the pitches count int32 elements
constexpr int YC_ROUND = 0, YC_ORDERED = 1, YC_FS_SAMPLES = 2;

constexpr int YC_YR = 3682, YC_YG = 9503, YC_YB = 831;
constexpr int YC_UR = -2002, YC_UG = -5166, YC_UB = 7168;
constexpr int YC_VR = 7168, YC_VG = -6591, YC_VB = -577;

__device__ __forceinline__ bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

__device__ __forceinline__ uint4 pack8(const uint32_t (&v)[8])
{
    return make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}

// the model's planar tensor: the codes hdrtv_post_rgb48 (PQ = false) / hdrtv_post_pq_rgb48 (PQ = true) write
template <typename T, bool PQ>
struct TensorSrc {
    const T *in;
    size_t plane;
    int W;
    float peak;
    const float *bnd;

    __device__ __forceinline__ void wide8(const T *p, float (&v)[8]) const
    {
        if (sizeof(T) == 2) {
            const f16x8 x = *reinterpret_cast<const f16x8 *>(p);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
        } else {
            const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
    }
    // pixels x .. x + 7 of row y, the first n (2 .. 8) inside the frame; the others repeat pixel x + n - 1
    __device__ __forceinline__ void px8(int y, int x, int n, uint32_t (&q)[3][8]) const
    {
        const T *p = in + (size_t)y * W + x;
        float v[3][8];
        if (n == 8 && aligned_to(p, 16) && aligned_to(p + plane, 16) && aligned_to(p + 2 * plane, 16)) {
            wide8(p, v[0]);
            wide8(p + plane, v[1]);
            wide8(p + 2 * plane, v[2]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int xi = min(i, n - 1);
                v[0][i] = (float)p[xi];
                v[1][i] = (float)p[plane + xi];
                v[2][i] = (float)p[2 * plane + xi];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) quant_rgb<PQ>(v[0][i], v[1][i], v[2][i], peak, bnd, q[0][i], q[1][i], q[2][i]);
    }
    __device__ __forceinline__ void px1(int y, int x, uint32_t (&q)[3]) const
    {
        const T *p = in + (size_t)y * W + x;
        quant_rgb<PQ>((float)p[0], (float)p[plane], (float)p[2 * plane], peak, bnd, q[0], q[1], q[2]);
    }
};

// RGB48 codes already in device memory: u16 [H][W][3]
struct Rgb48Src {
    const uint16_t *in;
    int W;

    __device__ __forceinline__ void px8(int y, int x, int n, uint32_t (&q)[3][8]) const
    {
        const uint16_t *p = in + ((size_t)y * W + x) * 3;
        if (n == 8 && aligned_to(p, 16)) {
            const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1],
                        c = reinterpret_cast<const uint4 *>(p)[2];
            const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int e = 3 * i + ch;
                    q[ch][i] = (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int xi = min(i, n - 1);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) q[ch][i] = p[xi * 3 + ch];
            }
        }
    }
    __device__ __forceinline__ void px1(int y, int x, uint32_t (&q)[3]) const
    {
        const uint16_t *p = in + ((size_t)y * W + x) * 3;
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
};

// The 16 x 16 Bayer index M(x, y) of the ordered-dither rule: bit i of (x ^ y) & 15 at bit 7 - 2i, bit i of y & 15 at bit 6 - 2i
__device__ __forceinline__ uint32_t bayer_spread4(uint32_t v)       // bit i of the reversed nibble -> bit 2 (3 - i)
{
    v = __brev(v) >> 28;
    v = (v | (v << 2)) & 0x33u;
    return (v | (v << 1)) & 0x55u;
}
__device__ __forceinline__ uint32_t bayer16(int x, int y) { return (bayer_spread4((uint32_t)(x ^ y) & 15u) << 1) | bayer_spread4((uint32_t)y & 15u); }

// Four chroma samples of chroma row `crow` of the tile, first luma column 8 * g.  VM = the vertical taps: 0 one row (4:2:2),
// 1 rows 2j, 2j + 1 (left siting, Wt 8), 2 rows 2j - 1, 2j, 2j + 1 with weights 1 2 1 (top-left siting, Wt 16); Wt = 4 << VM.
// YC_ORDERED: (ci, cj) = column and row of the first sample in the chroma plane; the rounding constant becomes (2 M + 1) << (SH - 9).
// YC_FS_SAMPLES: cb / cr hold the signed samples (sum + (1 << (SH - 13))) >> (SH - 12), without the 512.
template <int VM, int MODE>
__device__ __forceinline__ void chroma4(const uint16_t (*codes)[YC_LR][YC_RS], int crow, int g, int ci, int cj, uint32_t (&cb)[4],
                                        uint32_t (&cr)[4])
{
    const int lr0 = VM == 0 ? crow + 1 : (VM == 1 ? 2 * crow + 1 : 2 * crow);
    int h[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        uint32_t s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k <= VM; ++k) {
            const uint32_t wv = (VM == 2 && k == 1) ? 2u : 1u;
            const uint16_t *row = &codes[ch][lr0 + k][YC_C0 + 8 * g];
            const uint4 w = *reinterpret_cast<const uint4 *>(row);
            s[0] += wv * row[-1];
            s[1] += wv * (w.x & 0xffffu); s[2] += wv * (w.x >> 16);
            s[3] += wv * (w.y & 0xffffu); s[4] += wv * (w.y >> 16);
            s[5] += wv * (w.z & 0xffffu); s[6] += wv * (w.z >> 16);
            s[7] += wv * (w.w & 0xffffu); s[8] += wv * (w.w >> 16);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) h[ch][j] = (int)(s[2 * j] + 2 * s[2 * j + 1] + s[2 * j + 2]);
    }
    constexpr long long HALF = (long long)(4 << VM) << 19;
    constexpr int SH = 22 + VM;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long rnd = MODE == YC_FS_SAMPLES ? 1ll << (SH - 13) : MODE == YC_ORDERED ? (long long)(2 * bayer16(ci + j, cj) + 1) << (SH - 9) : HALF;
        const long long u = (long long)YC_UR * h[0][j] + (long long)YC_UG * h[1][j] + (long long)YC_UB * h[2][j] + rnd;
        const long long v = (long long)YC_VR * h[0][j] + (long long)YC_VG * h[1][j] + (long long)YC_VB * h[2][j] + rnd;
        if (MODE == YC_FS_SAMPLES) {
            cb[j] = (uint32_t)(int)(u >> (SH - 12));
            cr[j] = (uint32_t)(int)(v >> (SH - 12));
        } else {
            cb[j] = (uint32_t)(512 + (int)(u >> SH));
            cr[j] = (uint32_t)(512 + (int)(v >> SH));
        }
    }
}

template <typename SRC, int FMT, int MODE>
__device__ __forceinline__ void ycbcr_tile(const SRC &src, const Ycbcr10Params &p)
{
    __shared__ __attribute__((aligned(16))) uint16_t codes[3][YC_LR][YC_RS];
    constexpr int SHL = FMT == HDRTV_YCC_P010 ? 6 : 0;
    constexpr bool V422 = FMT == HDRTV_YCC_YUV422P10;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * YC_TW, y0 = blockIdx.y * YC_TH;
    const bool topleft = !V422 && p.siting == HDRTV_SITING_TOPLEFT;

    // 1. stage + luma: lane = eight pixels (tid & 15) of tile row (tid >> 4)
    {
        const int r = tid >> 4, g = tid & 15, x = x0 + 8 * g, y = y0 + r;
        if (y < p.H && x < p.W) {
            const int n = min(8, p.W - x);
            uint32_t q[3][8], yy[8];
            src.px8(y, x, n, q);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (MODE == YC_FS_SAMPLES) {
                    yy[i] = (uint32_t)((YC_YR * (int)q[0][i] + YC_YG * (int)q[1][i] + YC_YB * (int)q[2][i] + (1 << 7)) >> 8);
                } else {
                    const int rnd = MODE == YC_ORDERED ? (int)((2 * bayer16(x + i, y) + 1) << 11) : 1 << 19;
                    yy[i] = (uint32_t)(64 + ((YC_YR * (int)q[0][i] + YC_YG * (int)q[1][i] + YC_YB * (int)q[2][i] + rnd) >> 20)) << SHL;
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<uint4 *>(&codes[ch][r + 1][YC_C0 + 8 * g]) = pack8(q[ch]);
            uint16_t *d = p.dst_y + (size_t)y * p.y_pitch + x;
            if (MODE == YC_FS_SAMPLES) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(p.dst_y) + (size_t)y * p.y_pitch + x;
                if (n == 8 && aligned_to(d32, 16)) {
                    reinterpret_cast<uint4 *>(d32)[0] = make_uint4(yy[0], yy[1], yy[2], yy[3]);
                    reinterpret_cast<uint4 *>(d32)[1] = make_uint4(yy[4], yy[5], yy[6], yy[7]);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (i < n) d32[i] = yy[i];
                }
            } else if (n == 8 && aligned_to(d, 16)) {
                *reinterpret_cast<uint4 *>(d) = pack8(yy);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (i < n) d[i] = (uint16_t)yy[i];
            }
        }
    }
    // the row above the tile (top-left siting; row 0 repeats above the frame): wave 1
    if (topleft && tid >= 64 && tid < 64 + YC_GW) {
        const int g = tid - 64, x = x0 + 8 * g;
        if (x < p.W) {
            uint32_t q[3][8];
            src.px8(max(y0 - 1, 0), x, min(8, p.W - x), q);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<uint4 *>(&codes[ch][0][YC_C0 + 8 * g]) = pack8(q[ch]);
        }
    }
    // the column left of the tile (column 0 repeats left of the frame), LDS rows 0 .. YC_TH: wave 2
    if (tid >= 128 && tid < 128 + YC_LR) {
        const int lr = tid - 128, y = max(y0 - 1 + lr, 0);
        if (y < p.H) {
            uint32_t q[3];
            src.px1(y, max(x0 - 1, 0), q);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) codes[ch][lr][YC_C0 - 1] = (uint16_t)q[ch];
        }
    }
    __syncthreads();

    // 2. chroma: job = four samples (job & 15) of chroma row (job >> 4)
    constexpr int CROWS = V422 ? YC_TH : YC_TH / 2;
    for (int job = tid; job < CROWS * YC_GW; job += 256) {
        const int crow = job >> 4, g = job & 15;
        const int x = x0 + 8 * g, y = y0 + (V422 ? crow : 2 * crow);        // luma position of the first sample
        if (y >= p.H || x >= p.W) continue;
        uint32_t cb[4], cr[4];
        const int nc = min(4, (p.W - x) >> 1), cy = V422 ? y : y >> 1;
        if (V422) chroma4<0, MODE>(codes, crow, g, x >> 1, cy, cb, cr);
        else if (topleft) chroma4<2, MODE>(codes, crow, g, x >> 1, cy, cb, cr);
        else chroma4<1, MODE>(codes, crow, g, x >> 1, cy, cb, cr);
        if (MODE == YC_FS_SAMPLES) {
            uint32_t *du = reinterpret_cast<uint32_t *>(p.dst_u) + (size_t)cy * p.c_pitch + (x >> 1);
            uint32_t *dv = reinterpret_cast<uint32_t *>(p.dst_v) + (size_t)cy * p.c_pitch + (x >> 1);
            if (nc == 4 && aligned_to(du, 16) && aligned_to(dv, 16)) {
                *reinterpret_cast<uint4 *>(du) = make_uint4(cb[0], cb[1], cb[2], cb[3]);
                *reinterpret_cast<uint4 *>(dv) = make_uint4(cr[0], cr[1], cr[2], cr[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nc) {
                        du[j] = cb[j];
                        dv[j] = cr[j];
                    }
                }
            }
        } else if (FMT == HDRTV_YCC_P010) {
            uint16_t *d = p.dst_u + (size_t)cy * p.c_pitch + x;
            if (nc == 4 && aligned_to(d, 16)) {
                *reinterpret_cast<uint4 *>(d) = make_uint4((cb[0] | (cr[0] << 16)) << 6, (cb[1] | (cr[1] << 16)) << 6,
                                                           (cb[2] | (cr[2] << 16)) << 6, (cb[3] | (cr[3] << 16)) << 6);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nc) {
                        d[2 * j] = (uint16_t)(cb[j] << 6);
                        d[2 * j + 1] = (uint16_t)(cr[j] << 6);
                    }
                }
            }
        } else {
            uint16_t *du = p.dst_u + (size_t)cy * p.c_pitch + (x >> 1), *dv = p.dst_v + (size_t)cy * p.c_pitch + (x >> 1);
            if (nc == 4 && aligned_to(du, 8) && aligned_to(dv, 8)) {
                *reinterpret_cast<uint2 *>(du) = make_uint2(cb[0] | (cb[1] << 16), cb[2] | (cb[3] << 16));
                *reinterpret_cast<uint2 *>(dv) = make_uint2(cr[0] | (cr[1] << 16), cr[2] | (cr[3] << 16));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nc) {
                        du[j] = (uint16_t)cb[j];
                        dv[j] = (uint16_t)cr[j];
                    }
                }
            }
        }
    }
}

bool ycbcr_params_ok(const Ycbcr10Params &p)
{
    if (!p.in || !p.dst_y || !p.dst_u || p.H < 1 || p.W < 2 || (p.W & 1)) return false;
    if (p.fmt != HDRTV_YCC_P010 && p.fmt != HDRTV_YCC_YUV420P10 && p.fmt != HDRTV_YCC_YUV422P10) return false;
    if (p.fmt != HDRTV_YCC_YUV422P10 && (p.H & 1)) return false;
    if (p.fmt != HDRTV_YCC_P010 && !p.dst_v) return false;
    if (p.siting != HDRTV_SITING_LEFT && (p.siting != HDRTV_SITING_TOPLEFT || p.fmt == HDRTV_YCC_YUV422P10)) return false;
    return p.y_pitch >= p.W && p.c_pitch >= (p.fmt == HDRTV_YCC_P010 ? p.W : p.W / 2);
}

}  // namespace
