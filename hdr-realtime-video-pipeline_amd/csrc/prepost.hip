// prepost.hip -- the HBM-bound per-pixel stages either side of the network (gfx950).
//
//  pre_unpack      u8 HWC BGR -> f16 planar RGB * (1/255)     hdrtvnet_torch.py:2256-2261
//  cond_resize     0.25x antialiased bicubic -> f16 planar    hdrtvnet_torch.py:2278-2285
//  post_u8         planar -> u8 HWC BGR                       hdrtvnet_torch.py:2357-2361
//  post_rgb48      planar -> u16 HWC RGB (rgb48le)            gui_pipeline_worker_feeders.py:223-227
//  post_pq_rgb48   BT.709->BT.2020 matrix + ST.2084 PQ + u16  (north-star display variant)
//
// All are one pass, 8 pixels per lane, 16-byte planar accesses and 8/16-byte interleaved
// accesses, so every wave instruction moves whole cache lines.  Quantisers use __fmul_rn /
// __fadd_rn: the reference rounds the multiply and the add separately.
#include "launchers.h"
#include "post_quant.h"
#include "ycc_in.h"

#include <type_traits>

namespace {

__global__ __launch_bounds__(256) void pre_unpack_kernel(const uint8_t *__restrict__ bgr, f16 *__restrict__ out,
                                                         size_t npix)
{
    const float k = (float)(1.0 / 255.0);
    const size_t ngrp = npix / 8;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += (size_t)gridDim.x * blockDim.x) {
        const uint2 *src = reinterpret_cast<const uint2 *>(bgr + g * 24);
        const uint2 a = src[0], b = src[1], c = src[2];
        const uint32_t w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
        f16x8 r, gg, bb;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = i * 3;
            const uint32_t vb = (w[o >> 2] >> ((o & 3) * 8)) & 0xff;
            const uint32_t vg = (w[(o + 1) >> 2] >> (((o + 1) & 3) * 8)) & 0xff;
            const uint32_t vr = (w[(o + 2) >> 2] >> (((o + 2) & 3) * 8)) & 0xff;
            r[i] = (f16)__fmul_rn((float)vr, k);
            gg[i] = (f16)__fmul_rn((float)vg, k);
            bb[i] = (f16)__fmul_rn((float)vb, k);
        }
        *reinterpret_cast<f16x8 *>(out + g * 8) = r;
        *reinterpret_cast<f16x8 *>(out + npix + g * 8) = gg;
        *reinterpret_cast<f16x8 *>(out + 2 * npix + g * 8) = bb;
    }
    // tail (< 8 pixels)
    if (blockIdx.x == 0 && threadIdx.x < (npix & 7)) {
        const size_t i = ngrp * 8 + threadIdx.x;
        out[i] = (f16)__fmul_rn((float)bgr[i * 3 + 2], k);
        out[npix + i] = (f16)__fmul_rn((float)bgr[i * 3 + 1], k);
        out[2 * npix + i] = (f16)__fmul_rn((float)bgr[i * 3 + 0], k);
    }
}

// ---- 0.25x antialiased bicubic.  Tap tables (ATen _upsample_bicubic2d_aa weights, computed on
// the host in fp32 exactly as ATen does) : wtab[o][0..16], first input index mn[o], count ns[o].
constexpr int RT_W = 32, RT_H = 8;          // output tile
constexpr int RT_IW = RT_W * 4 + 12;        // 140 input columns cover 32 outputs
constexpr int RT_IH = RT_H * 4 + 12;        // 44 input rows cover 8 outputs
constexpr int AA_TAPS = 17;

__global__ __launch_bounds__(256) void cond_resize_kernel(const f16 *__restrict__ in, f16 *__restrict__ out, int H,
                                                          int W, int Ho, int Wo, const float *__restrict__ wx,
                                                          const int *__restrict__ xmn, const int *__restrict__ xns,
                                                          const float *__restrict__ wy, const int *__restrict__ ymn,
                                                          const int *__restrict__ yns)
{
    __shared__ float s_in[RT_IH][RT_IW + 1];
    __shared__ float s_h[RT_IH][RT_W + 1];
    const int c = blockIdx.z;
    const int ox0 = blockIdx.x * RT_W, oy0 = blockIdx.y * RT_H;
    const int ix0 = xmn[ox0], iy0 = ymn[oy0];
    const f16 *src = in + (size_t)c * H * W;
    for (int e = threadIdx.x; e < RT_IH * RT_IW; e += 256) {
        const int r = e / RT_IW, q = e % RT_IW;
        const int iy = iy0 + r, ix = ix0 + q;
        s_in[r][q] = (iy < H && ix < W) ? (float)src[(size_t)iy * W + ix] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < RT_IH * RT_W; e += 256) {
        const int r = e / RT_W, o = e % RT_W;
        const int ox = ox0 + o;
        float s = 0.f;
        if (ox < Wo) {
            const int base = xmn[ox] - ix0, n = xns[ox];
            const float *w = wx + (size_t)ox * AA_TAPS;
            for (int j = 0; j < n; ++j) s = __fadd_rn(s, __fmul_rn(w[j], s_in[r][base + j]));
        }
        s_h[r][o] = s;
    }
    __syncthreads();
    {
        const int o = threadIdx.x % RT_W, r = threadIdx.x / RT_W;
        const int ox = ox0 + o, oy = oy0 + r;
        if (ox < Wo && oy < Ho) {
            const int base = ymn[oy] - iy0, n = yns[oy];
            const float *w = wy + (size_t)oy * AA_TAPS;
            float s = 0.f;
            for (int j = 0; j < n; ++j) s = __fadd_rn(s, __fmul_rn(w[j], s_h[base + j][o]));
            out[((size_t)c * Ho + oy) * Wo + ox] = (f16)s;
        }
    }
}

// ---- pre_fused: both halves of preprocess in one pass over the u8 frame ----------------------
// A workgroup owns a 32 x 8 tile of the 0.25x condition map = 128 x 32 input pixels.  It stages the 140 x 44 u8 BGR
// patch those outputs' 16-tap windows cover (aligned dword loads, each byte converted once to the f16 value
// fp16(float(u8) * fp32(1/255)) the reference's tensor holds), writes the 128 x 32 pixels it owns to the three f16 planes
// with 16-byte stores, and resamples the SAME values into the condition tile: horizontal pass then vertical pass,
// fp32, the tap order and rounding of cond_resize_kernel (= ATen's separable _upsample_bicubic2d_aa).  The frame is read
// from HBM once (3 B per pixel; halo re-reads hit L2) instead of 3 B + 6 B.
// mode 1: HDRTVNetTorch(fast_condition_resize=True) -- F.interpolate(0.25, bilinear, align_corners=False): source
// coordinate 4d + 1.5, i.e. the mean of pixels (4d+1, 4d+2) in each direction (hdrtvnet_torch.py:2269-2276).
// mode 2: HDRTVNET_ZERO_COND -- the condition map is zero (hdrtvnet_torch.py:2265-2267).
constexpr int PF_OW = 32, PF_OH = 8, PF_IW = 140, PF_IH = 44, PF_ROWDW = 107;   // 107 dwords cover 420 B at any alignment
constexpr int PF_PITCH = 144;

// The staging step of pre_fused is its template argument: it fills s_in[c][r][q] (c = R, G, B) with fp16(float(u8) * fp32(1/255))
// of patch pixel (ix0 + q, iy0 + r), for every r with iy0 + r < H and q with ix0 + q < W.  Everything after it is shared.
//  PfBgr      u8 HWC BGR, the staging written out in the kernel body (its instruction sequence is that of the kernel before the
//             template: an inlined helper let hipcc pick another division sequence for e / PF_ROWDW)
//  Yuv420Src  I420 / NV12 planes: pf_stage below, the conversion rule of ycc_in.h at 8 bits
//  Ycc10Src   P010 / yuv420p10 / yuv422p10 planes: pf_stage10 below, the rule at 10 bits, fp16(float(code) * fp32(1/1023))
typedef const uint8_t *__restrict__ PfBgr;

// YUV staging.  Byte staging area: the horizontal pass's s_h (17.4 KB, unused until the barrier after staging), so the kernel's LDS
// and occupancy are those of the BGR form.  It holds the luma patch (44 rows x 140 bytes, pitch 144) and the chroma rows and columns
// that cover it with a one-sample halo, clamped at the frame edge: up to 25 rows x 72 samples per plane (I420: Cb at bytes 0..71 of
// a 144-byte row, Cr at 72..143; NV12: the CbCr pairs as they lie in memory).  Loads are whole aligned dwords that hold at least one
// byte of the segment (never a dword past a segment's last byte, whatever the plane's alignment and pitch); bytes outside it are
// dropped.  Then each patch pixel is converted once, two horizontally adjacent pixels (one chroma column) per item.
constexpr int PFY_PITCH = 144, PFY_DW = 36;              // 36 dwords cover 140 B at any alignment
constexpr int PFC_ROWS = 25, PFC_PITCH = 144, PFC_W = 72; // chroma rows / samples a patch needs at most (odd iy0 / ix0)
constexpr int PFC_DW1 = 19, PFC_DW2 = 37;                // dwords covering 72 B (an I420 plane row) / 144 B (an NV12 row)

__device__ __forceinline__ void pf_stage(const Yuv420Src &src, f16 (*s_in)[PF_IH][PF_PITCH], uint8_t *scratch, int tid, int H, int W,
                                         int ix0, int iy0)
{
    uint8_t *s_y = scratch, *s_c = scratch + PF_IH * PFY_PITCH;
    const bool nv12 = src.layout == YUV_NV12;
    const int Hc = H >> 1, Wc = W >> 1;
    const int ylast = min(iy0 + PF_IH, H) - 1, xlast = min(ix0 + PF_IW, W) - 1;
    const int jlo = max((iy0 >> 1) - 1, 0), jhi = min((ylast >> 1) + 1, Hc - 1);
    const int ilo = ix0 >> 1, ihi = min((xlast >> 1) + 1, Wc - 1);
    const int ylen = xlast - ix0 + 1, clen = (ihi - ilo + 1) << (nv12 ? 1 : 0);
    const int cdw = nv12 ? PFC_DW2 : PFC_DW1, nc = nv12 ? PFC_ROWS * PFC_DW2 : 2 * PFC_ROWS * PFC_DW1;
    constexpr int NY = PF_IH * PFY_DW;
    constexpr int NLD = (NY + 2 * PFC_ROWS * PFC_DW1 + 255) / 256;      // >= the NV12 count (25 x 37 < 2 x 25 x 19)
    uint32_t word[NLD];
    int rel[NLD], dst[NLD];                              // rel: byte offset of the dword from its segment's start (< -3: skip)
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + 256 * i;
        const uint8_t *seg = nullptr;
        int len = 0, d = 0;
        dst[i] = 0;
        if (e < NY) {
            const int r = e / PFY_DW;
            d = e - r * PFY_DW;
            if (iy0 + r < H) { seg = src.y + (size_t)(iy0 + r) * src.y_pitch + ix0; len = ylen; dst[i] = r * PFY_PITCH; }
        } else if (e < NY + nc) {
            const int e2 = e - NY, plane = e2 / (PFC_ROWS * cdw), e3 = e2 - plane * (PFC_ROWS * cdw), rr = e3 / cdw;
            d = e3 - rr * cdw;
            if (jlo + rr <= jhi) {
                seg = (plane ? src.v : src.u) + (size_t)(jlo + rr) * src.c_pitch + (ilo << (nv12 ? 1 : 0));
                len = clen;
                dst[i] = PF_IH * PFY_PITCH + rr * PFC_PITCH + plane * PFC_W;
            }
        }
        const uintptr_t a = ((uintptr_t)seg & ~(uintptr_t)3) + 4 * (uintptr_t)d;
        const bool ok = seg != nullptr && a < (uintptr_t)seg + len;
        rel[i] = ok ? (int)(a - (uintptr_t)seg) : -1000;
        word[i] = ok ? *reinterpret_cast<const uint32_t *>(a) : 0u;
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = rel[i] + k;
            if (b >= 0 && b < (tid + 256 * i < NY ? ylen : clen)) scratch[dst[i] + b] = (uint8_t)(word[i] >> (8 * k));
        }
    }
    __syncthreads();
    const int cs = nv12 ? 2 : 1, co = nv12 ? 1 : PFC_W;
    const float k255 = (float)(1.0 / 255.0);
    for (int e = tid; e < PF_IH * PFC_W; e += 256) {
        const int r = e / PFC_W, p = e - r * PFC_W;
        const int y = iy0 + r, i = ilo + p, q0 = 2 * i - ix0;
        if (y >= H || i > ihi) continue;          // (i <= ihi: a chroma column the patch uses)
        int j, n, u4a, u4b, v4a, v4b;
        ycc_rows(y, Hc, false, j, n);
        const uint8_t *cj = s_c + (j - jlo) * PFC_PITCH, *cn = s_c + (n - jlo) * PFC_PITCH;
        ycc_walk<8>(cj, cn, cs * p, cs * (ycc_col2(i, ihi) - ilo), co, 0, u4a, u4b, v4a, v4b);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = q0 + h;
            if (q < 0 || q >= PF_IW || ix0 + q >= W) continue;
            uint32_t R, G, B;
            ycc_rule<8>(s_y[r * PFY_PITCH + q], h ? u4a + u4b : 2 * u4a, h ? v4a + v4b : 2 * v4a, src.k, R, G, B);
            s_in[0][r][q] = (f16)__fmul_rn((float)R, k255);
            s_in[1][r][q] = (f16)__fmul_rn((float)G, k255);
            s_in[2][r][q] = (f16)__fmul_rn((float)B, k255);
        }
    }
}

// 10-bit staging (Ycc10Src: P010 / yuv420p10 / yuv422p10).  At two bytes per sample the byte layout above
// would need 19.9 KB, more than s_h holds, so the luma patch does not go there: its raw sample words are staged straight into
// s_in[0] (an f16 slot is 16 bits; the convert step reads the word of a patch pixel and overwrites it with that pixel's R, the same
// work item doing both).  s_h holds only the chroma rows, 288 bytes each: 25 rows for 4:2:0 (7.2 KB), 44 for 4:2:2 (12.7 KB), each
// Cb at samples 0..71 and Cr at 72..143 (planar) or the CbCr pairs as they lie in memory (P010).  So the kernel's LDS is that of the
// BGR form.  Loads keep pf_stage's discipline through ycc_in.h's ycc10_load / ycc10_keep (shared with letterbox10.hip): whole aligned dwords that hold at
// least one sample of the segment, never a dword past its last byte.  LDS accesses of the staging go
// through a may_alias type: the same addresses are f16 / float to the rest of the kernel.
typedef uint16_t __attribute__((may_alias)) pf_u16;
constexpr int PF10_YDW = 71;                              // 71 dwords cover 140 samples (280 B) at either alignment
constexpr int PF10_CPITCH = 144, PF10_CW = 72;            // u16 per staged chroma row / samples per plane in it
constexpr int PF10_CDW1 = 37, PF10_CDW2 = 73;             // dwords covering 144 B (a planar row) / 288 B (a P010 row)

__device__ __forceinline__ void pf_stage10(const Ycc10Src &src, f16 (*s_in)[PF_IH][PF_PITCH], pf_u16 *s_c, int tid, int H, int W,
                                           int ix0, int iy0)
{
    pf_u16 *s_y = reinterpret_cast<pf_u16 *>(&s_in[0][0][0]);
    const bool p010 = src.layout == YCC10_P010, c422 = src.layout == YCC10_YUV422P10;
    const int Hc = c422 ? H : H >> 1, Wc = W >> 1;
    const int ylast = min(iy0 + PF_IH, H) - 1, xlast = min(ix0 + PF_IW, W) - 1;
    const int jlo = c422 ? iy0 : max((iy0 >> 1) - 1, 0), jhi = c422 ? ylast : min((ylast >> 1) + 1, Hc - 1);
    const int ilo = ix0 >> 1, ihi = min((xlast >> 1) + 1, Wc - 1);
    const int ylen = xlast - ix0 + 1, clen = (ihi - ilo + 1) << (p010 ? 1 : 0);       // samples of a luma / chroma row segment
    {
        constexpr int NY = PF_IH * PF10_YDW, NLD = (NY + 255) / 256;
        uint32_t word[NLD];
        int rel[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i, r = e / PF10_YDW, d = e - r * PF10_YDW;
            const uint16_t *seg = nullptr;
            if (e < NY && iy0 + r < H)
                seg = row_of(src.y, iy0 + r, src.y_pitch) + ix0;
            ycc10_load(seg, ylen, d, word[i], rel[i]);
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int r = (tid + 256 * i) / PF10_YDW;
            ycc10_keep(s_y + r * PF_PITCH, ylen, word[i], rel[i]);
        }
    }
    {
        // a chroma row = 74 dwords (two planar segments) or 73 (one P010 segment); rows beyond jhi load nothing
        constexpr int NLD = (PF_IH * 2 * PF10_CDW1 + 255) / 256;           // >= the P010 count (44 x 73 < 44 x 74)
        uint32_t word[NLD];
        int rel[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            const int rr = p010 ? e / PF10_CDW2 : e / (2 * PF10_CDW1), rem = e - rr * (p010 ? PF10_CDW2 : 2 * PF10_CDW1);
            const int plane = (!p010 && rem >= PF10_CDW1) ? 1 : 0, d = rem - plane * PF10_CDW1;
            const uint16_t *seg = nullptr;
            if (jlo + rr <= jhi)
                seg = row_of(plane ? src.v : src.u, jlo + rr, src.c_pitch) + (ilo << (p010 ? 1 : 0));
            ycc10_load(seg, clen, d, word[i], rel[i]);
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            const int rr = p010 ? e / PF10_CDW2 : e / (2 * PF10_CDW1), rem = e - rr * (p010 ? PF10_CDW2 : 2 * PF10_CDW1);
            const int plane = (!p010 && rem >= PF10_CDW1) ? 1 : 0;
            if (rel[i] > -1000) ycc10_keep(s_c + rr * PF10_CPITCH + plane * PF10_CW, clen, word[i], rel[i]);
        }
    }
    __syncthreads();
    const int cs = p010 ? 2 : 1, co = p010 ? 1 : PF10_CW, sh = p010 ? 6 : 0;
    const float k1023 = (float)(1.0 / 1023.0);
    for (int e = tid; e < PF_IH * PF10_CW; e += 256) {
        const int r = e / PF10_CW, p = e - r * PF10_CW;
        const int y = iy0 + r, i = ilo + p, q0 = 2 * i - ix0;
        if (y >= H || i > ihi) continue;          // (i <= ihi: a chroma column the patch uses)
        int j, n, u4a, u4b, v4a, v4b;
        ycc_rows(y, Hc, c422, j, n);
        const pf_u16 *cj = s_c + (j - jlo) * PF10_CPITCH, *cn = s_c + (n - jlo) * PF10_CPITCH;
        ycc_walk<10>(cj, cn, cs * p, cs * (ycc_col2(i, ihi) - ilo), co, sh, u4a, u4b, v4a, v4b);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = q0 + h;
            if (q < 0 || q >= PF_IW || ix0 + q >= W) continue;
            uint32_t R, G, B;
            ycc_rule<10>(ycc_sample<10>(s_y[r * PF_PITCH + q], sh), h ? u4a + u4b : 2 * u4a, h ? v4a + v4b : 2 * v4a, src.k, R, G, B);
            s_in[0][r][q] = (f16)__fmul_rn((float)R, k1023);
            s_in[1][r][q] = (f16)__fmul_rn((float)G, k1023);
            s_in[2][r][q] = (f16)__fmul_rn((float)B, k1023);
        }
    }
}

template <typename Src>
__global__ __launch_bounds__(256) void pre_fused_kernel(const Src src, f16 *__restrict__ out, f16 *__restrict__ cond, int H, int W,
                                                        int Ho, int Wo, const float *__restrict__ wx, const int *__restrict__ xmn,
                                                        const int *__restrict__ xns, const float *__restrict__ wy,
                                                        const int *__restrict__ ymn, const int *__restrict__ yns, int mode)
{
    __shared__ __attribute__((aligned(16))) f16 s_in[3][PF_IH][PF_PITCH];     // 288-byte rows: 16-byte reads at columns 8k
    __shared__ float s_h[3][PF_IH][PF_OW + 1];
    __shared__ float s_wx[PF_OW][AA_TAPS], s_wy[PF_OH][AA_TAPS];      // this tile's tap tables (pitch 17: conflict-free across outputs)
    __shared__ int s_xb[PF_OW], s_xn[PF_OW], s_yb[PF_OH], s_yn[PF_OH];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * PF_OW, oy0 = blockIdx.y * PF_OH;
    const int ix0 = xmn[ox0], iy0 = ymn[oy0];
    for (int e = tid; e < PF_OW * AA_TAPS; e += 256) {
        const int o = e / AA_TAPS;
        s_wx[o][e - o * AA_TAPS] = ox0 + o < Wo ? wx[(size_t)(ox0 + o) * AA_TAPS + (e - o * AA_TAPS)] : 0.f;
    }
    if (tid < PF_OH * AA_TAPS) {
        const int o = tid / AA_TAPS;
        s_wy[o][tid - o * AA_TAPS] = oy0 + o < Ho ? wy[(size_t)(oy0 + o) * AA_TAPS + (tid - o * AA_TAPS)] : 0.f;
    }
    if (tid < PF_OW) { const bool in = ox0 + tid < Wo; s_xb[tid] = in ? xmn[ox0 + tid] - ix0 : 0; s_xn[tid] = in ? xns[ox0 + tid] : 0; }
    if (tid >= 64 && tid < 64 + PF_OH) { const int o = tid - 64; const bool in = oy0 + o < Ho; s_yb[o] = in ? ymn[oy0 + o] - iy0 : 0; s_yn[o] = in ? yns[oy0 + o] : 0; }
    if constexpr (std::is_same<Src, PfBgr>::value) {
        const size_t total = (size_t)H * W * 3;
        const float k255 = (float)(1.0 / 255.0);
        // all of this thread's dword loads first (19 independent loads in flight), then the byte unpacking: a loop that loads and
        // unpacks one dword at a time pays one HBM round trip per dword
        constexpr int NLD = (PF_IH * PF_ROWDW + 255) / 256;
        uint32_t word[NLD];
        long rel[NLD];                                     // byte offset of the dword's first byte from its row segment's start; < -3: skip
    #pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            const int r = e / PF_ROWDW, d = e - r * PF_ROWDW;
            const int iy = iy0 + r;
            const size_t row0 = ((size_t)(iy < H ? iy : 0) * W + ix0) * 3;
            const size_t addr = (row0 & ~(size_t)3) + 4 * (size_t)d;
            const bool ok = e < PF_IH * PF_ROWDW && iy < H && addr < total;
            rel[i] = ok ? (long)addr - (long)row0 : -1000;
            word[i] = 0;
            if (ok) {
                if (addr + 4 <= total) {
                    word[i] = *reinterpret_cast<const uint32_t *>(src + addr);
                } else {
                    for (size_t k = 0; addr + k < total; ++k) word[i] |= (uint32_t)src[addr + k] << (8 * k);
                }
            }
        }
    #pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            const int r = e / PF_ROWDW;
    #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = (int)rel[i] + k;
                if (b >= 0 && b < PF_IW * 3) {
                    const int q = (b * 683) >> 11, ch = b - 3 * q;             // b / 3 for b < 600
                    if (ix0 + q < W) s_in[2 - ch][r][q] = (f16)__fmul_rn((float)((word[i] >> (8 * k)) & 0xff), k255);
                }
            }
        }
    } else if constexpr (std::is_same<Src, Yuv420Src>::value) {
        pf_stage(src, s_in, reinterpret_cast<uint8_t *>(&s_h[0][0][0]), tid, H, W, ix0, iy0);
    } else {
        pf_stage10(src, s_in, reinterpret_cast<pf_u16 *>(&s_h[0][0][0]), tid, H, W, ix0, iy0);
    }
    __syncthreads();
    // ---- the pixels this tile owns -> f16 planes.  The last tile of a row / column also owns the W % 4 (H % 4) remainder.
    const int wx0 = 4 * ox0, wy0 = 4 * oy0;
    const int wx1 = (ox0 + PF_OW >= Wo) ? W : wx0 + 4 * PF_OW, wy1 = (oy0 + PF_OH >= Ho) ? H : wy0 + 4 * PF_OH;
    constexpr int NCX = 4 * PF_OW / 8 + 1, NRY = 4 * PF_OH + 3;
    const size_t npix = (size_t)H * W;
    for (int e = tid; e < 3 * NRY * NCX; e += 256) {
        const int c = e / (NRY * NCX), rr = (e / NCX) % NRY, j = e % NCX;
        const int y = wy0 + rr, x = wx0 + 8 * j;
        if (y >= wy1 || x >= wx1) continue;
        const f16 *src = &s_in[c][y - iy0][x - ix0];
        f16 *dst = out + c * npix + (size_t)y * W + x;
        if (x + 8 <= wx1) {
            f16x8 v;
            if (((x - ix0) & 1) == 0) {            // (always, for the 0.25x tables: xmn is even) four dword reads
                const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
                i32x4 u;
#pragma unroll
                for (int i = 0; i < 4; ++i) u[i] = (int)s32[i];
                v = __builtin_bit_cast(f16x8, u);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = src[i];
            }
            *reinterpret_cast<f16x8 *>(dst) = v;
        } else {
            for (int i = 0; x + i < wx1; ++i) dst[i] = src[i];
        }
    }
    if (mode == 2) {
        for (int e = tid; e < 3 * PF_OH * PF_OW; e += 256) {
            const int c = e / (PF_OH * PF_OW), r = (e / PF_OW) % PF_OH, o = e % PF_OW;
            if (ox0 + o < Wo && oy0 + r < Ho) cond[((size_t)c * Ho + oy0 + r) * Wo + ox0 + o] = (f16)0.f;
        }
        return;
    }
    if (mode == 1) {
        for (int e = tid; e < 3 * PF_OH * PF_OW; e += 256) {
            const int c = e / (PF_OH * PF_OW), r = (e / PF_OW) % PF_OH, o = e % PF_OW;
            const int ox = ox0 + o, oy = oy0 + r;
            if (ox < Wo && oy < Ho) {
                const int y1 = 4 * oy + 1, x1 = 4 * ox + 1;
                const int yp = y1 < H - 1 ? 1 : 0, xp = x1 < W - 1 ? 1 : 0;
                const float a = (float)s_in[c][y1 - iy0][x1 - ix0], b = (float)s_in[c][y1 - iy0][x1 + xp - ix0];
                const float cc = (float)s_in[c][y1 + yp - iy0][x1 - ix0], dd = (float)s_in[c][y1 + yp - iy0][x1 + xp - ix0];
                // upsample_bilinear2d: h0lambda * (w0lambda * a + w1lambda * b) + h1lambda * (w0lambda * c + w1lambda * d), lambdas 0.5
                const float top = __fadd_rn(__fmul_rn(0.5f, a), __fmul_rn(0.5f, b)), bot = __fadd_rn(__fmul_rn(0.5f, cc), __fmul_rn(0.5f, dd));
                cond[((size_t)c * Ho + oy) * Wo + ox] = (f16)__fadd_rn(__fmul_rn(0.5f, top), __fmul_rn(0.5f, bot));
            }
        }
        return;
    }
    // horizontal pass: a thread owns the four adjacent outputs o0 .. o0 + 3 (o0 = 4 * (tid % 8), the same in every trip: their
    // 4 x 16 weights stay in registers) of one row per trip.  Interior outputs -- 16 taps each, windows 4 samples apart -- read
    // their 28 samples as four 16-byte LDS reads instead of 64 two-byte gathers; anything else (image borders) goes tap by tap.
    // Either way: fp32, taps in order, separate multiply and add (ATen's _upsample_bicubic2d_aa, as cond_resize_kernel).
    {
        const int o0 = 4 * (tid & 7);
        float wv[4][16];
        int xb[4], xn1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xb[i] = s_xb[o0 + i]; xn1[i] = s_xn[o0 + i] - 1;     // n1 < 0 for outputs beyond the image
#pragma unroll
            for (int j = 0; j < 16; ++j) wv[i][j] = s_wx[o0 + i][j];
        }
        const int wstart = xb[0] & ~7, d = xb[0] - wstart;
        const bool fast = (d == 0 || d == 2) && xn1[0] == 15 && xn1[1] == 15 && xn1[2] == 15 && xn1[3] == 15 &&
                          xb[1] == xb[0] + 4 && xb[2] == xb[0] + 8 && xb[3] == xb[0] + 12;
        for (int e = tid >> 3; e < 3 * PF_IH; e += 32) {
            const int c = e / PF_IH, r = e - c * PF_IH;
            float sacc[4] = {0.f, 0.f, 0.f, 0.f};
            if (iy0 + r < H) {
                if (fast) {
                    const f16x8 *src = reinterpret_cast<const f16x8 *>(&s_in[c][r][wstart]);
                    const f16x8 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
                    float xv[32];
#pragma unroll
                    for (int k = 0; k < 8; ++k) { xv[k] = (float)q0[k]; xv[8 + k] = (float)q1[k]; xv[16 + k] = (float)q2[k]; xv[24 + k] = (float)q3[k]; }
                    if (d == 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 16; ++j) sacc[i] = __fadd_rn(sacc[i], __fmul_rn(wv[i][j], xv[4 * i + j]));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 16; ++j) sacc[i] = __fadd_rn(sacc[i], __fmul_rn(wv[i][j], xv[2 + 4 * i + j]));
                    }
                } else {
                    // taps beyond an output's count have weight 0 in the table and re-read the last valid sample: they add exactly +0
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (xn1[i] >= 0) {
                            float xv[16];
#pragma unroll
                            for (int j = 0; j < 16; ++j) xv[j] = (float)s_in[c][r][xb[i] + (j < xn1[i] ? j : xn1[i])];
#pragma unroll
                            for (int j = 0; j < 16; ++j) sacc[i] = __fadd_rn(sacc[i], __fmul_rn(wv[i][j], xv[j]));
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) s_h[c][r][o0 + i] = sacc[i];
        }
    }
    __syncthreads();
    for (int e = tid; e < 3 * PF_OH * PF_OW; e += 256) {
        const int c = e / (PF_OH * PF_OW), r = (e / PF_OW) % PF_OH, o = e % PF_OW;
        const int ox = ox0 + o, oy = oy0 + r;
        if (ox < Wo && oy < Ho) {
            const int base = s_yb[r], n1 = s_yn[r] - 1;
            float sacc = 0.f, xv[16], wv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) { xv[j] = s_h[c][base + (j < n1 ? j : n1)][o]; wv[j] = s_wy[r][j]; }
#pragma unroll
            for (int j = 0; j < 16; ++j) sacc = __fadd_rn(sacc, __fmul_rn(wv[j], xv[j]));
            cond[((size_t)c * Ho + oy) * Wo + ox] = (f16)sacc;
        }
    }
}

// ---- post-process quantisers ----------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load8(const T *p, float (&v)[8]);
template <>
__device__ __forceinline__ void load8<f16>(const f16 *p, float (&v)[8])
{
    const f16x8 x = *reinterpret_cast<const f16x8 *>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
}
template <>
__device__ __forceinline__ void load8<float>(const float *p, float (&v)[8])
{
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// u8: the reference quantises in the tensor's own dtype (fp16 model: every op rounds to fp16).
template <typename T>
__device__ __forceinline__ uint32_t quant_u8(float x)
{
    if (sizeof(T) == 2) {
        const f16 c = (f16)clamp01(x);
        const f16 m = (f16)__fmul_rn((float)c, 255.f);
        const f16 a = (f16)__fadd_rn((float)m, 0.5f);
        return (uint32_t)(int)(float)a & 0xff;
    }
    return (uint32_t)(int)__fadd_rn(__fmul_rn(clamp01(x), 255.f), 0.5f) & 0xff;
}

template <typename T>
__global__ __launch_bounds__(256) void post_u8_kernel(const T *__restrict__ in, uint8_t *__restrict__ bgr, size_t npix)
{
    const size_t ngrp = npix / 8;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += (size_t)gridDim.x * blockDim.x) {
        float r[8], gg[8], b[8];
        load8<T>(in + g * 8, r);
        load8<T>(in + npix + g * 8, gg);
        load8<T>(in + 2 * npix + g * 8, b);
        uint32_t w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = i * 3;
            w[o >> 2] |= quant_u8<T>(b[i]) << ((o & 3) * 8);
            w[(o + 1) >> 2] |= quant_u8<T>(gg[i]) << (((o + 1) & 3) * 8);
            w[(o + 2) >> 2] |= quant_u8<T>(r[i]) << (((o + 2) & 3) * 8);
        }
        uint2 *dst = reinterpret_cast<uint2 *>(bgr + g * 24);
        dst[0] = make_uint2(w[0], w[1]);
        dst[1] = make_uint2(w[2], w[3]);
        dst[2] = make_uint2(w[4], w[5]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (npix & 7)) {
        const size_t i = ngrp * 8 + threadIdx.x;
        bgr[i * 3 + 0] = (uint8_t)quant_u8<T>((float)in[2 * npix + i]);
        bgr[i * 3 + 1] = (uint8_t)quant_u8<T>((float)in[npix + i]);
        bgr[i * 3 + 2] = (uint8_t)quant_u8<T>((float)in[i]);
    }
}

// PQ constants: gui_objective_metrics.py:63-67
#define PQ_M1 0.1593017578125f
#define PQ_M2 78.84375f
#define PQ_C1 0.8359375f
#define PQ_C2 18.8515625f
#define PQ_C3 18.6875f

__device__ __forceinline__ float pq_oetf(float nits)
{
    float y = nits / 10000.f;
    y = fminf(fmaxf(y, 0.f), 1.f);
    const float yp = powf(y, PQ_M1);
    return powf((PQ_C1 + PQ_C2 * yp) / (1.f + PQ_C3 * yp), PQ_M2);
}

template <typename T, bool PQ>
__global__ __launch_bounds__(256) void post_rgb48_kernel(const T *__restrict__ in, uint16_t *__restrict__ rgb,
                                                         size_t npix, float peak, const float *__restrict__ bnd)
{
    const size_t ngrp = npix / 8;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngrp; g += (size_t)gridDim.x * blockDim.x) {
        float r[8], gg[8], b[8];
        load8<T>(in + g * 8, r);
        load8<T>(in + npix + g * 8, gg);
        load8<T>(in + 2 * npix + g * 8, b);
        uint32_t w[12];
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            uint32_t q[6];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                quant_rgb<PQ>(r[i + k], gg[i + k], b[i + k], peak, bnd, q[k * 3], q[k * 3 + 1], q[k * 3 + 2]);
            }
            w[(i / 2) * 3 + 0] = q[0] | (q[1] << 16);
            w[(i / 2) * 3 + 1] = q[2] | (q[3] << 16);
            w[(i / 2) * 3 + 2] = q[4] | (q[5] << 16);
        }
        uint4 *dst = reinterpret_cast<uint4 *>(rgb + g * 24);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
        dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (npix & 7)) {
        const size_t i = ngrp * 8 + threadIdx.x;
        uint32_t q[3];
        quant_rgb<PQ>((float)in[i], (float)in[npix + i], (float)in[2 * npix + i], peak, bnd, q[0], q[1], q[2]);
        for (int ch = 0; ch < 3; ++ch) rgb[i * 3 + ch] = (uint16_t)q[ch];
    }
}

inline int ew_grid(size_t ngrp)
{
    size_t g = (ngrp + 255) / 256;
    if (g > 2048) g = 2048;   // 256 CUs x 8 blocks, grid-stride beyond (guide: Guideline 11)
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

hipError_t pre_unpack_launch(const uint8_t *bgr, f16 *out, int H, int W, hipStream_t s)
{
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(pre_unpack_kernel, dim3(ew_grid(npix / 8)), dim3(256), 0, s, bgr, out, npix);
    return hipGetLastError();
}

hipError_t cond_resize_launch(const f16 *in, f16 *out, int H, int W, int Ho, int Wo, const AaTables &t, hipStream_t s)
{
    dim3 grid((Wo + RT_W - 1) / RT_W, (Ho + RT_H - 1) / RT_H, 3);
    hipLaunchKernelGGL(cond_resize_kernel, grid, dim3(256), 0, s, in, out, H, W, Ho, Wo, t.wx, t.xmn, t.xns, t.wy, t.ymn, t.yns);
    return hipGetLastError();
}

// mode 0: 0.25x antialiased bicubic; 1: bilinear (fast_condition_resize); 2: zero condition.  Needs Ho = H / 4 >= 1, Wo = W / 4 >= 1.
template <typename Src>
static hipError_t pre_fused_any(const Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s)
{
    if (Ho != H / 4 || Wo != W / 4 || Ho < 1 || Wo < 1) return hipErrorInvalidValue;
    const dim3 grid((Wo + PF_OW - 1) / PF_OW, (Ho + PF_OH - 1) / PF_OH, 1);
    hipLaunchKernelGGL(pre_fused_kernel<Src>, grid, dim3(256), 0, s, src, out, cond, H, W, Ho, Wo, t.wx, t.xmn, t.xns, t.wy, t.ymn, t.yns, mode);
    return hipGetLastError();
}

hipError_t pre_fused_launch(const uint8_t *bgr, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s)
{
    return pre_fused_any<PfBgr>(bgr, out, cond, H, W, Ho, Wo, t, mode, s);
}

hipError_t pre_fused_yuv_launch(const Yuv420Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s)
{
    if ((H & 1) || (W & 1)) return hipErrorInvalidValue;
    return pre_fused_any(src, out, cond, H, W, Ho, Wo, t, mode, s);
}

hipError_t pre_fused_ycbcr10_launch(const Ycc10Src &src, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s)
{
    if (!ycc_ok(src, H, W)) return hipErrorInvalidValue;
    return pre_fused_any(src, out, cond, H, W, Ho, Wo, t, mode, s);
}

hipError_t post_u8_launch(const void *in, int is_f32, int H, int W, uint8_t *bgr, hipStream_t s)
{
    const size_t npix = (size_t)H * W;
    if (is_f32)
        hipLaunchKernelGGL(post_u8_kernel<float>, dim3(ew_grid(npix / 8)), dim3(256), 0, s, (const float *)in, bgr, npix);
    else
        hipLaunchKernelGGL(post_u8_kernel<f16>, dim3(ew_grid(npix / 8)), dim3(256), 0, s, (const f16 *)in, bgr, npix);
    return hipGetLastError();
}

// pq != 0 needs pq_bnd: device table of the 65536 code boundaries (entry 0 unused)
hipError_t post_rgb48_launch(const void *in, int is_f32, int H, int W, uint16_t *rgb, int pq, float peak, hipStream_t s,
                             const float *pq_bnd)
{
    if (pq && !pq_bnd) return hipErrorInvalidValue;
    const size_t npix = (size_t)H * W;
    const dim3 g(ew_grid(npix / 8)), b(256);
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((post_rgb48_kernel<float, true>), g, b, 0, s, (const float *)in, rgb, npix, peak, pq_bnd);
        else hipLaunchKernelGGL((post_rgb48_kernel<float, false>), g, b, 0, s, (const float *)in, rgb, npix, peak, pq_bnd);
    } else {
        if (pq) hipLaunchKernelGGL((post_rgb48_kernel<f16, true>), g, b, 0, s, (const f16 *)in, rgb, npix, peak, pq_bnd);
        else hipLaunchKernelGGL((post_rgb48_kernel<f16, false>), g, b, 0, s, (const f16 *)in, rgb, npix, peak, pq_bnd);
    }
    return hipGetLastError();
}
