// post_down.hip -- hdrtv_post_rgb48_down (gfx950): quantise + shrink of the RGB48 output in one kernel, the other direction of
// post_scale.hip / post_fsr.hip: a Mitchell downscale of the u16 codes with the kernel stretched by the ratio (stage A, integer,
// anti-ringing as in post_scale_tile.h) and, with SSIM, the structure-preserving correction of the reference's display chain behind
// it (stage B, float32).  include/hdrtv_mi355x.h states the rule, tests/rgb48_down_ref.py restates it in NumPy; the device is held
// to that bit for bit, so every float operation of stage B is one rounded float32 operation: __fmul_rn / __fadd_rn / __fsub_rn /
// __fdiv_rn / sqrtf, no fused multiply-add (the file is built with -ffp-contract=off on top), denormals kept.  The two fused
// operations of down_sample are post_fsr.hip's fsr_sample, written as such.  The SSIM = false instances hold no float stage.
//
// No frame at the processing size goes to HBM: a workgroup of 256 lanes owns TH x TW output pixels and reads their source
// footprint from the model's tensor -- with SSIM the footprint of the tile and the two-pixel ring stage B reads around it (TRH x TRW
// = (TH + 4) x (TW + 4) positions; RG = 0, TRH x TRW = TH x TW without).  An output index d of an axis reads source taps
// lo(d) .. lo(d) + cnt(d) - 1, cnt <= 4 r + 1 for the ratio r = n / m <= RMAX, and both ends rise with d, so T neighbouring indices
// read at most (T + 3) RMAX + 1 source samples: SR x SC = ((TRH + 3) RMAX + 1) x ((TRW + 3) RMAX + 1).  The tile is sized by the
// ratio: 16 x 32 for r <= 2 on both axes (RMAX = 2), 8 x 32 up to 4 (RMAX = 4); DESIGN.md has the bytes.
//   1. stage    the footprint is read once, quantised once (quant_rgb, plain or PQ) and kept as u16 codes[ch][row][col]; an index
//               outside the frame reads the clamped pixel, so the taps never clamp.
//   2. stage A  per channel: the horizontal sums of every footprint row for the TRW columns, pulled towards their two inner taps,
//               to hor (int32); then the vertical sums (int64), pulled likewise, shifted and clamped to the Mitchell codes mc (u16).
//   3. L2       (SSIM) per channel: the vertical Catmull-Rom mean of s * s of every footprint column for the TRH rows to v1, then
//               the horizontal one to l2.
//   4. MR       (SSIM) for the tile and its one-pixel ring: the 3 x 3 means of Ms, Ms * Ms and L2, the variance ratio R; mM and R
//               are kept.
//   5. final    (SSIM) the 3 x 3 means of R mM, mM and R, the corrected pixel, the quantiser; without SSIM the codes mc.
// A position of the ring that lies outside the image is never computed: every neighbour is read at its clamped position, which
// lies inside the part of the ring that is (the image's edge is the tile's or lies beyond the ring).
// LDS, bytes, every array on a 16-byte boundary: LDS(SSIM, TH, TW, RMAX) = 2 * 3 * SR * SC (codes) + 4 * NU (hor / v1 / mM and R
// share one buffer, NU = max(SR * TRW, SSIM ? max(TRH * SC, 4 * (TH + 2) * (TW + 2)) : 0)) + 2 * 3 * TRH * TRW (mc) + (SSIM ?
// 4 * 3 * TRH * TRW : 0) (l2) + the tile's tables, with NT = 4 RMAX + 1 taps per index: 16 * (TRW + TRH) (xi, yi) + 2 * NT * TRW
// + 2 * NT * TRH (xq, yq) + (SSIM ? 4 * NT * TRW + 4 * NT * TRH : 0) (xw, yw): 26,320 / 48,976 bytes for RMAX = 2 without /
// with SSIM, 47,376 / 79,712 for RMAX = 4: two workgroups per CU at least, three or more for every instance but the last
// (tests/test_isa_post_down.py).
// Banks (MI355X_MICROARCH.md): in the passes a lane owns one output column and neighbouring lanes neighbouring columns; the reads
// of hor, v1, mc and l2 are consecutive dwords or halves, the reads of codes in the horizontal pass step by r <= 4 halves (at
// most two-way on the 32 banks of a 32-lane group at r = 4).
#include "launchers.h"
#include "post_quant.h"

namespace {

__device__ __forceinline__ float fm(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fa(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float fs(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float fd(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float sat(float a) { return fminf(fmaxf(a, 0.f), 1.f); }
// the correctly rounded square root: sqrtf, which hipcc rounds correctly unless told otherwise (__fsqrt_rn is the NATIVE, approximate
// root in this toolchain's headers unless OCML_BASIC_ROUNDED_OPERATIONS is defined)
__device__ __forceinline__ float fsq(float a) { return sqrtf(a); }

// u16 code -> float32(c / 65535), correctly rounded for every code (post_fsr.hip's fsr_sample; tests/test_rgb48_fsr_host.py)
__device__ __forceinline__ float down_sample(uint32_t c)
{
    constexpr float r = (float)(1.0 / 65535.0);
    const float x = (float)c;
    const float q = __fmul_rn(x, r);
    return __fmaf_rn(__fmaf_rn(-q, 65535.f, x), r, q);
}

// the 0.5 / 1 / 0.5 mean of three values: ((0.5 a + b) + 0.5 c) / 2 (the halving is exact, a multiply by 0.5 rounds as the division)
__device__ __forceinline__ float mean3(float a, float b, float c) { return fm(fa(fa(fm(0.5f, a), b), fm(0.5f, c)), 0.5f); }

__device__ __forceinline__ float luma(float r, float g, float b) { return fa(fa(fm(0.2126f, r), fm(0.7152f, g)), fm(0.0722f, b)); }

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <typename T, bool PQ, bool SSIM, int TH, int TW, int RMAX>
__global__ __launch_bounds__(256) void post_down_kernel(const PostDownParams p, const int a)
{
    constexpr int RG = SSIM ? 2 : 0, TRH = TH + 2 * RG, TRW = TW + 2 * RG;
    constexpr int SR = (TRH + 3) * RMAX + 1, SC = (TRW + 3) * RMAX + 1;
    constexpr int MH = TH + 2, MW = TW + 2;                                   // the tile and its one-pixel ring (MR)
    constexpr int NU = cmax(SR * TRW, SSIM ? cmax(TRH * SC, 4 * MH * MW) : 0);
    __shared__ uint16_t codes[3][SR][SC];
    __shared__ int ubuf[NU];
    __shared__ uint16_t mc[3][TRH][TRW];
    // the tile's slice of the tables: a tap loop that fetched its coefficients from global memory would wait for one load per tap
    constexpr int NT = 4 * RMAX + 1;                                          // taps of an index at a ratio of RMAX at most
    __shared__ int4 xi[TRW], yi[TRH];
    __shared__ short xq[TRW * NT], yq[TRH * NT];
    __shared__ float xw[SSIM ? TRW * NT : 1], yw[SSIM ? TRH * NT : 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int ox = x0 - RG, oy = y0 - RG;                                     // the ring's origin: position (y, x) is cell (y - oy, x - ox)
    const int xa = max(ox, 0), xb = min(x0 + TW - 1 + RG, p.dW - 1);
    const int ya = max(oy, 0), yb = min(y0 + TH - 1 + RG, p.dH - 1);
    const int nx = xb - xa + 1, ny = yb - ya + 1;
    const int xs0 = p.xinfo[xa].x, ys0 = p.yinfo[ya].x;
    const int nc = min(p.xinfo[xb].x + p.xinfo[xb].y - xs0, SC), nr = min(p.yinfo[yb].x + p.yinfo[yb].y - ys0, SR);

    // 0. the tables of the tile's columns xa .. xb and rows ya .. yb
    {
        const int ntx = min(p.ntx, NT), nty = min(p.nty, NT);
        if (tid < nx) xi[tid] = p.xinfo[xa + tid];
        if (tid < ny) yi[tid] = p.yinfo[ya + tid];
        for (int i = tid; i < nx * NT; i += 256) {
            const int j = i / NT, k = i - j * NT;
            if (k < ntx) {
                xq[i] = (short)p.xq[(size_t)(xa + j) * p.ntx + k];
                if constexpr (SSIM) xw[i] = p.xw[(size_t)(xa + j) * p.ntx + k];
            }
        }
        for (int i = tid; i < ny * NT; i += 256) {
            const int j = i / NT, k = i - j * NT;
            if (k < nty) {
                yq[i] = (short)p.yq[(size_t)(ya + j) * p.nty + k];
                if constexpr (SSIM) yw[i] = p.yw[(size_t)(ya + j) * p.nty + k];
            }
        }
    }

    // 1. stage + quantise
    {
        const T *__restrict__ in = static_cast<const T *>(p.in);
        const size_t plane = (size_t)p.H * p.W;
        for (int i = tid; i < nr * nc; i += 256) {
            const int r = i / nc, c = i - r * nc;
            const int sy = min(max(ys0 + r, 0), p.H - 1), sx = min(max(xs0 + c, 0), p.W - 1);
            const size_t o = (size_t)sy * p.W + sx;
            const float cr = (float)in[o], cg = (float)in[plane + o], cb = (float)in[2 * plane + o];
            uint32_t q0, q1, q2;
            quant_rgb<PQ>(cr, cg, cb, p.peak, p.pq_bnd, q0, q1, q2);
            codes[0][r][c] = (uint16_t)q0;
            codes[1][r][c] = (uint16_t)q1;
            codes[2][r][c] = (uint16_t)q2;
        }
    }
    __syncthreads();

    // 2. stage A, one channel at a time through hor
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        int *hor = ubuf;                                                      // [nr][TRW], column j = output column xa + j
#pragma unroll 1
        for (int i = tid; i < nr * nx; i += 256) {
            const int r = i / nx, j = i - r * nx;
            const int4 t = xi[j];
            const short *q = xq + j * NT;
            const uint16_t *row = &codes[ch][r][0];
            int raw = 0;
#pragma unroll 4
            for (int k = 0; k < t.y; ++k) raw += (int)row[t.x - xs0 + k] * q[k];
            const int t2 = row[t.z - xs0], t3 = row[t.w - xs0];
            const int lo = min(t2, t3) << 14, hi = max(t2, t3) << 14;
            const long long d = (long long)min(max(raw, lo), hi) - raw;
            hor[r * TRW + j] = raw + (int)((d * a + 128) >> 8);
        }
        __syncthreads();
#pragma unroll 1
        for (int i = tid; i < ny * nx; i += 256) {
            const int r = i / nx, j = i - r * nx;
            const int4 t = yi[r];
            const short *q = yq + r * NT;
            const int *col = hor + (t.x - ys0) * TRW + j;
            long long raw = 0;
#pragma unroll 4
            for (int k = 0; k < t.y; ++k) raw += (long long)col[k * TRW] * q[k];
            const long long t2 = hor[(t.z - ys0) * TRW + j], t3 = hor[(t.w - ys0) * TRW + j];
            const long long lo = (t2 < t3 ? t2 : t3) << 14, hi = (t2 < t3 ? t3 : t2) << 14;
            const long long d = (raw < lo ? lo : raw > hi ? hi : raw) - raw;
            const long long v = (raw + ((d * a + 128) >> 8) + (1ll << 27)) >> 28;
            mc[ch][ya - oy + r][xa - ox + j] = (uint16_t)(v < 0 ? 0 : v > 65535 ? 65535 : v);
        }
        __syncthreads();
    }

    if constexpr (!SSIM) {
        // 5. store the Mitchell codes
        for (int i = tid; i < TH * TW; i += 256) {
            const int ly = i / TW, lx = i - ly * TW;
            if (y0 + ly >= p.dH || x0 + lx >= p.dW) continue;
            uint16_t *d = p.dst + ((size_t)(y0 + ly) * p.dW + x0 + lx) * 3;
            d[0] = mc[0][ly][lx];
            d[1] = mc[1][ly][lx];
            d[2] = mc[2][ly][lx];
        }
    } else {
        __shared__ float l2[3][TRH][TRW];
        // 3. L2, one channel at a time through v1
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            float *v1 = reinterpret_cast<float *>(ubuf);                      // [ny][SC], column c = footprint column c
#pragma unroll 1
            for (int i = tid; i < ny * nc; i += 256) {
                const int r = i / nc, c = i - r * nc;
                const int4 t = yi[r];
                const float *w = yw + r * NT;
                float acc = 0.f;
#pragma unroll 4
                for (int k = 0; k < t.y; ++k) {
                    const float s = down_sample(codes[ch][t.x - ys0 + k][c]);
                    acc = fa(acc, fm(w[k], fm(s, s)));
                }
                v1[r * SC + c] = acc;
            }
            __syncthreads();
#pragma unroll 1
            for (int i = tid; i < ny * nx; i += 256) {
                const int r = i / nx, j = i - r * nx;
                const int4 t = xi[j];
                const float *w = xw + j * NT;
                const float *row = v1 + r * SC + (t.x - xs0);
                float acc = 0.f;
#pragma unroll 4
                for (int k = 0; k < t.y; ++k) acc = fa(acc, fm(w[k], row[k]));
                l2[ch][ya - oy + r][xa - ox + j] = acc;
            }
            __syncthreads();
        }

        // 4. MR of the tile and its one-pixel ring, the positions inside the image: mM[ch] and R to mr[4][MH][MW]
        float *mr = reinterpret_cast<float *>(ubuf);
        const float sigma = (float)(10.0 / (255.0 * 255.0));
        {
            const int ma = max(y0 - 1, 0), mb = min(y0 + TH, p.dH - 1), la = max(x0 - 1, 0), lb = min(x0 + TW, p.dW - 1);
            const int mw = lb - la + 1, mn = (mb - ma + 1) * mw;
#pragma unroll 1
            for (int i = tid; i < mn; i += 256) {
                const int r = i / mw, y = ma + r, x = la + (i - r * mw);
                const int cy[3] = {max(y - 1, 0) - oy, y - oy, min(y + 1, p.dH - 1) - oy};
                const int cx[3] = {max(x - 1, 0) - ox, x - ox, min(x + 1, p.dW - 1) - ox};
                float mm[3], sl[3], sh[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float hm[3], hq[3], hl[3];
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const float s0 = down_sample(mc[ch][cy[v]][cx[0]]), s1 = down_sample(mc[ch][cy[v]][cx[1]]),
                                    s2 = down_sample(mc[ch][cy[v]][cx[2]]);
                        hm[v] = mean3(s0, s1, s2);
                        hq[v] = mean3(fm(s0, s0), fm(s1, s1), fm(s2, s2));
                        hl[v] = mean3(l2[ch][cy[v]][cx[0]], l2[ch][cy[v]][cx[1]], l2[ch][cy[v]][cx[2]]);
                    }
                    mm[ch] = mean3(hm[0], hm[1], hm[2]);
                    const float sq = fm(mm[ch], mm[ch]);
                    sl[ch] = fmaxf(fs(mean3(hq[0], hq[1], hq[2]), sq), 0.f);
                    sh[ch] = fmaxf(fs(mean3(hl[0], hl[1], hl[2]), sq), 0.f);
                }
                const float Sl = luma(sl[0], sl[1], sl[2]), Sh = luma(sh[0], sh[1], sh[2]);
                const float R = Sl > Sh ? sat(fd(Sh, Sl)) : fsq(fd(fa(Sh, sigma), fa(Sl, sigma)));
                const int o = (y - (y0 - 1)) * MW + (x - (x0 - 1));
                mr[o] = mm[0];
                mr[MH * MW + o] = mm[1];
                mr[2 * MH * MW + o] = mm[2];
                mr[3 * MH * MW + o] = R;
            }
        }
        __syncthreads();

        // 5. final pass + quantise + store
#pragma unroll 1
        for (int i = tid; i < TH * TW; i += 256) {
            const int ly = i / TW, lx = i - ly * TW;
            const int y = y0 + ly, x = x0 + lx;
            if (y >= p.dH || x >= p.dW) continue;
            const int cy[3] = {max(y - 1, 0) - (y0 - 1), ly + 1, min(y + 1, p.dH - 1) - (y0 - 1)};
            const int cx[3] = {max(x - 1, 0) - (x0 - 1), lx + 1, min(x + 1, p.dW - 1) - (x0 - 1)};
            float R[3][3], h[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
#pragma unroll
                for (int u = 0; u < 3; ++u) R[v][u] = mr[3 * MH * MW + cy[v] * MW + cx[u]];
                h[v] = mean3(R[v][0], R[v][1], R[v][2]);
            }
            const float a2 = mean3(h[0], h[1], h[2]);
            uint16_t *d = p.dst + ((size_t)y * p.dW + x) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float *m = mr + ch * MH * MW;
                float h0[3], h1[3];
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const float m0 = m[cy[v] * MW + cx[0]], m1 = m[cy[v] * MW + cx[1]], m2 = m[cy[v] * MW + cx[2]];
                    h0[v] = mean3(fm(R[v][0], m0), fm(R[v][1], m1), fm(R[v][2], m2));
                    h1[v] = mean3(m0, m1, m2);
                }
                const float a0 = mean3(h0[0], h0[1], h0[2]), a1 = mean3(h1[0], h1[1], h1[2]);
                const float ms = down_sample(mc[ch][ly + RG][lx + RG]);
                d[ch] = (uint16_t)quant_u16(sat(fs(fa(a1, fm(a2, ms)), a0)));
            }
        }
    }
}

template <typename T, bool PQ, bool SSIM>
void launch(const PostDownParams &p, int a, bool wide, hipStream_t s)
{
    if (wide) {
        const dim3 g((p.dW + DN_TW - 1) / DN_TW, (p.dH + DN_TH4 - 1) / DN_TH4);
        hipLaunchKernelGGL((post_down_kernel<T, PQ, SSIM, DN_TH4, DN_TW, 4>), g, dim3(256), 0, s, p, a);
    } else {
        const dim3 g((p.dW + DN_TW - 1) / DN_TW, (p.dH + DN_TH2 - 1) / DN_TH2);
        hipLaunchKernelGGL((post_down_kernel<T, PQ, SSIM, DN_TH2, DN_TW, 2>), g, dim3(256), 0, s, p, a);
    }
}

template <typename T, bool PQ>
void launch(const PostDownParams &p, int a, int ssim, bool wide, hipStream_t s)
{
    if (ssim) launch<T, PQ, true>(p, a, wide, s);
    else launch<T, PQ, false>(p, a, wide, s);
}

}  // namespace

hipError_t post_down_launch(const PostDownParams &p, int antiring, int ssim, int is_f32, int pq, hipStream_t s)
{
    if (p.dH < 1 || p.dW < 1 || p.dH > p.H || p.dW > p.W || 4 * (long long)p.dH < p.H || 4 * (long long)p.dW < p.W || p.ntx < 1 ||
        p.ntx > 17 || p.nty < 1 || p.nty > 17 || antiring < 0 || antiring > 256 || (pq && !p.pq_bnd))
        return hipErrorInvalidValue;
    const bool wide = 2 * (long long)p.dH < p.H || 2 * (long long)p.dW < p.W;      // a ratio above 2 on an axis: the small tile
    if (is_f32) {
        if (pq) launch<float, true>(p, antiring, ssim, wide, s);
        else launch<float, false>(p, antiring, ssim, wide, s);
    } else {
        if (pq) launch<f16, true>(p, antiring, ssim, wide, s);
        else launch<f16, false>(p, antiring, ssim, wide, s);
    }
    return hipGetLastError();
}
