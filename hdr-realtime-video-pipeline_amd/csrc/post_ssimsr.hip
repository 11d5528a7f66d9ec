// post_ssimsr.hip -- hdrtv_post_rgb48_ssimsr (gfx950): quantise + enlargement of the RGB48 output in one kernel, the third scaler of
// the reference's display chain beside post_scale.hip (Lanczos) and post_fsr.hip (FSR): a spline36 upscale of the u16 codes (stage A,
// the integer rule of post_scale.hip with another kernel and no anti-ringing) and, with SSIM, the four passes of the reference's
// SSimSuperRes shader behind it (stage B, float32).  include/hdrtv_mi355x.h states the rule, tests/rgb48_ssimsr_ref.py restates it in
// NumPy; the device is held to that bit for bit, so every float operation of stage B is one rounded float32 operation: __fmul_rn /
// __fadd_rn / __fsub_rn / __fdiv_rn / sqrtf, no fused multiply-add (the file is built with -ffp-contract=off on top), denormals kept.
// The two fused operations of sr_sample are post_fsr.hip's fsr_sample, written as such.  No cosine is evaluated here: the Hann weights
// come from the host's tables.  The SSIM = false instances hold no float stage.
//
// No frame-sized intermediate goes to HBM: a workgroup of 256 lanes owns SR_TH x SR_TW = 16 x 32 output pixels d0 .. d1 per axis and
// keeps, per axis with n source and m destination samples, r = m / n in (1, 2] (each region clamped to its frame; an index outside a
// frame reads the clamped pixel, which lies inside the clamped region because every table below rises with its index):
//   F  low-resolution pixels ip(d0) - 1 .. ip(d1) + 1, the 3 x 3 taps of the final pass: var is computed here.  ip(d1) - ip(d0) <=
//      ceil((T - 1) / r), so at most T + 2 of them.
//   L  F and one more pixel on either side, the cross neighbours of var: pass I and pass II are computed here.  At most
//      NL = ceil((T - 1) / r) + 5 <= T + 4 = sr_nl(T).
//   P  high-resolution pixels lo(L first) .. hi(L last), the footprints of the two low-resolution passes (the step-4 footprint of a
//      low pixel spans its centre +- 2 r, which holds the tile's own pixels and the two columns of pass II's linear fetch): the
//      spline36 codes are computed here.  At most (NL - 1) r + 4 r + 1 < T + 9 r <= T + 18 = sr_np(T).
//   C  source pixels i0(P first) - 2 .. i0(P last) + 3, the six spline36 taps: the model's tensor is read and quantised here.  At
//      most ceil((NP - 1) / r) + 6 <= NL + 9 <= T + 13 (sr_nc(T) = T + 14); it holds L, whose samples var and the final pass read.
// Without SSIM P is the tile and C its taps, at most T + 5.  hdrtv_api.hip checks every one of these bounds and containments on the
// host's tables of a geometry before its first launch.  The halo is largest in high-resolution pixels at 2x (P = 34 x 50 for 16 x 32
// outputs) and in low-resolution pixels next to 1x (L = 20 x 36).
//   0. tables   the slices of the host's tables that belong to the tile's regions, to LDS (as post_down.hip keeps them).
//   1. codes    C is read once, quantised once (quant_rgb, plain or PQ) and kept as u16 codes[ch][row][col].
//   2. stage A  per channel: the horizontal sums of every row of C for the columns of P to hor (int32), then the vertical sums
//               (int64), shifted and clamped, to the spline36 codes pc (u16).  Without SSIM the tile's codes are stored and the kernel ends.
//   3. pass I   for the rows of L and the columns of P: A.rgb, A.q and from them e1, to A (float, four planes; hor is dead).
//   4. pass II  for L: Lr.rgb, q2, e2, the linear fetch of e1 and Lr.a, to lr (float, four planes).
//   5. var      for F: vL from the source samples, vH from Lr.rgb, to the first two planes of the buffer A left.
//   6. final    per output pixel: mV, the nine taps, the division, the quantiser, the store.
// LDS, bytes, every array on a 16-byte boundary, with NCy x NCx = sr_nc, NPy x NPx = sr_np, NLy x NLx = sr_nl of the tile:
// LDS(SSIM) = 2 * 3 * NCy * NCx (codes) + 2 * 3 * NPy * NPx (pc) + 4 * NU (hor / A / var share one buffer, NU = max(NCy * NPx,
// SSIM ? max(4 * NLy * NPx, 2 * (TH + 2) * (TW + 2)) : 0)) + (SSIM ? 4 * 4 * NLy * NLx : 0) (lr) + the tile's slice of the tables,
// 16 * (NPx + NPy) (xsp, ysp) + (SSIM ? 16 * (TW + TH) (xfin, yfin) + 16 * (NLx + NLy) (xlow, ylow) + 4 * 9 * (NLx + NLy) (xw, yw) : 0):
// 11,200 / 51,040 bytes without / with SSIM, three workgroups per CU (tests/test_isa_post_ssimsr.py).
// Banks (MI355X_MICROARCH.md): in every phase a lane owns one column of its region and neighbouring lanes neighbouring columns.
// The reads of hor, A (pass I's stores), lr (pass II's stores) and the var planes are consecutive dwords; the reads of codes and pc
// consecutive halves (two lanes share a dword: a broadcast).  Pass II reads A at a stride of r <= 2 dwords between lanes (two-way
// at 2x), stage A's horizontal pass reads codes and the final pass reads lr and var at a stride of 1 / r (neighbours share a word).
#include "launchers.h"
#include "post_quant.h"

namespace {

__device__ __forceinline__ float fm(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fa(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float fs(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float fd(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float sat(float a) { return fminf(fmaxf(a, 0.f), 1.f); }
// the correctly rounded square root: sqrtf, as in post_down.hip (__fsqrt_rn is the approximate root in this toolchain's headers
// unless OCML_BASIC_ROUNDED_OPERATIONS is defined)
__device__ __forceinline__ float fsq(float a) { return sqrtf(a); }

// u16 code -> float32(c / 65535), correctly rounded for every code (post_fsr.hip's fsr_sample; tests/test_rgb48_fsr_host.py)
__device__ __forceinline__ float sr_sample(uint32_t c)
{
    constexpr float r = (float)(1.0 / 65535.0);
    const float x = (float)c;
    const float q = __fmul_rn(x, r);
    return __fmaf_rn(__fmaf_rn(-q, 65535.f, x), r, q);
}

// the shader's Luma, which squares first: (0.2126 (r r) + 0.7152 (g g)) + 0.0722 (b b)
__device__ __forceinline__ float sq3(float r, float g, float b)
{
    return fa(fa(fm(0.2126f, fm(r, r)), fm(0.7152f, fm(g, g))), fm(0.0722f, fm(b, b)));
}

struct Rgb { float r, g, b; };

// the mean and the variance of a pixel and its four cross neighbours, weights 1 and 0.25, halved (a multiply by 0.5 rounds as the
// division by 2), the variance floored at 1e-6
__device__ __forceinline__ float cross_var(const Rgb (&v)[5])
{
    float mr = v[0].r, mg = v[0].g, mb = v[0].b;
#pragma unroll
    for (int i = 1; i < 5; ++i) {
        mr = fa(mr, fm(0.25f, v[i].r));
        mg = fa(mg, fm(0.25f, v[i].g));
        mb = fa(mb, fm(0.25f, v[i].b));
    }
    mr = fm(mr, 0.5f);
    mg = fm(mg, 0.5f);
    mb = fm(mb, 0.5f);
    float acc = sq3(fs(v[0].r, mr), fs(v[0].g, mg), fs(v[0].b, mb));
#pragma unroll
    for (int i = 1; i < 5; ++i) acc = fa(acc, fm(0.25f, sq3(fs(v[i].r, mr), fs(v[i].g, mg), fs(v[i].b, mb))));
    return fmaxf(fm(acc, 0.5f), 1e-6f);
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

template <typename T, bool PQ, bool SSIM>
__global__ __launch_bounds__(256) void post_ssimsr_kernel(const PostSsimsrParams p)
{
    constexpr int TH = SR_TH, TW = SR_TW;
    constexpr int NCY = sr_nc(SSIM, TH), NCX = sr_nc(SSIM, TW), NPY = sr_np(SSIM, TH), NPX = sr_np(SSIM, TW);
    constexpr int NLY = sr_nl(TH), NLX = sr_nl(TW), NFY = TH + 2, NFX = TW + 2;
    constexpr int NU = cmax(NCY * NPX, SSIM ? cmax(4 * NLY * NPX, 2 * NFY * NFX) : 0);
    __shared__ __attribute__((aligned(16))) uint16_t codes[3][NCY][NCX];
    __shared__ __attribute__((aligned(16))) uint16_t pc[3][NPY][NPX];
    __shared__ __attribute__((aligned(16))) int ubuf[NU];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int x1 = min(x0 + TW, p.dW) - 1, y1 = min(y0 + TH, p.dH) - 1;

    // 0. the regions of this tile: F [fxa, fxb] x [fya, fyb], L, P, C likewise
    int fxa = 0, fxb = 0, fya = 0, fyb = 0, lxa = 0, lxb = 0, lya = 0, lyb = 0;
    int pxa = x0, pxb = x1, pya = y0, pyb = y1;
    if constexpr (SSIM) {
        fxa = max(p.xfin[x0].x - 1, 0), fxb = min(p.xfin[x1].x + 1, p.W - 1);
        fya = max(p.yfin[y0].x - 1, 0), fyb = min(p.yfin[y1].x + 1, p.H - 1);
        lxa = max(fxa - 1, 0), lxb = min(fxb + 1, p.W - 1);
        lya = max(fya - 1, 0), lyb = min(fyb + 1, p.H - 1);
        const int4 ta = p.xlow[lxa], tb = p.xlow[lxb], ua = p.ylow[lya], ub = p.ylow[lyb];
        pxa = max(ta.x, 0), pxb = min(tb.x + tb.y - 1, p.dW - 1);
        pya = max(ua.x, 0), pyb = min(ub.x + ub.y - 1, p.dH - 1);
    }
    const int cxa = max(p.xsp[pxa].x, 0), cxb = min(p.xsp[pxb].x + 5, p.W - 1);
    const int cya = max(p.ysp[pya].x, 0), cyb = min(p.ysp[pyb].x + 5, p.H - 1);
    const int npx = min(pxb - pxa + 1, NPX), npy = min(pyb - pya + 1, NPY);
    const int ncx = min(cxb - cxa + 1, NCX), ncy = min(cyb - cya + 1, NCY);
    const int nlx = min(lxb - lxa + 1, NLX), nly = min(lyb - lya + 1, NLY);
    // the tile's slice of the tables: a tap loop that fetched its coefficients from global memory would wait for one load per tap
    __shared__ int4 sxsp[NPX], sysp[NPY];
    __shared__ int4 sxfin[SSIM ? TW : 1], syfin[SSIM ? TH : 1], sxlow[SSIM ? NLX : 1], sylow[SSIM ? NLY : 1];
    __shared__ __attribute__((aligned(16))) float sxw[SSIM ? NLX * SR_NT : 4], syw[SSIM ? NLY * SR_NT : 4];
    if (tid < npx) sxsp[tid] = p.xsp[pxa + tid];
    if (tid < npy) sysp[tid] = p.ysp[pya + tid];
    if constexpr (SSIM) {
        if (tid <= x1 - x0) sxfin[tid] = p.xfin[x0 + tid];
        if (tid <= y1 - y0) syfin[tid] = p.yfin[y0 + tid];
        if (tid < nlx) sxlow[tid] = p.xlow[lxa + tid];
        if (tid < nly) sylow[tid] = p.ylow[lya + tid];
        for (int i = tid; i < nlx * SR_NT; i += 256) sxw[i] = p.xw[(size_t)lxa * SR_NT + i];
        for (int i = tid; i < nly * SR_NT; i += 256) syw[i] = p.yw[(size_t)lya * SR_NT + i];
    }

    // 1. stage + quantise
    {
        const T *__restrict__ in = static_cast<const T *>(p.in);
        const size_t plane = (size_t)p.H * p.W;
        for (int i = tid; i < ncy * ncx; i += 256) {
            const int r = i / ncx, c = i - r * ncx;
            const size_t o = (size_t)(cya + r) * p.W + (cxa + c);
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
        int *hor = ubuf;                                                      // [ncy][NPX], column j = destination column pxa + j
#pragma unroll 1
        for (int i = tid; i < ncy * npx; i += 256) {
            const int r = i / npx, j = i - r * npx;
            const int4 t = sxsp[j];
            const uint16_t *row = &codes[ch][r][0];
            const int q[6] = {(short)t.y, t.y >> 16, (short)t.z, t.z >> 16, (short)t.w, t.w >> 16};
            int acc = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc += (int)row[clampi(t.x + k, p.W - 1) - cxa] * q[k];
            hor[r * NPX + j] = acc;
        }
        __syncthreads();
#pragma unroll 1
        for (int i = tid; i < npy * npx; i += 256) {
            const int r = i / npx, j = i - r * npx;
            const int4 t = sysp[r];
            const int q[6] = {(short)t.y, t.y >> 16, (short)t.z, t.z >> 16, (short)t.w, t.w >> 16};
            long long acc = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc += (long long)hor[(clampi(t.x + k, p.H - 1) - cya) * NPX + j] * q[k];
            const long long v = (acc + (1ll << 27)) >> 28;
            pc[ch][r][j] = (uint16_t)(v < 0 ? 0 : v > 65535 ? 65535 : v);
        }
        __syncthreads();
    }

    if constexpr (!SSIM) {
        // the spline36 codes of the tile
        for (int i = tid; i < TH * TW; i += 256) {
            const int ly = i / TW, lx = i - ly * TW;
            if (y0 + ly > y1 || x0 + lx > x1) continue;
            uint16_t *d = p.dst + ((size_t)(y0 + ly) * p.dW + x0 + lx) * 3;
            d[0] = pc[0][ly][lx];
            d[1] = pc[1][ly][lx];
            d[2] = pc[2][ly][lx];
        }
    } else {
        __shared__ __attribute__((aligned(16))) float lr[4][NLY][NLX];
        const int nfx = min(fxb - fxa + 1, NFX), nfy = min(fyb - fya + 1, NFY);
        float *A = reinterpret_cast<float *>(ubuf);                           // [4][NLY][NPX]: A.rgb and e1
        constexpr int AP = NLY * NPX;

        // 3. pass I, vertical: row ly = low-resolution row lya + ly, column j = high-resolution column pxa + j
#pragma unroll 1
        for (int i = tid; i < nly * npx; i += 256) {
            const int ly = i / npx, j = i - ly * npx;
            const int4 t = sylow[ly];
            const float *w = syw + ly * SR_NT;
            float ar = 0.f, ag = 0.f, ab = 0.f, aq = 0.f;
#pragma unroll 3
            for (int k = 0; k < t.y; ++k) {
                const int r = clampi(t.x + k, p.dH - 1) - pya;
                const float s0 = sr_sample(pc[0][r][j]), s1 = sr_sample(pc[1][r][j]), s2 = sr_sample(pc[2][r][j]);
                const float wk = w[k];
                ar = fa(ar, fm(wk, s0));
                ag = fa(ag, fm(wk, s1));
                ab = fa(ab, fm(wk, s2));
                aq = fa(aq, fm(wk, sq3(s0, s1, s2)));
            }
            const int o = ly * NPX + j;
            A[o] = ar;
            A[AP + o] = ag;
            A[2 * AP + o] = ab;
            A[3 * AP + o] = fmaxf(fabsf(fs(aq, sq3(ar, ag, ab))), 5e-7f);
        }
        __syncthreads();

        // 4. pass II, horizontal: column li = low-resolution column lxa + li
#pragma unroll 1
        for (int i = tid; i < nly * nlx; i += 256) {
            const int ly = i / nlx, li = i - ly * nlx;
            const int4 t = sxlow[li];
            const float *w = sxw + li * SR_NT;
            const float *row = A + ly * NPX;
            float ar = 0.f, ag = 0.f, ab = 0.f, aq = 0.f;
#pragma unroll 3
            for (int k = 0; k < t.y; ++k) {
                const int c = clampi(t.x + k, p.dW - 1) - pxa;
                const float s0 = row[c], s1 = row[AP + c], s2 = row[2 * AP + c];
                const float wk = w[k];
                ar = fa(ar, fm(wk, s0));
                ag = fa(ag, fm(wk, s1));
                ab = fa(ab, fm(wk, s2));
                aq = fa(aq, fm(wk, sq3(s0, s1, s2)));
            }
            const float e2 = fmaxf(fabsf(fs(aq, sq3(ar, ag, ab))), 5e-7f);
            const float f = __int_as_float(t.w);
            const float e1i = fa(fm(fs(1.f, f), row[3 * AP + clampi(t.z, p.dW - 1) - pxa]), fm(f, row[3 * AP + clampi(t.z + 1, p.dW - 1) - pxa]));
            lr[0][ly][li] = ar;
            lr[1][ly][li] = ag;
            lr[2][ly][li] = ab;
            lr[3][ly][li] = fa(e2, e1i);
        }
        __syncthreads();

        // 5. var on F: vL [NFY][NFX] then vH
        float *vv = reinterpret_cast<float *>(ubuf);
        constexpr int VP = NFY * NFX;
#pragma unroll 1
        for (int i = tid; i < nfy * nfx; i += 256) {
            const int fy = i / nfx, gy = fya + fy, gx = fxa + (i - fy * nfx);
            const int ny[5] = {gy, gy, gy, max(gy - 1, 0), min(gy + 1, p.H - 1)};
            const int nx[5] = {gx, max(gx - 1, 0), min(gx + 1, p.W - 1), gx, gx};
            Rgb s[5], l[5];
#pragma unroll
            for (int n = 0; n < 5; ++n) {
                const int sy = ny[n] - cya, sx = nx[n] - cxa, qy = ny[n] - lya, qx = nx[n] - lxa;
                s[n] = Rgb{sr_sample(codes[0][sy][sx]), sr_sample(codes[1][sy][sx]), sr_sample(codes[2][sy][sx])};
                l[n] = Rgb{lr[0][qy][qx], lr[1][qy][qx], lr[2][qy][qx]};
            }
            vv[fy * NFX + (gx - fxa)] = cross_var(s);
            vv[VP + fy * NFX + (gx - fxa)] = cross_var(l);
        }
        __syncthreads();

        // 6. final pass + quantise + store
#pragma unroll 1
        for (int i = tid; i < TH * TW; i += 256) {
            const int ty = i / TW, tx = i - ty * TW;
            const int y = y0 + ty, x = x0 + tx;
            if (y > y1 || x > x1) continue;
            const int4 ey = syfin[ty], ex = sxfin[tx];
            const int gy[3] = {max(ey.x - 1, 0), ey.x, min(ey.x + 1, p.H - 1)};
            const int gx[3] = {max(ex.x - 1, 0), ex.x, min(ex.x + 1, p.W - 1)};
            const float ky[3] = {__int_as_float(ey.y), __int_as_float(ey.z), __int_as_float(ey.w)};
            const float kx[3] = {__int_as_float(ex.y), __int_as_float(ex.z), __int_as_float(ex.w)};
            const float hw[3] = {0.5f, 1.f, 0.5f};
            const float c0r = sr_sample(pc[0][y - pya][x - pxa]), c0g = sr_sample(pc[1][y - pya][x - pxa]), c0b = sr_sample(pc[2][y - pya][x - pxa]);
            float mv = 0.f;
#pragma unroll
            for (int X = 0; X < 3; ++X)
#pragma unroll
                for (int Y = 0; Y < 3; ++Y) mv = fa(mv, fm(fm(hw[X], hw[Y]), lr[3][gy[Y] - lya][gx[X] - lxa]));
            mv = fm(mv, 0.25f);
            float dr = 0.f, dg = 0.f, db = 0.f, ws = 0.f;
#pragma unroll
            for (int X = 0; X < 3; ++X) {
#pragma unroll
                for (int Y = 0; Y < 3; ++Y) {
                    const int qy = gy[Y] - lya, qx = gx[X] - lxa, sy = gy[Y] - cya, sx = gx[X] - cxa;
                    const int vo = (gy[Y] - fya) * NFX + (gx[X] - fxa);
                    const float l0 = lr[0][qy][qx], l1 = lr[1][qy][qx], l2 = lr[2][qy][qx], la = lr[3][qy][qx];
                    const float R = fm(-1.5f, fsq(fd(vv[vo], fa(vv[VP + vo], mv))));
                    const float wt = fd(fm(kx[X], ky[Y]), fa(sq3(fs(c0r, l0), fs(c0g, l1), fs(c0b, l2)), la));
                    const float omr = fs(-1.f, R);
                    dr = fa(dr, fm(wt, fa(fa(sr_sample(codes[0][sy][sx]), fm(l0, R)), fm(omr, c0r))));
                    dg = fa(dg, fm(wt, fa(fa(sr_sample(codes[1][sy][sx]), fm(l1, R)), fm(omr, c0g))));
                    db = fa(db, fm(wt, fa(fa(sr_sample(codes[2][sy][sx]), fm(l2, R)), fm(omr, c0b))));
                    ws = fa(ws, wt);
                }
            }
            uint16_t *d = p.dst + ((size_t)y * p.dW + x) * 3;
            d[0] = (uint16_t)quant_u16(sat(fa(c0r, fd(dr, ws))));
            d[1] = (uint16_t)quant_u16(sat(fa(c0g, fd(dg, ws))));
            d[2] = (uint16_t)quant_u16(sat(fa(c0b, fd(db, ws))));
        }
    }
}

template <typename T, bool PQ>
void launch(const PostSsimsrParams &p, int ssim, hipStream_t s)
{
    const dim3 g((p.dW + SR_TW - 1) / SR_TW, (p.dH + SR_TH - 1) / SR_TH);
    if (ssim) hipLaunchKernelGGL((post_ssimsr_kernel<T, PQ, true>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((post_ssimsr_kernel<T, PQ, false>), g, dim3(256), 0, s, p);
}

}  // namespace

hipError_t post_ssimsr_launch(const PostSsimsrParams &p, int ssim, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH <= p.H || p.dW <= p.W || p.dH > 2 * (long long)p.H || p.dW > 2 * (long long)p.W || (pq && !p.pq_bnd))
        return hipErrorInvalidValue;
    if (is_f32) {
        if (pq) launch<float, true>(p, ssim, s);
        else launch<float, false>(p, ssim, s);
    } else {
        if (pq) launch<f16, true>(p, ssim, s);
        else launch<f16, false>(p, ssim, s);
    }
    return hipGetLastError();
}
