// letterbox10.hip -- letterbox of a 10-bit Y'CbCr frame (P010, yuv420p10le, yuv422p10le) at ten bits, on the GPU (gfx950): the
// reference's order of operations -- decode to RGB, then _letterbox_bgr -- in one launch that reads the planes at the SOURCE size and
// writes at the PROCESSING size.  No source-sized RGB buffer exists in device memory.  The rule: include/hdrtv_mi355x.h
// (hdrtv_letterbox_ycbcr10), restated in tests/letterbox10_ref.py; the geometry and tables are letterbox_setup's (hdrtv_api.hip),
// the ones letterbox_kernel (letterbox.hip) reads.
//
//  letterbox10_kernel<STORE>  a 256-thread workgroup owns a 32 x 8 tile of destination pixels.  It stages the source patch the tile's
//                             taps cover (raw luma words into the patch itself, the chroma rows and columns around it beside it),
//                             converts every patch pixel ONCE with ycc_rule<10> into one packed 10:10:10 word in LDS, and resamples
//                             its 256 pixels from there; pixels outside the rectangle are written as zeros by the same launch.
//                             STORE: u16 HWC codes | f16 CHW planes fp16(float(code) * fp32(1/1023)) | f32 CHW planes, the same
//                             expression without the last conversion.
//  cond_quarter_f16_kernel    the 0.25x condition map of an f16 tensor in condition modes 1 (bilinear) and 2 (zero), which
//                             cond_resize_launch does not have; the arithmetic of pre_fused's and cond_resize_f32's mode 1.
//
// LDS: the patch is at most 130 x 34 (a 4x shrink per axis is the cap: 128 x 32, one more row and column for a fractional ratio,
// rounded up to even), 17.4 KB at pitch 131; the chroma area 34 rows of 2 x 68 samples, 9.0 KB.  26.4 KB per workgroup.
// The plane stager and the chroma walk are ycc_in.h's.  Built with -ffp-contract=off (csrc/Makefile), as letterbox.hip: the area modes
// multiply and add separately in float32.
#include "ycc_in.h"

namespace {

constexpr int LB10_TW = 32, LB10_TH = 8;                       // destination tile
constexpr int LB10_PW = 130, LB10_PH = 34, LB10_PITCH = 131;   // patch: pixels, rows, row pitch in words
constexpr int LB10_CW = 68, LB10_CROWS = 34;                   // chroma samples per plane of a staged row / staged rows
static_assert(LB10_TW * LB10_TH == 256, "one thread per destination pixel");
static_assert(LB10_PW >= 4 * LB10_TW + 1 && LB10_PH >= 4 * LB10_TH + 1, "a 4x fractional shrink");
static_assert(LB10_PW / 2 + 2 <= LB10_CW && LB10_PH <= LB10_CROWS, "the chroma columns / rows a full patch needs");

template <int STORE>
__device__ __forceinline__ void lb10_store(void *__restrict__ dst, int dh, int dw, int y, int x, uint32_t r, uint32_t g, uint32_t b)
{
    const float k1023 = (float)(1.0 / 1023.0);
    const size_t npix = (size_t)dh * dw, o = (size_t)y * dw + x;
    if (STORE == LB10_U16_HWC) {
        uint16_t *d = static_cast<uint16_t *>(dst) + o * 3;
        d[0] = (uint16_t)r; d[1] = (uint16_t)g; d[2] = (uint16_t)b;
    } else if (STORE == LB10_F16_CHW) {
        f16 *d = static_cast<f16 *>(dst);
        d[o] = (f16)__fmul_rn((float)r, k1023);
        d[npix + o] = (f16)__fmul_rn((float)g, k1023);
        d[2 * npix + o] = (f16)__fmul_rn((float)b, k1023);
    } else {
        float *d = static_cast<float *>(dst);
        d[o] = __fmul_rn((float)r, k1023);
        d[npix + o] = __fmul_rn((float)g, k1023);
        d[2 * npix + o] = __fmul_rn((float)b, k1023);
    }
}

__device__ __forceinline__ uint32_t sat10_rint(float v)
{
    const float r = rintf(v);                                  // cvRound: half to even
    return (uint32_t)(r < 0.f ? 0.f : (r > 1023.f ? 1023.f : r));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int STORE>
__global__ __launch_bounds__(256) void letterbox10_kernel(const Ycc10Src src, const LetterboxParams p, void *__restrict__ dst)
{
    __shared__ uint32_t s_px[LB10_PH][LB10_PITCH];             // raw luma word, then R | G << 10 | B << 20 of the patch pixel
    __shared__ uint16_t s_c[LB10_CROWS][2 * LB10_CW];          // planar: Cb at 0.., Cr at LB10_CW..; P010: the CbCr pairs as they lie
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * LB10_TW, ty0 = blockIdx.y * LB10_TH;
    // the part of the rectangle this tile covers, in rectangle coordinates (block-uniform)
    const int rx0 = max(tx0 - p.x0, 0), rx1 = min(tx0 + LB10_TW - 1 - p.x0, p.new_w - 1);
    const int ry0 = max(ty0 - p.y0, 0), ry1 = min(ty0 + LB10_TH - 1 - p.y0, p.new_h - 1);
    int px0 = 0, py0 = 0, pw = 1, ph = 1;
    if (rx0 <= rx1 && ry0 <= ry1) {
        // ---- the source patch the tile's taps cover
        int x1, y1;
        if (p.mode == LB_COPY) {
            px0 = rx0; x1 = rx1; py0 = ry0; y1 = ry1;
        } else if (p.mode == LB_AREA_INT) {
            px0 = rx0 * p.ix; x1 = rx1 * p.ix + p.ix - 1; py0 = ry0 * p.iy; y1 = ry1 * p.iy + p.iy - 1;
        } else if (p.mode == LB_AREA_FRAC) {                   // runs and the indices inside a run ascend
            px0 = p.xsrc[p.xbeg[rx0]]; x1 = p.xsrc[p.xbeg[rx1 + 1] - 1];
            py0 = p.ysrc[p.ybeg[ry0]]; y1 = p.ysrc[p.ybeg[ry1 + 1] - 1];
        } else {                                               // four taps from the offset, replicated at the frame's borders
            px0 = p.xsrc[rx0]; x1 = p.xsrc[rx1] + 3; py0 = p.ysrc[ry0]; y1 = p.ysrc[ry1] + 3;
        }
        px0 = clampi(px0, 0, p.sw - 1); x1 = clampi(x1, px0, p.sw - 1);
        py0 = clampi(py0, 0, p.sh - 1); y1 = clampi(y1, py0, p.sh - 1);
        pw = min(x1 - px0 + 1, LB10_PW); ph = min(y1 - py0 + 1, LB10_PH);      // (never cut: the launcher refuses a shrink beyond 4x)
        x1 = px0 + pw - 1; y1 = py0 + ph - 1;
        // ---- stage: luma words into the patch, the chroma rows / columns the patch's pixels use (clamped at the frame's edges)
        const bool p010 = src.layout == YCC10_P010, c422 = src.layout == YCC10_YUV422P10;
        const int Hc = c422 ? p.sh : p.sh >> 1, Wc = p.sw >> 1;
        const int jlo = c422 ? py0 : max((py0 >> 1) - 1, 0), jhi = c422 ? y1 : min((y1 >> 1) + 1, Hc - 1);
        const int ilo = px0 >> 1, ihi = min((x1 >> 1) + 1, Wc - 1);
        const int nrow = min(jhi - jlo + 1, LB10_CROWS), ncol = min(ihi - ilo + 1, LB10_CW);
        ycc10_stage(src.y, src.y_pitch, py0, ph, px0, pw, &s_px[0][0], LB10_PITCH, tid);
        if (p010) {
            ycc10_stage(src.u, src.c_pitch, jlo, nrow, 2 * ilo, 2 * ncol, &s_c[0][0], 2 * LB10_CW, tid);
        } else {
            ycc10_stage(src.u, src.c_pitch, jlo, nrow, ilo, ncol, &s_c[0][0], 2 * LB10_CW, tid);
            ycc10_stage(src.v, src.c_pitch, jlo, nrow, ilo, ncol, &s_c[0][LB10_CW], 2 * LB10_CW, tid);
        }
        __syncthreads();
        // ---- convert: one item = one chroma column of one row = the two patch pixels that share it; the item that reads a pixel's
        // luma word is the one that overwrites it
        const int cs = p010 ? 2 : 1, co = p010 ? 1 : LB10_CW, sh = p010 ? 6 : 0;
        for (int e = tid; e < ph * ncol; e += 256) {
            const int r = e / ncol, c = e - r * ncol;
            const int y = py0 + r, i = ilo + c, q0 = 2 * i - px0;
            int j, n, u4a, u4b, v4a, v4b;
            ycc_rows(y, Hc, c422, j, n);
            const uint16_t *cj = s_c[min(j - jlo, nrow - 1)], *cn = s_c[min(n - jlo, nrow - 1)];
            ycc_walk<10>(cj, cn, cs * c, cs * min(ycc_col2(i, ihi) - ilo, ncol - 1), co, sh, u4a, u4b, v4a, v4b);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = q0 + h;
                if (q < 0 || q >= pw) continue;
                uint32_t R, G, B;
                ycc_rule<10>(ycc_sample<10>(s_px[r][q], sh), h ? u4a + u4b : 2 * u4a, h ? v4a + v4b : 2 * v4a, src.k, R, G, B);
                s_px[r][q] = R | (G << 10) | (B << 20);
            }
        }
        __syncthreads();
    }
    // ---- resample this thread's pixel from the patch
    const int x = tx0 + (tid & (LB10_TW - 1)), y = ty0 + tid / LB10_TW;
    if (x >= p.dw || y >= p.dh) return;
    const int rx = x - p.x0, ry = y - p.y0;
    if (rx < 0 || ry < 0 || rx >= p.new_w || ry >= p.new_h) { lb10_store<STORE>(dst, p.dh, p.dw, y, x, 0u, 0u, 0u); return; }
    // patch word of source pixel (sx, sy); the clamps keep a read inside the staged patch whatever the tables hold
    auto at = [&](int sx, int sy) { return s_px[clampi(sy - py0, 0, ph - 1)][clampi(sx - px0, 0, pw - 1)]; };
    uint32_t out[3];
    if (p.mode == LB_COPY) {
        const uint32_t w = at(rx, ry);
        out[0] = w & 1023u; out[1] = (w >> 10) & 1023u; out[2] = w >> 20;
    } else if (p.mode == LB_AREA_INT) {
        int sum[3] = {0, 0, 0};
        for (int j = 0; j < p.iy; ++j)
            for (int i = 0; i < p.ix; ++i) {
                const uint32_t w = at(rx * p.ix + i, ry * p.iy + j);
                sum[0] += (int)(w & 1023u); sum[1] += (int)((w >> 10) & 1023u); sum[2] += (int)(w >> 20);
            }
        if (p.ix == 2 && p.iy == 2) {
            for (int c = 0; c < 3; ++c) out[c] = (uint32_t)((sum[c] + 2) >> 2);
        } else {
            const float scale = __fdiv_rn(1.0f, (float)(p.ix * p.iy));
            for (int c = 0; c < 3; ++c) out[c] = sat10_rint(__fmul_rn((float)sum[c], scale));
        }
    } else if (p.mode == LB_AREA_FRAC) {
        // float32, multiply and add separate, accumulation in table order: letterbox_kernel's sequence on the codes
        const int xb = p.xbeg[rx], xn = p.xbeg[rx + 1] - xb, yb = p.ybeg[ry], yn = p.ybeg[ry + 1] - yb;
        float sum[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < yn; ++j) {
            const int sy = p.ysrc[yb + j];
            const float beta = p.yw[yb + j];
            float buf[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < xn; ++i) {
                const uint32_t w = at(p.xsrc[xb + i], sy);
                const float a = p.xw[xb + i];
                buf[0] = __fadd_rn(buf[0], __fmul_rn((float)(w & 1023u), a));
                buf[1] = __fadd_rn(buf[1], __fmul_rn((float)((w >> 10) & 1023u), a));
                buf[2] = __fadd_rn(buf[2], __fmul_rn((float)(w >> 20), a));
            }
            for (int c = 0; c < 3; ++c) sum[c] = j == 0 ? __fmul_rn(beta, buf[c]) : __fadd_rn(sum[c], __fmul_rn(beta, buf[c]));
        }
        for (int c = 0; c < 3; ++c) out[c] = sat10_rint(sum[c]);
    } else {   // LB_CUBIC: 11-bit coefficients, horizontal then vertical, replicated borders; 1023 x 2560 x 2560 exceeds 2^31
        const int xo = p.xsrc[rx], yo = p.ysrc[ry];
        long long acc[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            const int sy = clampi(yo + k, 0, p.sh - 1);
            long long hor[3] = {0, 0, 0};
            for (int i = 0; i < 4; ++i) {
                const uint32_t w = at(clampi(xo + i, 0, p.sw - 1), sy);
                const int cx = p.xc[rx * 4 + i];
                hor[0] += (long long)(w & 1023u) * cx; hor[1] += (long long)((w >> 10) & 1023u) * cx; hor[2] += (long long)(w >> 20) * cx;
            }
            const int cy = p.yc[ry * 4 + k];
            for (int c = 0; c < 3; ++c) acc[c] += hor[c] * cy;
        }
        for (int c = 0; c < 3; ++c) {
            const long long v = (acc[c] + (1ll << 21)) >> 22;
            out[c] = (uint32_t)(v < 0 ? 0 : (v > 1023 ? 1023 : v));
        }
    }
    lb10_store<STORE>(dst, p.dh, p.dw, y, x, out[0], out[1], out[2]);
}

// mode 1: upsample_bilinear2d at 0.25x, the mean of pixels (4d+1, 4d+2) per direction in ATen's operation order (pre_fused_kernel's
// and cond_resize_f32_kernel's mode 1); mode 2: zeros
__global__ __launch_bounds__(256) void cond_quarter_f16_kernel(const f16 *__restrict__ in, f16 *__restrict__ out, int H, int W, int Ho,
                                                               int Wo, int mode)
{
    const size_t n = (size_t)3 * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (mode == 1) {
            const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), c = (int)(i / ((size_t)Wo * Ho));
            const f16 *src = in + (size_t)c * H * W;
            const int y1 = 4 * oy + 1, x1 = 4 * ox + 1;
            const int y2 = y1 + 1 < H ? y1 + 1 : H - 1, x2 = x1 + 1 < W ? x1 + 1 : W - 1;
            const float top = __fadd_rn(__fmul_rn(0.5f, (float)src[(size_t)y1 * W + x1]), __fmul_rn(0.5f, (float)src[(size_t)y1 * W + x2]));
            const float bot = __fadd_rn(__fmul_rn(0.5f, (float)src[(size_t)y2 * W + x1]), __fmul_rn(0.5f, (float)src[(size_t)y2 * W + x2]));
            v = __fadd_rn(__fmul_rn(0.5f, top), __fmul_rn(0.5f, bot));
        }
        out[i] = (f16)v;
    }
}

}  // namespace

bool letterbox10_size_ok(const LetterboxParams &p)
{
    return p.sh > 0 && p.sw > 0 && p.dh > 0 && p.dw > 0 && p.new_w > 0 && p.new_h > 0 && p.sw <= LB10_MAX_SHRINK * (long long)p.new_w &&
           p.sh <= LB10_MAX_SHRINK * (long long)p.new_h;
}

hipError_t letterbox10_launch(const Ycc10Src &src, const LetterboxParams &p, int store, void *dst, hipStream_t s)
{
    if (!ycc_ok(src, p.sh, p.sw) || !dst || !letterbox10_size_ok(p))
        return hipErrorInvalidValue;
    if (p.mode == LB_AREA_INT && (p.ix < 1 || p.iy < 1 || p.ix > LB10_MAX_SHRINK || p.iy > LB10_MAX_SHRINK)) return hipErrorInvalidValue;
    const dim3 g((p.dw + LB10_TW - 1) / LB10_TW, (p.dh + LB10_TH - 1) / LB10_TH), b(256);
    if (store == LB10_U16_HWC) hipLaunchKernelGGL(letterbox10_kernel<LB10_U16_HWC>, g, b, 0, s, src, p, dst);
    else if (store == LB10_F16_CHW) hipLaunchKernelGGL(letterbox10_kernel<LB10_F16_CHW>, g, b, 0, s, src, p, dst);
    else if (store == LB10_F32_CHW) hipLaunchKernelGGL(letterbox10_kernel<LB10_F32_CHW>, g, b, 0, s, src, p, dst);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t cond_quarter_f16_launch(const f16 *in, f16 *out, int H, int W, int mode, hipStream_t s)
{
    const int Ho = H / 4, Wo = W / 4;
    if (!in || !out || Ho < 1 || Wo < 1 || (mode != 1 && mode != 2)) return hipErrorInvalidValue;
    size_t g = ((size_t)3 * Ho * Wo + 255) / 256;
    if (g > 2048) g = 2048;                                    // 256 CUs x 8 blocks, grid-stride beyond
    hipLaunchKernelGGL(cond_quarter_f16_kernel, dim3((unsigned)g), dim3(256), 0, s, in, out, H, W, Ho, Wo, mode);
    return hipGetLastError();
}
