// post_scale.hip -- RGB48 at the display size in one launch (gfx950): the u16 quantiser of post_rgb48 / post_pq_rgb48 and a
// separable six-tap Lanczos-3 upscale of its codes (hdrtv_post_rgb48_scaled; include/hdrtv_mi355x.h states the integer rule).
// Doing it as post_rgb48 + a resize kernel would write and re-read a frame of codes, and the PQ variant would run pq_code on
// dH x dW values rather than H x W.
//
// A workgroup of 256 lanes owns PS_TH x PS_TW = 32 x 64 output pixels:
//   1. stage   the source footprint -- rows [ys0, ys0 + nr), columns [xs0, xs0 + nc), nr <= 38 and nc <= 70 whatever the ratio
//              because dH >= H, dW >= W (a step of one output pixel moves the first tap by at most one source pixel); indices
//              outside the frame read the clamped pixel, so the passes below never clamp -- is read from HBM once, quantised
//              once (plain or PQ: the three planes of a pixel by one lane, as the matrix needs them) and kept as u16 codes
//              `codes[ch][row][col]`.
//   2. horizontal  hor[ch][row][dx] = sum_k codes[ch][row][xs(dx) - xs0 + k] * qx_k(dx): exact in int32 (sum |q| <= 25290).  A lane
//              keeps one output column and its six coefficients in registers and walks the (ch, row) pairs of its wave.
//   3. vertical    a lane owns four neighbouring pixels of an output row: per channel and tap one 16-byte row segment of `hor`, the
//              46-bit sums in int64, (sum + 2^27) >> 28 clamped to u16, twelve codes = 24 bytes as three 8-byte stores
//              (post_rgb48_kernel's packing, at the alignment a row pitch of dW * 6 bytes leaves).  A group whose address is not
//              8-byte aligned (odd dW) or that crosses the right edge stores its valid codes one by one.
// LDS banks (MI355X_MICROARCH.md): the horizontal reads of a wave are 64 u16 addresses that rise by at most one element per lane
// (same dword = broadcast), its writes 64 consecutive dwords; the vertical ds_read_b128 of a 16-lane group covers one 256-byte
// row of `hor` (rows are 64 dwords apart, so lanes of different output rows in a group still hit different banks).
// 16.0 KiB + 28.5 KiB of LDS: three workgroups per CU.
#include "launchers.h"
#include "post_quant.h"

namespace {

constexpr int PS_SR = PS_TH + 6, PS_SC = PS_TW + 6, PS_SCP = PS_SC + 2;

__device__ __forceinline__ void unpack_taps(const int4 t, int (&q)[6])
{
    q[0] = (t.y << 16) >> 16; q[1] = t.y >> 16;
    q[2] = (t.z << 16) >> 16; q[3] = t.z >> 16;
    q[4] = (t.w << 16) >> 16; q[5] = t.w >> 16;
}

template <typename T, bool PQ>
__global__ __launch_bounds__(256) void post_scale_kernel(PostScaleParams p)
{
    __shared__ uint16_t codes[3][PS_SR][PS_SCP];
    __shared__ __attribute__((aligned(16))) int hor[3][PS_SR][PS_TW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PS_TW, y0 = blockIdx.y * PS_TH;
    const int xl = min(x0 + PS_TW, p.dW) - 1, yl = min(y0 + PS_TH, p.dH) - 1;
    const int xs0 = p.xtab[x0].x, ys0 = p.ytab[y0].x;
    const int nc = min(p.xtab[xl].x + 6 - xs0, PS_SC), nr = min(p.ytab[yl].x + 6 - ys0, PS_SR);

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

    // 2. horizontal pass: lane = output column, wave w takes rows w, w + 4, ... of each channel
    {
        const int dxl = tid & 63, w = tid >> 6;
        const int4 xt = p.xtab[min(x0 + dxl, p.dW - 1)];
        const int xo = xt.x - xs0;
        int q[6];
        unpack_taps(xt, q);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            for (int r = w; r < nr; r += 4) {
                const uint16_t *row = &codes[ch][r][xo];
                int acc = 0;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc += __mul24((int)row[k], q[k]);
                hor[ch][r][dxl] = acc;
            }
        }
    }
    __syncthreads();

    // 3. vertical pass + store: lane = four pixels (tid & 15) of output row (tid >> 4) and of the row 16 below
#pragma unroll
    for (int pass = 0; pass < PS_TH / 16; ++pass) {
        const int g = tid & 15, dy = y0 + (tid >> 4) + 16 * pass;
        const int4 yt = p.ytab[min(dy, p.dH - 1)];
        const int ro = yt.x - ys0;
        int q[6];
        unpack_taps(yt, q);
        uint32_t o[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            long long acc[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int4 h = *reinterpret_cast<const int4 *>(&hor[ch][ro + k][4 * g]);
                acc[0] += (long long)h.x * q[k];
                acc[1] += (long long)h.y * q[k];
                acc[2] += (long long)h.z * q[k];
                acc[3] += (long long)h.w * q[k];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long v = (acc[j] + (1LL << 27)) >> 28;
                o[ch][j] = (uint32_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
            }
        }
        const int dx = x0 + 4 * g;
        if (dy < p.dH && dx < p.dW) {
            uint16_t *d = p.dst + ((size_t)dy * p.dW + dx) * 3;
            if (dx + 3 < p.dW && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
                uint2 *d2 = reinterpret_cast<uint2 *>(d);
                d2[0] = make_uint2(o[0][0] | (o[1][0] << 16), o[2][0] | (o[0][1] << 16));
                d2[1] = make_uint2(o[1][1] | (o[2][1] << 16), o[0][2] | (o[1][2] << 16));
                d2[2] = make_uint2(o[2][2] | (o[0][3] << 16), o[1][3] | (o[2][3] << 16));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (dx + j < p.dW) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) d[j * 3 + ch] = (uint16_t)o[ch][j];
                    }
                }
            }
        }
    }
}

}  // namespace

// pq != 0 needs p.pq_bnd (hdrtv_api.hip pq_boundaries).  Needs dH >= H, dW >= W: the LDS footprint bound rests on it.
hipError_t post_scale_launch(const PostScaleParams &p, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || (pq && !p.pq_bnd)) return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH), b(256);
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((post_scale_kernel<float, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((post_scale_kernel<float, false>), g, b, 0, s, p);
    } else {
        if (pq) hipLaunchKernelGGL((post_scale_kernel<f16, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((post_scale_kernel<f16, false>), g, b, 0, s, p);
    }
    return hipGetLastError();
}
