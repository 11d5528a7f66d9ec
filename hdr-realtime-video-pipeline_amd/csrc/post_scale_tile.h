// post_scale_tile.h -- the tile body of the fused quantise + Lanczos-3 upscale (gfx950), shared by post_scale.hip (AR = false:
// hdrtv_post_rgb48_scaled, nothing of the anti-ringing is compiled), post_scale_ar.hip (AR = true: hdrtv_post_rgb48_scaled_ex
// with a strength of 1 .. 256) and post_scale_cas.hip (CAS = true, AR either: hdrtv_post_rgb48_scaled_cas, contrast-adaptive
// sharpening of the codes in front of the passes).  include/hdrtv_mi355x.h states the three integer rules.
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
// Anti-ringing (AR) pulls the sum of each pass towards the interval of its two inner taps, k = 2 and 3, the samples that bracket
// the sampling position: sum += ((clamp(sum, lo, hi) - sum) * a + 128) >> 8 with lo / hi = min / max of the two taps << 14.  The
// horizontal pass has both as row[2] / row[3] in registers, the vertical pass as the k = 2, 3 row segments it has loaded anyway:
// no LDS beyond the plain form's and no second read, only vector ALU.  The products stay off the 64-bit multiplier:
//   horizontal  d fits int32 (|d| < 2^31; measured < 2^28): d = dh * 256 + dl, dl = d & 255, and
//               (d * a + 128) >> 8 = dh * a + ((dl * a + 128) >> 8) exactly, both products 24-bit (|dh| < 2^23, a <= 256)
//   vertical    |d| < 2^46: d = dh * 65536 + dl, dl = d & 65535, and
//               (d * a + 128) >> 8 = dh * (a * 256) + ((dl * a + 128) >> 8), the first one 32 x 32 -> 64 multiply-add, dl * a < 2^24
// LDS banks (MI355X_MICROARCH.md): the horizontal reads of a wave are 64 u16 addresses that rise by at most one element per lane
// (same dword = broadcast), its writes 64 consecutive dwords; the vertical ds_read_b128 of a 16-lane group covers one 256-byte
// row of `hor` (rows are 64 dwords apart, so lanes of different output rows in a group still hit different banks).
// 16.0 KiB + 28.5 KiB of LDS: three workgroups per CU.
// Sharpening (CAS) splits the staging in two.  1a quantises the footprint with a halo of one pixel -- rows [ys0 - 1, ys0 + nr],
// columns [xs0 - 1, xs0 + nc], clamped to the frame like the footprint itself -- into raw[ch][40][72] u16, 16.9 KiB that lie in
// `hor`'s storage: `hor` is not written before the horizontal pass, and raw is dead once `codes` is complete, so the barrier that
// already separates staging from the horizontal pass separates the two uses, and 1a / 1b need one barrier more.  1b writes
// codes[ch][r][c] = the sharpened code of the FRAME pixel (cy, cx) = clamp(ys0 + r), clamp(xs0 + c), whose neighbours are the frame
// pixels clamp(cy +- 1), clamp(cx +- 1): a tap outside the frame reads the sharpened edge pixel, as the rule has it, not a pixel
// sharpened from neighbours that were clamped by position.  Frame row y lies at raw row y - (ys0 - 1), which is inside 0 .. nr + 1
// for every row asked for (ys0 <= H - 3 and ys0 + nr - 1 >= 2, from the tap tables), columns alike; no index is clamped twice.
// A lane takes one pixel and its three channels; consecutive lanes take consecutive columns, so the nine u16 reads of a wave are
// 64 consecutive u16 = 32 consecutive dwords (two lanes per dword broadcast), split over two rows 36 dwords apart at a row's end.
// The two floor divisions and the root are a float reciprocal / root and one exact integer correction step each (ps_cas below).
// Film grain (GRAIN, post_scale_grain.hip: hdrtv_post_rgb48_scaled_grain) replaces each code written to `codes` -- step 1's, or step
// 1b's sharpened one -- by its grained code (film_grain.h) at the FRAME pixel it belongs to, the clamped (sy, sx) / (cy, cx) over
// H x W: in the reference's chain the grain hooks MAIN at the processing size, behind ffmpeg's cas and in front of mpv's scaler, so a
// tap outside the frame reads the grained edge pixel.  One g per staged pixel, three grain_code; vector ALU only, the LDS of the twin.
#pragma once
#include "common.h"
#include "post_quant.h"
#include "film_grain.h"

constexpr int PS_SR = PS_TH + 6, PS_SC = PS_TW + 6, PS_SCP = PS_SC + 2;

__device__ __forceinline__ void ps_unpack_taps(const int4 t, int (&q)[6])
{
    q[0] = (t.y << 16) >> 16; q[1] = t.y >> 16;
    q[2] = (t.z << 16) >> 16; q[3] = t.z >> 16;
    q[4] = (t.w << 16) >> 16; q[5] = t.w >> 16;
}

// the horizontal pass's anti-ringing: sum in int32, the inner taps as u16 codes, a in 1 .. 256
__device__ __forceinline__ int ps_antiring_h(int raw, int t2, int t3, int a)
{
    const int lo = min(t2, t3) << 14, hi = max(t2, t3) << 14;
    const int d = min(max(raw, lo), hi) - raw;
    return raw + __mul24(d >> 8, a) + ((__mul24(d & 255, a) + 128) >> 8);
}

// the vertical pass's: sum in int64, the inner taps as values of `hor`
__device__ __forceinline__ long long ps_antiring_v(long long raw, int h2, int h3, int a)
{
    const long long lo = (long long)min(h2, h3) << 14, hi = (long long)max(h2, h3) << 14;
    const long long d = (raw < lo ? lo : (raw > hi ? hi : raw)) - raw;
    const int dh = (int)(d >> 16), dl = (int)(d & 0xffff);
    return raw + (long long)dh * (a << 8) + ((__mul24(dl, a) + 128) >> 8);
}

// The sharpened code of e in the 3 x 3 neighbourhood a b c / d e f / g h i, K = the CAS code 1032 .. 4096 (include/hdrtv_mi355x.h
// states the rule).  Every product is 24 x 24 bits.
//   r = floor(n / m), n = q << 15 < 2^31, m <= 131070, r <= 32768: the float estimate n * rcp(m) is off by less than 2^-6 (three
//       roundings of 2^-23 relative on a value <= 2^15), so its truncation is r or r +- 1 and the remainder says which.
//   A = floor(sqrt(x)), x = r << 9 <= 2^24 exact in float, the root within one ulp of a value <= 4096: A or A +- 1, squares decide.
//   floor(N / den), |N| < 2^31, 128 <= den <= 65536: only quotients inside +-65535 can survive the clamp of e + quotient, so the
//       estimate is clamped to +-70000 first (there it is off by less than 2^-5; beyond, the true quotient is beyond +-69990 and the
//       result saturates whatever the correction does), then corrected by its remainder, which fits int32 where it matters.
__device__ __forceinline__ uint32_t ps_cas(int a, int b, int c, int d, int e, int f, int g, int h, int i, int K)
{
    const int mn5 = min(min(min(b, d), min(f, h)), e), mx5 = max(max(max(b, d), max(f, h)), e);
    const int mn = mn5 + min(mn5, min(min(a, c), min(g, i))), mx = mx5 + max(mx5, max(max(a, c), max(g, i)));
    const int n = min(mn, 131070 - mx) << 15, m = max(mx, 1);
    int r = (int)((float)n * __builtin_amdgcn_rcpf((float)m));
    const int rr = n - __mul24(r, m);
    r += (rr >= m) - (rr < 0);
    const int x = r << 9;
    int A = (int)__builtin_amdgcn_sqrtf((float)x);
    A += (__mul24(A + 1, A + 1) <= x) - (__mul24(A, A) > x);
    const int den = 16 * K - 4 * A;
    const int N = __mul24(A, 4 * e - (b + d + f + h)) + (den >> 1);
    int v = (int)floorf(fminf(fmaxf((float)N * __builtin_amdgcn_rcpf((float)den), -70000.f), 70000.f));
    const int vr = N - __mul24(v, den);
    v += (vr >= den) - (vr < 0);
    return (uint32_t)min(max(e + v, 0), 65535);
}

constexpr int PS_RR = PS_SR + 2, PS_RC = PS_SC + 2;        // the raw codes of the CAS form: the footprint and its halo

// a = the anti-ringing strength, 1 .. 256 (read only where AR); cas = the CAS code, 1032 .. 4096 (read only where CAS); intensity, seed
// = the film grain's (read only where GRAIN)
template <typename T, bool PQ, bool AR, bool CAS = false, bool GRAIN = false>
__device__ __forceinline__ void post_scale_tile(const PostScaleParams p, const int a, const int cas = 0, const float intensity = 0.f,
                                                const float seed = 0.f)
{
    __shared__ uint16_t codes[3][PS_SR][PS_SCP];
    __shared__ __attribute__((aligned(16))) int hor[3][PS_SR][PS_TW];
    static_assert(sizeof(uint16_t) * 3 * PS_RR * PS_RC <= sizeof(hor), "the raw codes of the CAS form lie in hor");
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PS_TW, y0 = blockIdx.y * PS_TH;
    const int xl = min(x0 + PS_TW, p.dW) - 1, yl = min(y0 + PS_TH, p.dH) - 1;
    const int xs0 = p.xtab[x0].x, ys0 = p.ytab[y0].x;
    const int nc = min(p.xtab[xl].x + 6 - xs0, PS_SC), nr = min(p.ytab[yl].x + 6 - ys0, PS_SR);

    // 1a / 1b. stage + quantise with a halo, sharpen
    if constexpr (CAS) {
        uint16_t(*raw)[PS_RR][PS_RC] = reinterpret_cast<uint16_t(*)[PS_RR][PS_RC]>(&hor[0][0][0]);
        const T *__restrict__ in = static_cast<const T *>(p.in);
        const size_t plane = (size_t)p.H * p.W;
        const int nch = nc + 2;
        for (int i = tid; i < (nr + 2) * nch; i += 256) {
            const int r = i / nch, c = i - r * nch;
            const int sy = min(max(ys0 - 1 + r, 0), p.H - 1), sx = min(max(xs0 - 1 + c, 0), p.W - 1);
            const size_t o = (size_t)sy * p.W + sx;
            const float cr = (float)in[o], cg = (float)in[plane + o], cb = (float)in[2 * plane + o];
            uint32_t q0, q1, q2;
            quant_rgb<PQ>(cr, cg, cb, p.peak, p.pq_bnd, q0, q1, q2);
            raw[0][r][c] = (uint16_t)q0;
            raw[1][r][c] = (uint16_t)q1;
            raw[2][r][c] = (uint16_t)q2;
        }
        __syncthreads();
        for (int i = tid; i < nr * nc; i += 256) {
            const int r = i / nc, c = i - r * nc;
            const int cy = min(max(ys0 + r, 0), p.H - 1), cx = min(max(xs0 + c, 0), p.W - 1);
            const int r1 = cy - (ys0 - 1), r0 = max(cy - 1, 0) - (ys0 - 1), r2 = min(cy + 1, p.H - 1) - (ys0 - 1);
            const int c1 = cx - (xs0 - 1), c0 = max(cx - 1, 0) - (xs0 - 1), c2 = min(cx + 1, p.W - 1) - (xs0 - 1);
            [[maybe_unused]] float Ig = 0.f;
            if constexpr (GRAIN) Ig = grain_term(intensity, cx, cy, p.W, p.H, seed);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const uint16_t *t = raw[ch][r0], *m = raw[ch][r1], *b = raw[ch][r2];
                const uint32_t v = ps_cas(t[c0], t[c1], t[c2], m[c0], m[c1], m[c2], b[c0], b[c1], b[c2], cas);
                if constexpr (GRAIN) codes[ch][r][c] = (uint16_t)grain_code(v, Ig);
                else codes[ch][r][c] = (uint16_t)v;
            }
        }
    } else {
        const T *__restrict__ in = static_cast<const T *>(p.in);
        const size_t plane = (size_t)p.H * p.W;
        for (int i = tid; i < nr * nc; i += 256) {
            const int r = i / nc, c = i - r * nc;
            const int sy = min(max(ys0 + r, 0), p.H - 1), sx = min(max(xs0 + c, 0), p.W - 1);
            const size_t o = (size_t)sy * p.W + sx;
            const float cr = (float)in[o], cg = (float)in[plane + o], cb = (float)in[2 * plane + o];
            uint32_t q0, q1, q2;
            quant_rgb<PQ>(cr, cg, cb, p.peak, p.pq_bnd, q0, q1, q2);
            if constexpr (GRAIN) {                   // the grain of the frame pixel (sy, sx), not of the tap's own position
                const float Ig = grain_term(intensity, sx, sy, p.W, p.H, seed);
                q0 = grain_code(q0, Ig);
                q1 = grain_code(q1, Ig);
                q2 = grain_code(q2, Ig);
            }
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
        ps_unpack_taps(xt, q);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            for (int r = w; r < nr; r += 4) {
                const uint16_t *row = &codes[ch][r][xo];
                if constexpr (AR) {
                    int s[6], acc = 0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        s[k] = (int)row[k];
                        acc += __mul24(s[k], q[k]);
                    }
                    hor[ch][r][dxl] = ps_antiring_h(acc, s[2], s[3], a);
                } else {
                    int acc = 0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) acc += __mul24((int)row[k], q[k]);
                    hor[ch][r][dxl] = acc;
                }
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
        ps_unpack_taps(yt, q);
        uint32_t o[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            long long acc[4] = {0, 0, 0, 0};
            [[maybe_unused]] int4 h2, h3;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int4 h = *reinterpret_cast<const int4 *>(&hor[ch][ro + k][4 * g]);
                acc[0] += (long long)h.x * q[k];
                acc[1] += (long long)h.y * q[k];
                acc[2] += (long long)h.z * q[k];
                acc[3] += (long long)h.w * q[k];
                if constexpr (AR) {
                    if (k == 2) h2 = h;
                    if (k == 3) h3 = h;
                }
            }
            if constexpr (AR) {
                acc[0] = ps_antiring_v(acc[0], h2.x, h3.x, a);
                acc[1] = ps_antiring_v(acc[1], h2.y, h3.y, a);
                acc[2] = ps_antiring_v(acc[2], h2.z, h3.z, a);
                acc[3] = ps_antiring_v(acc[3], h2.w, h3.w, a);
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
