// scale_tables.h -- the host-built tables of the four RGB48 scaler families (the rules: include/hdrtv_mi355x.h), as plain C++17:
// no HIP header and no HIP call, so that a stand-alone host program can run every builder (tests/test_scale_tables_host.py holds
// them to the NumPy references entry for entry).  Per family: the per-axis builder, the layout of the one blob a geometry uploads
// (byte offsets, used by the builder to fill it and by hdrtv_api.hip to slice the device copy), and build_<family>().
// All arithmetic is double, in a fixed order: the GPU tests hold the kernels to the references bit for bit through these tables.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "scale_tiles.h"

namespace scale_tables {

struct I4 { int x, y, z, w; };     // uploaded as int4
struct I2 { int x, y; };           // uploaded as int2

enum Kind { LANCZOS = 0, FSR, DOWN, SSIMSR, NKINDS };

// What a geometry (H, W) -> (dH, dW) uploads: one blob, and the scalars a launch needs beside it (the downscaler's taps per index).
struct Built {
    std::vector<char> blob;
    int ntx = 0, nty = 0;
};

constexpr double PI = 3.14159265358979323846;

inline int float_bits(float v)
{
    int b;
    memcpy(&b, &v, sizeof b);
    return b;
}

// cnt weights -> integer coefficients that sum to 16384: divided by their sum (taken in tap order), rounded half up, the remainder
// to the largest coefficient (the lowest k on a tie)
inline void quantise_taps(const double *w, int cnt, int *q)
{
    double sum = 0.0;
    for (int k = 0; k < cnt; ++k) sum += w[k];
    int tot = 0, big = 0;
    for (int k = 0; k < cnt; ++k) {
        q[k] = (int)std::floor(w[k] / sum * 16384.0 + 0.5);
        tot += q[k];
        if (q[k] > q[big]) big = k;
    }
    q[big] += 16384 - tot;
}

inline double lanczos3(double x)
{
    auto sinc = [](double v) { return v == 0.0 ? 1.0 : std::sin(PI * v) / (PI * v); };
    return std::fabs(x) < 3.0 ? sinc(x) * sinc(x / 3.0) : 0.0;
}
inline double spline36(double x)
{
    x = std::fabs(x);
    if (x < 1.0) return ((13.0 / 11.0 * x - 453.0 / 209.0) * x - 3.0 / 209.0) * x + 1.0;
    if (x < 2.0) { const double y = x - 1.0; return ((-6.0 / 11.0 * y + 270.0 / 209.0) * y - 156.0 / 209.0) * y; }
    if (x < 3.0) { const double y = x - 2.0; return ((1.0 / 11.0 * y - 45.0 / 209.0) * y + 26.0 / 209.0) * y; }
    return 0.0;
}

// Six-tap table of one axis, n source -> m >= n destination samples: per destination index the first of six source taps (i0 - 2,
// unclamped) and six int16 coefficients that sum to 16384, packed in pairs.
template <class Kernel>
inline void six_taps(int n, int m, Kernel kernel, I4 *out)
{
    for (int d = 0; d < m; ++d) {
        const double c = (d + 0.5) * n / m - 0.5, f = std::floor(c), t = c - f;
        double w[6];
        for (int k = 0; k < 6; ++k) w[k] = kernel(t - (k - 2));
        int q[6];
        quantise_taps(w, 6, q);
        auto pack = [](int lo, int hi) { return (int)(((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16)); };
        out[d] = I4{(int)f - 2, pack(q[0], q[1]), pack(q[2], q[3]), pack(q[4], q[5])};
    }
}

// ---- hdrtv_post_rgb48_scaled*: I4 xtab [dW], ytab [dH]
inline size_t lanczos_ytab(int dW) { return (size_t)dW * sizeof(I4); }
inline bool build_lanczos(int H, int W, int dH, int dW, Built &b)
{
    b.blob.resize(((size_t)dW + dH) * sizeof(I4));
    I4 *t = reinterpret_cast<I4 *>(b.blob.data());
    six_taps(W, dW, lanczos3, t);
    six_taps(H, dH, lanczos3, t + dW);
    return true;
}

// ---- hdrtv_post_rgb48_fsr: I2 xtab [dW], ytab [dH]; per destination index fp = floor(p) and the bits of the float32 pp = p - fp
inline void fsr_positions(int n, int m, I2 *out)
{
    for (int d = 0; d < m; ++d) {
        const double p = (d + 0.5) * n / m - 0.5, f = std::floor(p);
        out[d] = I2{(int)f, float_bits((float)(p - f))};
    }
}
inline size_t fsr_ytab(int dW) { return (size_t)dW * sizeof(I2); }
inline bool build_fsr(int H, int W, int dH, int dW, Built &b)
{
    b.blob.resize(((size_t)dW + dH) * sizeof(I2));
    I2 *t = reinterpret_cast<I2 *>(b.blob.data());
    fsr_positions(W, dW, t);
    fsr_positions(H, dH, t + dW);
    return true;
}

// ---- hdrtv_post_rgb48_down.  One axis, n source -> m destination samples, m <= n <= 4 m: per destination index {first tap, tap
// count, the two inner taps of the pull}, the Mitchell coefficients (int, sum 16384) and the Catmull-Rom weights of the L2 passes
// (divided by their sum in double, then float32), both padded with zeros to nt = the largest count.
struct DownAxis {
    std::vector<I4> info;
    std::vector<int> q;
    std::vector<float> w;
    int nt = 1;
};
inline void down_axis(int n, int m, DownAxis &t)
{
    t.info.resize(m);
    if (m == n) {                                 // one tap, k = d, weight one; the pull of an identity is a no-op on any pair of taps
        t.nt = 1;
        t.q.assign(m, 16384);
        t.w.assign(m, 1.f);
        for (int d = 0; d < m; ++d) t.info[d] = I4{d, 1, d, d};
        return;
    }
    auto mitchell = [](double x) {
        x = std::fabs(x);
        if (x < 1.0) return ((7.0 * x - 12.0) * x * x + 16.0 / 3.0) / 6.0;
        if (x < 2.0) return ((((-7.0 / 3.0) * x + 12.0) * x - 20.0) * x + 32.0 / 3.0) / 6.0;
        return 0.0;
    };
    auto catrom = [](double x) {
        x = std::fabs(x);
        if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
        return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    };
    const double hw = 2.0 * n / m;
    int nt = 1;
    for (int d = 0; d < m; ++d) {
        const double ctr = (d + 0.5) * n / m;
        const int lo = (int)std::ceil(ctr - hw - 0.5), hi = (int)std::floor(ctr + hw - 0.5), k2 = (int)std::floor(ctr - 0.5);
        t.info[d] = I4{lo, hi - lo + 1, k2, k2 + 1};
        nt = std::max(nt, hi - lo + 1);
    }
    t.nt = nt;
    t.q.assign((size_t)m * nt, 0);
    t.w.assign((size_t)m * nt, 0.f);
    for (int d = 0; d < m; ++d) {
        const double ctr = (d + 0.5) * n / m;
        const int lo = t.info[d].x, cnt = t.info[d].y;
        double v[17], cr[17], cs = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const double x = (lo + k + 0.5 - ctr) * m / n;
            v[k] = mitchell(x);
            cr[k] = catrom(x);
            cs += cr[k];
        }
        quantise_taps(v, cnt, &t.q[(size_t)d * nt]);
        for (int k = 0; k < cnt; ++k) t.w[(size_t)d * nt + k] = (float)(cr[k] / cs);
    }
}
// I4 xinfo [dW], yinfo [dH]; int xq [dW * ntx], yq [dH * nty]; float xw, yw of the same extents
struct DownLayout { size_t yinfo, xq, yq, xw, yw, bytes; };
inline DownLayout down_layout(int dH, int dW, int ntx, int nty)
{
    const size_t nqx = (size_t)dW * ntx, nqy = (size_t)dH * nty;
    DownLayout l;
    l.yinfo = (size_t)dW * sizeof(I4);
    l.xq = l.yinfo + (size_t)dH * sizeof(I4);
    l.yq = l.xq + nqx * sizeof(int);
    l.xw = l.yq + nqy * sizeof(int);
    l.yw = l.xw + nqx * sizeof(float);
    l.bytes = l.yw + nqy * sizeof(float);
    return l;
}
template <class T>
inline void put(std::vector<char> &blob, size_t at, const std::vector<T> &v) { memcpy(blob.data() + at, v.data(), v.size() * sizeof(T)); }
inline bool build_down(int H, int W, int dH, int dW, Built &b)
{
    DownAxis ax, ay;
    down_axis(W, dW, ax);
    down_axis(H, dH, ay);
    b.ntx = ax.nt;
    b.nty = ay.nt;
    const DownLayout l = down_layout(dH, dW, ax.nt, ay.nt);
    b.blob.resize(l.bytes);
    put(b.blob, 0, ax.info), put(b.blob, l.yinfo, ay.info);
    put(b.blob, l.xq, ax.q), put(b.blob, l.yq, ay.q);
    put(b.blob, l.xw, ax.w), put(b.blob, l.yw, ay.w);
    return true;
}

// ---- hdrtv_post_rgb48_ssimsr.  One axis, n source -> m destination samples, n < m <= 2 n.  Per destination index: sp, the spline36
// taps in six_taps' form; fin, {ip, the bits of the Hann weights at -1, 0, 1}.  Per source index: low, {first tap of the step-4
// footprint (unclamped), tap count, b0, the bits of f}; w, SR_NT weights (divided by their sum in double, then float32, zero-padded).
struct SsimsrAxis {
    std::vector<I4> sp, fin, low;
    std::vector<float> w;
};
inline bool ssimsr_axis(int n, int m, SsimsrAxis &t)
{
    auto mn = [](double x) {
        const double b = 0.334, c = 0.333;
        x = std::fabs(x);
        if (x < 1.0) return ((2.0 - 1.5 * b - c) * x + (-3.0 + 2.0 * b + c)) * x * x + (1.0 - b / 3.0);
        return (((-b / 6.0 - c) * x + (b + 5.0 * c)) * x + (-2.0 * b - 8.0 * c)) * x + (4.0 / 3.0 * b + 4.0 * c);
    };
    t.sp.resize(m);
    t.fin.resize(m);
    six_taps(n, m, spline36, t.sp.data());
    for (int d = 0; d < m; ++d) {
        const double c = (d + 0.5) * n / m - 0.5;
        const double ip = std::floor(c + 0.5), off = c - ip;           // GLSL's round with the tie going up
        t.fin[d] = I4{(int)ip, float_bits((float)std::cos(PI * (-1.0 - off) / 3.0)), float_bits((float)std::cos(PI * (0.0 - off) / 3.0)),
                      float_bits((float)std::cos(PI * (1.0 - off) / 3.0))};
    }
    t.low.resize(n);
    t.w.assign((size_t)n * SR_NT, 0.f);
    const double hw = 2.0 * m / n;
    for (int j = 0; j < n; ++j) {
        const double ctr = (j + 0.5) * m / n;
        const int lo = (int)std::ceil(ctr - hw - 0.5), hi = (int)std::floor(ctr + hw - 0.5), cnt = hi - lo + 1;
        if (cnt < 1 || cnt > SR_NT) return false;
        double v[SR_NT], s = 0.0;
        for (int k = 0; k < cnt; ++k) {
            v[k] = mn((lo + k + 0.5 - ctr) * n / m);
            s += v[k];
        }
        for (int k = 0; k < cnt; ++k) t.w[(size_t)j * SR_NT + k] = (float)(v[k] / s);
        const double u = ctr - 0.5, b0 = std::floor(u);
        t.low[j] = I4{lo, cnt, (int)b0, float_bits((float)(u - b0))};
    }
    return true;
}

// What post_ssimsr.hip's header derives, checked on the tables themselves: along one axis, every tile's regions fit the kernel's
// arrays and every index a phase reads lies in the region the phase before it filled.
inline bool ssimsr_axis_fits(const SsimsrAxis &t, int n, int m, int T, bool ssim)
{
    auto cl = [](int v, int hi) { return std::min(std::max(v, 0), hi); };
    for (int d0 = 0; d0 < m; d0 += T) {
        const int d1 = std::min(d0 + T, m) - 1;
        int fa = 0, fb = 0, la = 0, lb = 0, pa = d0, pb = d1;
        if (ssim) {
            fa = std::max(t.fin[d0].x - 1, 0), fb = std::min(t.fin[d1].x + 1, n - 1);
            la = std::max(fa - 1, 0), lb = std::min(fb + 1, n - 1);
            pa = std::max(t.low[la].x, 0), pb = std::min(t.low[lb].x + t.low[lb].y - 1, m - 1);
        }
        const int ca = std::max(t.sp[pa].x, 0), cb = std::min(t.sp[pb].x + 5, n - 1);
        if (pa > pb || ca > cb || pb - pa + 1 > sr_np(ssim, T) || cb - ca + 1 > sr_nc(ssim, T)) return false;
        for (int d = pa; d <= pb; ++d)
            if (cl(t.sp[d].x, n - 1) < ca || cl(t.sp[d].x + 5, n - 1) > cb) return false;
        if (!ssim) continue;
        if (fa > fb || lb - la + 1 > sr_nl(T) || fb - fa + 1 > T + 2 || la < ca || lb > cb || d0 < pa || d1 > pb) return false;
        for (int j = la; j <= lb; ++j) {
            const I4 e = t.low[j];
            if (cl(e.x, m - 1) < pa || cl(e.x + e.y - 1, m - 1) > pb || cl(e.z, m - 1) < pa || cl(e.z + 1, m - 1) > pb) return false;
        }
        for (int d = d0; d <= d1; ++d)
            if (cl(t.fin[d].x - 1, n - 1) < fa || cl(t.fin[d].x + 1, n - 1) > fb || t.fin[d].x < 0 || t.fin[d].x > n - 1) return false;
    }
    return true;
}
// I4 xsp [dW], ysp [dH], xfin [dW], yfin [dH], xlow [W], ylow [H]; float xw [W * SR_NT], yw [H * SR_NT]
struct SsimsrLayout { size_t ysp, xfin, yfin, xlow, ylow, xw, yw, bytes; };
inline SsimsrLayout ssimsr_layout(int H, int W, int dH, int dW)
{
    SsimsrLayout l;
    l.ysp = (size_t)dW * sizeof(I4);
    l.xfin = l.ysp + (size_t)dH * sizeof(I4);
    l.yfin = l.xfin + (size_t)dW * sizeof(I4);
    l.xlow = l.yfin + (size_t)dH * sizeof(I4);
    l.ylow = l.xlow + (size_t)W * sizeof(I4);
    l.xw = l.ylow + (size_t)H * sizeof(I4);
    l.yw = l.xw + (size_t)W * SR_NT * sizeof(float);
    l.bytes = l.yw + (size_t)H * SR_NT * sizeof(float);
    return l;
}
// false: the tables of this geometry leave the kernel's tile bounds (with or without stage B: one cache entry serves both)
inline bool build_ssimsr(int H, int W, int dH, int dW, Built &b)
{
    SsimsrAxis ax, ay;
    if (!ssimsr_axis(W, dW, ax) || !ssimsr_axis(H, dH, ay) || !ssimsr_axis_fits(ax, W, dW, SR_TW, false) ||
        !ssimsr_axis_fits(ax, W, dW, SR_TW, true) || !ssimsr_axis_fits(ay, H, dH, SR_TH, false) || !ssimsr_axis_fits(ay, H, dH, SR_TH, true))
        return false;
    const SsimsrLayout l = ssimsr_layout(H, W, dH, dW);
    b.blob.resize(l.bytes);
    put(b.blob, 0, ax.sp), put(b.blob, l.ysp, ay.sp);
    put(b.blob, l.xfin, ax.fin), put(b.blob, l.yfin, ay.fin);
    put(b.blob, l.xlow, ax.low), put(b.blob, l.ylow, ay.low);
    put(b.blob, l.xw, ax.w), put(b.blob, l.yw, ay.w);
    return true;
}

}   // namespace scale_tables
