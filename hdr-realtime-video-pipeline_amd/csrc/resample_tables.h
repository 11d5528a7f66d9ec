// resample_tables.h -- the host-built tables of the letterbox (8- and 10-bit), of the full-reference chain's INTER_AREA reduction and
// of the PQ quantiser, as plain C++17: no HIP header and no HIP call, so that a stand-alone host program can run every builder
// (tests/test_resample_tables_host.py holds them entry for entry to oracle/letterbox_oracle.py and to the ST.2084 formula).  Geometry
// and tables of _letterbox_bgr (gui_scaling.py:228-244) as restated in that oracle: OpenCV's computeResizeAreaTab and 11-bit cubic
// coefficients.  hdrtv_api.hip uploads a Built's words and slices the device copy by its offsets.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace resample_tables {

enum Mode { COPY = 0, AREA_INT = 1, AREA_FRAC = 2, CUBIC = 3 };      // common.h's LB_* (hdrtv_api.hip asserts it)

// ---- the letterbox of an (sh, sw) frame into (dh, dw): the resized size, where it is pasted, which resize gets it there and, for
// AREA_INT, the integer shrink factors
struct Geometry { int new_w, new_h, x0, y0, mode, ix, iy; };
inline Geometry letterbox_geometry(int sh, int sw, int dh, int dw)
{
    Geometry g{};
    const double scale = std::min(dw / (double)std::max(sw, 1), dh / (double)std::max(sh, 1));
    g.new_w = std::max(1, (int)std::nearbyint(sw * scale));          // Python round(): half to even
    g.new_h = std::max(1, (int)std::nearbyint(sh * scale));
    g.x0 = (dw - g.new_w) / 2; g.y0 = (dh - g.new_h) / 2;
    g.mode = g.new_w == sw && g.new_h == sh ? COPY : (scale < 1.0 ? AREA_FRAC : CUBIC);
    if (g.mode != AREA_FRAC) return g;
    const double sx = sw / (double)g.new_w, sy = sh / (double)g.new_h;
    const int ix = (int)std::nearbyint(sx), iy = (int)std::nearbyint(sy);
    if (std::fabs(sx - ix) < DBL_EPSILON && std::fabs(sy - iy) < DBL_EPSILON) { g.mode = AREA_INT; g.ix = ix; g.iy = iy; }
    return g;
}

// ---- one axis of a resize, ssize -> dsize samples.  Area (computeResizeAreaTab, built in double): destination index d owns the run
// beg[d] .. beg[d + 1] of source indices src[] and float weights w[].  Cubic: src[d] is the first of four source taps (unclamped),
// co[4 d ..] their coefficients.
struct Axis { std::vector<int> beg, src, co; std::vector<float> w; };
inline Axis area_axis(int ssize, int dsize)
{
    const double sc = ssize / (double)dsize;
    Axis t;
    t.beg.assign(dsize + 1, 0);
    for (int dx = 0; dx < dsize; ++dx) {
        t.beg[dx] = (int)t.src.size();
        const double f1 = dx * sc, f2 = f1 + sc, cell = std::min(sc, ssize - f1);
        int s1 = (int)std::ceil(f1), s2 = (int)std::floor(f2);
        s2 = std::min(s2, ssize - 1); s1 = std::min(s1, s2);
        if (s1 - f1 > 1e-3) { t.src.push_back(s1 - 1); t.w.push_back((float)((s1 - f1) / cell)); }
        for (int q = s1; q < s2; ++q) { t.src.push_back(q); t.w.push_back((float)(1.0 / cell)); }
        if (f2 - s2 > 1e-3) { t.src.push_back(s2); t.w.push_back((float)(std::min(std::min(f2 - s2, 1.0), cell) / cell)); }
    }
    t.beg[dsize] = (int)t.src.size();
    return t;
}

// what is wrong with an area axis the full-reference kernel cannot walk (a run is empty, leaves the ssize samples or steps back), or null
inline const char *area_runs_err(const Axis &t, int ssize)
{
    for (size_t i = 0; i + 1 < t.beg.size(); ++i) {
        if (t.beg[i + 1] <= t.beg[i]) return "empty area run";
        for (int k = t.beg[i]; k < t.beg[i + 1]; ++k)
            if (t.src[k] < 0 || t.src[k] >= ssize || (k > 0 && t.src[k] < t.src[k - 1])) return "area run leaves the source";
    }
    return nullptr;
}

// INTER_CUBIC: the Keys kernel A = -0.75 in float, op by op (volatile: no contraction, no excess precision); cvRound(c * 2048) as int16
inline Axis cubic_axis(int ssize, int dsize)
{
    const double sc = ssize / (double)dsize;
    Axis t{{}, std::vector<int>(dsize), std::vector<int>(4 * (size_t)dsize), {}};
    const float A = -0.75f;
    for (int d = 0; d < dsize; ++d) {
        float fx = (float)((d + 0.5) * sc - 0.5);
        const int s0 = (int)std::floor(fx);
        fx = fx - (float)s0;
        t.src[d] = s0 - 1;
        volatile float c0 = ((A * (fx + 1.f) - 5.f * A) * (fx + 1.f) + 8.f * A) * (fx + 1.f) - 4.f * A;
        volatile float c1 = ((A + 2.f) * fx - (A + 3.f)) * fx * fx + 1.f;
        volatile float c2 = ((A + 2.f) * (1.f - fx) - (A + 3.f)) * (1.f - fx) * (1.f - fx) + 1.f;
        volatile float c3 = 1.f - c0 - c1 - c2;
        const float cs[4] = {c0, c1, c2, c3};
        for (int k = 0; k < 4; ++k) {
            const float r = std::nearbyint(cs[k] * 2048.f);
            t.co[4 * (size_t)d + k] = (int)std::max(-32768.f, std::min(32767.f, r));
        }
    }
    return t;
}

// ---- what a geometry uploads: the two axes' tables in one array of 32-bit words, the ints first, then the floats (as their
// bits), and the word offset of each table (an empty table takes no room)
struct Layout { size_t xbeg = 0, ybeg = 0, xsrc = 0, ysrc = 0, xc = 0, yc = 0, xw = 0, yw = 0; };
struct Built : Layout {
    std::vector<int32_t> words;
    size_t bytes() const { return words.size() * sizeof(int32_t); }
};
inline Built pack(const Axis &x, const Axis &y)
{
    Built b;
    auto put = [&b](const auto &v) {                 // ints, or floats as their bits -> where they start
        const size_t at = b.words.size();
        b.words.resize(at + v.size());
        if (!v.empty()) memcpy(&b.words[at], v.data(), v.size() * sizeof(int32_t));
        return at;
    };
    b.xbeg = put(x.beg); b.xsrc = put(x.src); b.xc = put(x.co); b.ybeg = put(y.beg); b.ysrc = put(y.src); b.yc = put(y.co);
    b.xw = put(x.w); b.yw = put(y.w);
    return b;
}

// ---- ST.2084 OETF in double precision (constants gui_objective_metrics.py:63-67) -> u16 code, floor(pq * 65535 + 0.5): the
// definition the oracle's orc_pq_code states.  bnd[v] = the smallest fp32 y in [0, 1] with code(y) >= v.
inline int pq_code64(float y)
{
    const double yp = std::pow((double)y, 0.1593017578125);
    const double v = std::pow((0.8359375 + 18.8515625 * yp) / (1.0 + 18.6875 * yp), 78.84375);
    const double q = std::floor(v * 65535.0 + 0.5);
    return (int)(q < 0.0 ? 0.0 : (q > 65535.0 ? 65535.0 : q));
}
constexpr int PQ_GUESS_BASE = (127 - 27) << 6, PQ_GUESS_N = 27 * 64 + 2;      // the first-guess table behind the 65536 boundaries
inline void pq_boundaries(std::vector<float> &bnd)
{
    bnd.assign(65536, 0.f);
    for (int v = 1; v <= 65535; ++v) {
        // analytic inverse (EOTF) as the first guess, then walk the fp32 grid to the exact boundary
        const double p = ((double)v - 0.5) / 65535.0, t = std::pow(p, 1.0 / 78.84375);
        const double num = std::max(t - 0.8359375, 0.0), den = 18.8515625 - 18.6875 * t;
        float f = (float)std::min(1.0, std::max(0.0, std::pow(num / den, 1.0 / 0.1593017578125)));
        while (f > 0.f && pq_code64(std::nextafterf(f, -1.f)) >= v) f = std::nextafterf(f, -1.f);
        while (f < 1.f && pq_code64(f) < v) f = std::nextafterf(f, 2.f);
        bnd[v] = f;
    }
    // first-guess table of the kernel (prepost.hip pq_code): exact codes at the fp32 values ((127 - 27) * 64 + i) << 17
    bnd.resize(65536 + PQ_GUESS_N);
    for (int i = 0; i < PQ_GUESS_N; ++i) {
        const uint32_t bits = (uint32_t)(PQ_GUESS_BASE + i) << 17;
        float y;
        memcpy(&y, &bits, 4);
        bnd[65536 + i] = (float)pq_code64(y > 1.f ? 1.f : y);
    }
}

// ---- the way back, for the tone map (post_tonemap.hip): lin[c] = the fp32 nearest to the ST.2084 EOTF of c / 65535 (1.0 = 10000
// nits), then moved along the fp32 grid until pq_code64(lin[c]) == c.  So the round trip code -> level -> code is the identity on
// all 65536 codes, and a level scaled by exactly 1.0f comes back as the code it was read from.
inline void pq_eotf_table(std::vector<float> &lin)
{
    lin.assign(65536, 0.f);
    for (int c = 1; c <= 65535; ++c) {
        const double t = std::pow((double)c / 65535.0, 1.0 / 78.84375);
        const double num = std::max(t - 0.8359375, 0.0), den = 18.8515625 - 18.6875 * t;
        float f = (float)std::min(1.0, std::max(0.0, std::pow(num / den, 1.0 / 0.1593017578125)));
        while (f < 1.f && pq_code64(f) < c) f = std::nextafterf(f, 2.f);
        while (f > 0.f && pq_code64(f) > c) f = std::nextafterf(f, -1.f);
        lin[c] = f;
    }
}

}  // namespace resample_tables
