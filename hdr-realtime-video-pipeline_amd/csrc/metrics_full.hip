// metrics_full.hip -- what the reference does to two frames before and beside its three metric formulas
// (_compute_full_reference_metrics, src/gui_objective_metrics.py:617-677), on RGB48 codes u16 [H][W][3] in device memory;
// include/hdrtv_mi355x.h states the rules R1 .. R6, tests/metrics_full_ref.py restates them in numpy.
//   border_counts_kernel  R1: signal pixels per row and per column of both frames (integer adds only)
//   area_reduce_kernel    R3: OpenCV's INTER_AREA on 16-bit codes (PARITY UNPINNED against cv2 itself, as letterbox.hip's 8-bit
//                         form: OpenCV is not part of the reference tree); the crop is an offset into the source
//   channel_hist_kernel   R5: six exact histograms (2 frames x 3 channels x 65536 bins)
//   grade_match_host      R5: mean / std / gain / bias from those histograms, on the host in double
// The metric kernel itself is metrics.hip's, through its CodeLoad policy (R4, R6).
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): R3's table path multiplies and adds separately in float32, and the
// host sums of R5 are held to numpy's bits.
#include "launchers.h"

#include <cmath>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------------------- R1
// A workgroup owns BC_ROWS rows x 256 columns of one frame: a thread walks its column down the rows (adjacent threads read adjacent
// pixels), keeps the column's count in a register, and each wave adds its ballot's population to the row's LDS counter.
constexpr int BC_ROWS = 32;

__global__ __launch_bounds__(256) void border_counts_kernel(BorderCountsParams p)
{
    __shared__ uint32_t s_row[BC_ROWS];
    const int tid = threadIdx.x, f = blockIdx.z;
    const int x = blockIdx.x * 256 + tid, y0 = blockIdx.y * BC_ROWS;
    const int rows = min(BC_ROWS, p.H - y0);
    if (tid < BC_ROWS) s_row[tid] = 0;
    __syncthreads();
    const uint16_t *F = f ? p.frame[1] : p.frame[0];
    uint32_t col = 0;
    for (int r = 0; r < rows; ++r) {
        bool sig = false;
        if (x < p.W) {
            const uint16_t *px = F + ((size_t)(y0 + r) * p.W + x) * 3;
            sig = max(max((int)px[0], (int)px[1]), (int)px[2]) >= FR_SIGNAL_MIN;
        }
        col += sig ? 1u : 0u;
        const unsigned long long m = __ballot(sig);
        if ((tid & 63) == 0 && m) atomicAdd(&s_row[r], (uint32_t)__popcll(m));
    }
    __syncthreads();
    uint32_t *out = p.counts + (size_t)f * (p.H + p.W);
    if (tid < rows && s_row[tid]) atomicAdd(out + y0 + tid, s_row[tid]);
    if (x < p.W && col) atomicAdd(out + p.H + x, col);
}

// ---------------------------------------------------------------------------------------------------------------- R3
// One workgroup per output row and strip of FR_STRIP output columns; thread t owns output column t / 3, channel t % 3.  For every
// contributing source row the strip's source segment (at most FR_STRIP * FR_MAX_SHRINK + 2 pixels) is staged into LDS with
// coalesced loads; the thread then walks its own table entries over it, so no sum crosses threads and the order is the rule's.
constexpr int AR_SEG = FR_STRIP * FR_MAX_SHRINK + 2;       // pixels
constexpr int AR_THREADS = FR_STRIP * 3;

__device__ __forceinline__ uint16_t sat_u16_rint(float v)
{
    const float r = rintf(v);                       // cvRound: half to even
    return (uint16_t)(r < 0.f ? 0.f : (r > 65535.f ? 65535.f : r));
}

__global__ __launch_bounds__(AR_THREADS) void area_reduce_kernel(AreaReduceParams p)
{
    __shared__ uint16_t s_seg[AR_SEG * 3];
    const int tid = threadIdx.x, dy = blockIdx.y, f = blockIdx.z;
    const int dx0 = blockIdx.x * FR_STRIP, dx1 = min(dx0 + FR_STRIP, p.nw);
    const int dx = dx0 + tid / 3, ch = tid % 3;
    const bool own = dx < dx1;
    const bool tab = p.mode == FR_AREA_TAB;
    // the strip's source columns [x_lo, x_lo + seg_w) and this thread's run of them
    int x_lo, x_hi, xb = 0, xn = p.ix, yb = 0, yn = p.iy;
    if (tab) {
        x_lo = p.xsrc[p.xbeg[dx0]];
        x_hi = p.xsrc[p.xbeg[dx1] - 1];
        if (own) { xb = p.xbeg[dx]; xn = p.xbeg[dx + 1] - xb; }
        yb = p.ybeg[dy]; yn = p.ybeg[dy + 1] - yb;
    } else {
        x_lo = dx0 * p.ix;
        x_hi = dx1 * p.ix - 1;
    }
    const int seg_n = min(x_hi - x_lo + 1, AR_SEG) * 3;      // u16 elements; the min never binds for a ratio <= FR_MAX_SHRINK
    const uint16_t *S = (f ? p.src[1] : p.src[0]) + (size_t)x_lo * 3;
    float fsum = 0.f;
    int isum = 0;
    for (int j = 0; j < yn; ++j) {
        const int sy = tab ? p.ysrc[yb + j] : dy * p.iy + j;
        const uint16_t *row = S + (size_t)sy * p.pitch;
        __syncthreads();                                     // the previous row's readers are done
        for (int e = tid; e < seg_n; e += AR_THREADS) s_seg[e] = row[e];
        __syncthreads();
        if (!own) continue;
        if (tab) {
            float buf = 0.f;
            for (int i = 0; i < xn; ++i) {
                const int e = min((p.xsrc[xb + i] - x_lo) * 3 + ch, AR_SEG * 3 - 1);
                buf = buf + (float)s_seg[e] * p.xw[xb + i];
            }
            const float beta = p.yw[yb + j];
            fsum = j == 0 ? beta * buf : fsum + beta * buf;
        } else {
            const int e0 = (dx - dx0) * p.ix * 3 + ch;
            for (int i = 0; i < xn; ++i) isum += s_seg[e0 + i * 3];
        }
    }
    if (!own) return;
    uint16_t v;
    if (tab) v = sat_u16_rint(fsum);
    else if (p.mode == FR_AREA_2X2) v = (uint16_t)((isum + 2) >> 2);
    else v = sat_u16_rint((float)isum * __fdiv_rn(1.0f, (float)(p.ix * p.iy)));      // isum < 2^24: exact in float32
    (f ? p.dst[1] : p.dst[0])[((size_t)dy * p.nw + dx) * 3 + ch] = v;
}

// ---------------------------------------------------------------------------------------------------------------- R5
// 65536 u32 bins are 256 KiB per histogram, more than a CU's LDS, so the bins live in device memory and a wave privatises what it
// can in registers instead: the lanes that hold the first active lane's code add their population with one atomic (a flat frame, or
// a black bar, is one atomic per wave and channel), the rest add one each.  Integer atomics: the histogram is exact whatever the order.
__device__ __forceinline__ void hist_add(uint32_t *h, int code, bool active)
{
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const int first = __shfl(code, __ffsll((long long)act) - 1);
    const bool same = active && code == first;
    const unsigned long long m = __ballot(same);
    if (same) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(h + first, (uint32_t)__popcll(m));
    } else if (active) {
        atomicAdd(h + code, 1u);
    }
}

__global__ __launch_bounds__(256) void channel_hist_kernel(ChannelHistParams p)
{
    const int f = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const bool in = x < p.W;
    int c[3] = {0, 0, 0};
    if (in) {
        const uint16_t *px = (f ? p.frame[1] : p.frame[0]) + (size_t)y * p.pitch + (size_t)x * 3;
        c[0] = px[0]; c[1] = px[1]; c[2] = px[2];
    }
    uint32_t *h = p.hist + (size_t)f * 3 * 65536;
    for (int k = 0; k < 3; ++k) hist_add(h + (size_t)k * 65536, c[k], in);
}

}  // namespace

hipError_t border_counts_launch(const BorderCountsParams &p, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || !p.frame[0] || !p.frame[1] || !p.counts) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(p.counts, 0, (size_t)2 * (p.H + p.W) * sizeof(uint32_t), s); e != hipSuccess) return e;
    hipLaunchKernelGGL(border_counts_kernel, dim3((p.W + 255) / 256, (p.H + BC_ROWS - 1) / BC_ROWS, 2), dim3(256), 0, s, p);
    return hipGetLastError();
}

bool area_reduce_size_ok(int sh, int sw, int nh, int nw)
{
    return nh >= 1 && nw >= 1 && nh <= sh && nw <= sw && (long long)sh <= (long long)FR_MAX_SHRINK * nh &&
           (long long)sw <= (long long)FR_MAX_SHRINK * nw;
}

hipError_t area_reduce_launch(const AreaReduceParams &p, hipStream_t s)
{
    if (!area_reduce_size_ok(p.sh, p.sw, p.nh, p.nw) || !p.src[0] || !p.dst[0] || (p.src[1] != nullptr) != (p.dst[1] != nullptr) ||
        p.pitch < 3 * p.sw)
        return hipErrorInvalidValue;
    if (p.mode == FR_AREA_TAB ? !(p.xbeg && p.ybeg && p.xsrc && p.ysrc && p.xw && p.yw)
                              : (p.ix < 1 || p.iy < 1 || p.ix * p.nw != p.sw || p.iy * p.nh != p.sh || (p.mode == FR_AREA_2X2 && (p.ix != 2 || p.iy != 2))))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(area_reduce_kernel, dim3((p.nw + FR_STRIP - 1) / FR_STRIP, p.nh, p.src[1] ? 2 : 1), dim3(AR_THREADS), 0, s, p);
    return hipGetLastError();
}

hipError_t channel_hist_launch(const ChannelHistParams &p, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.pitch < 3 * p.W || !p.frame[0] || !p.frame[1] || !p.hist) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(p.hist, 0, (size_t)6 * 65536 * sizeof(uint32_t), s); e != hipSuccess) return e;
    hipLaunchKernelGGL(channel_hist_kernel, dim3((p.W + 255) / 256, p.H, 2), dim3(256), 0, s, p);
    return hipGetLastError();
}

// R5 on the host: hist = u32 [2][3][65536] (prediction, then ground truth), n = samples per histogram.  Sums run in ascending code
// order in double; an empty bin adds +0.0, which changes no partial sum, so it is skipped.  out12 = gain[3], bias[3] (code domain),
// gain_abs[3], bias_abs[3] (absolute RGB, v(code) = float32(clip(float32(code) / 65535, 0, 1) * peak_nits)), rounded to float32.
void grade_match_host(const uint32_t *hist, double n, float peak_nits, float *out12)
{
    static const std::vector<float> unit = [] {
        std::vector<float> u(65536);
        for (int c = 0; c < 65536; ++c) u[c] = std::fmin(std::fmax((float)c / 65535.0f, 0.f), 1.f);
        return u;
    }();
    // Per histogram: its occupied bins, ascending (an evaluation frame fills a fraction of the 65536; the compaction is branch-free,
    // occupancy being as good as random), then one pass for the two means and one for the two deviations.  The two domains are
    // independent sums, each in the rule's order.
    double mean[2][6], sd[2][6];
    std::vector<int> code(65536 + 1);
    for (int k = 0; k < 6; ++k) {
        const uint32_t *h = hist + (size_t)k * 65536;
        int cnt = 0;
        for (int c = 0; c < 65536; ++c) { code[cnt] = c; cnt += h[c] != 0; }
        double s1c = 0.0, s1a = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const int c = code[i];
            const double hc = (double)h[c];
            s1c = s1c + hc * (double)c;
            s1a = s1a + hc * (double)(float)(unit[c] * peak_nits);
        }
        const double mc = mean[0][k] = s1c / n, ma = mean[1][k] = s1a / n;
        double s2c = 0.0, s2a = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const int c = code[i];
            const double hc = (double)h[c];
            const double dc = (double)c - mc, da = (double)(float)(unit[c] * peak_nits) - ma;
            s2c = s2c + hc * (dc * dc);
            s2a = s2a + hc * (da * da);
        }
        sd[0][k] = std::sqrt(s2c / n);
        sd[1][k] = std::sqrt(s2a / n);
    }
    for (int dom = 0; dom < 2; ++dom)
        for (int ch = 0; ch < 3; ++ch) {
            const double gain = sd[dom][ch] < 1e-6 ? 1.0 : sd[dom][3 + ch] / sd[dom][ch];       // [ch]: prediction, [3 + ch]: ground truth
            const double bias = mean[dom][3 + ch] - gain * mean[dom][ch];
            out12[dom * 6 + ch] = (float)gain;
            out12[dom * 6 + 3 + ch] = (float)bias;
        }
}
