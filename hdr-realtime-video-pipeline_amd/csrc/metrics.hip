// metrics.hip -- the reference's objective metrics core on the device: PSNR, SSIM
// (11x11 Gaussian, sigma 1.5, reflect-101 borders) and dE-ITP (BT.2124) between two unit-range images
// [3][H][W] (R, G, B planes; f16 or f32) -- src/gui_objective_metrics.py:438-528 as restated in
// oracle/metrics_oracle.py (parity unpinned: that module needs cv2).  One 16x16-pixel tile per workgroup,
// per-workgroup fp64 partial sums, summed in index order on the host: results are reproducible bit for bit.
// A load policy says where the two images come from: PlanarLoad<T> is the above; CodeLoad<NORM> reads two interleaved
// u16 [H][W][3] RGB48 frames as float32(code) / 65535 (the full-reference chain, include/hdrtv_mi355x.h R4), and with NORM
// passes the first frame's codes through the grade match while it loads them (R6): no normalised frame exists in memory.
#include "launchers.h"

namespace {

constexpr int MT = 16, R = 5, HT = MT + 2 * R;   // 26 x 26 halo tile
__constant__ float c_gauss[11];

__device__ __forceinline__ int reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

template <typename T>
__device__ __forceinline__ float ld(const void *p, size_t i) { return (float)reinterpret_cast<const T *>(p)[i]; }

__device__ __forceinline__ float pq_oetf(float lum)
{
    const float y = fminf(fmaxf(lum / 10000.0f, 0.f), 1.f);
    const float ym = powf(y, 2610.0f / 16384.0f);
    const float num = 3424.0f / 4096.0f + (2413.0f / 128.0f) * ym;
    const float den = 1.0f + (2392.0f / 128.0f) * ym;
    return powf(num / fmaxf(den, 1e-12f), 2523.0f / 32.0f);
}

__device__ __forceinline__ void to_itp(const float rgb[3], float out[3])
{
    const float l = (1688.0f * rgb[0] + 2146.0f * rgb[1] + 262.0f * rgb[2]) / 4096.0f;
    const float m = (683.0f * rgb[0] + 2951.0f * rgb[1] + 462.0f * rgb[2]) / 4096.0f;
    const float s = (99.0f * rgb[0] + 309.0f * rgb[1] + 3688.0f * rgb[2]) / 4096.0f;
    const float lp = pq_oetf(l), mp = pq_oetf(m), sp = pq_oetf(s);
    out[0] = 0.5f * lp + 0.5f * mp;
    out[1] = 0.5f * ((6610.0f * lp - 13613.0f * mp + 7003.0f * sp) / 4096.0f);
    out[2] = (17933.0f * lp - 17390.0f * mp - 543.0f * sp) / 4096.0f;
}

// x * g + b as two float32 operations: the empty asm keeps the backend from contracting them into one FMA, which
// -ffp-contract=fast (this file's setting, and what the planar instantiations' bits depend on) would otherwise do
__device__ __forceinline__ float mul_then_add(float x, float g, float b)
{
    float t = x * g;
    asm volatile("" : "+v"(t));
    return t + b;
}

__device__ __forceinline__ float pick3(const float (&v)[3], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

template <typename T>
struct PlanarLoad {
    static constexpr bool NORM = false;
    static __device__ __forceinline__ void load(const MetricsParams &p, int c, int y, int x, float &a, float &b)
    {
        const size_t idx = c * ((size_t)p.H * p.W) + (size_t)y * p.W + x;
        a = ld<T>(p.a, idx);
        b = ld<T>(p.b, idx);
    }
};

template <bool NORM_>
struct CodeLoad {
    static constexpr bool NORM = NORM_;
    static __device__ __forceinline__ void load(const MetricsParams &p, int c, int y, int x, float &a, float &b)
    {
        const size_t idx = (size_t)y * p.pitch + (size_t)x * 3 + c;
        float fa = (float)reinterpret_cast<const uint16_t *>(p.a)[idx];
        if (NORM)          // trunc(clip(code * gain + bias, 0, 65535)): the reference's .astype(uint16)
            fa = (float)(int)fminf(fmaxf(mul_then_add(fa, pick3(p.gain, c), pick3(p.bias, c)), 0.f), 65535.f);
        a = fa / 65535.0f;
        b = (float)reinterpret_cast<const uint16_t *>(p.b)[idx] / 65535.0f;
    }
    // the first frame's absolute RGB after the grade match in cd/m^2, from its raw codes
    static __device__ __forceinline__ void abs_norm(const MetricsParams &p, int y, int x, float out[3])
    {
        const uint16_t *px = reinterpret_cast<const uint16_t *>(p.a) + (size_t)y * p.pitch + (size_t)x * 3;
        const float peak = fmaxf(1.0f, p.peak_nits);
        for (int c = 0; c < 3; ++c) {
            const float v = fminf(fmaxf((float)px[c] / 65535.0f, 0.f), 1.f) * p.peak_nits;
            out[c] = fminf(fmaxf(mul_then_add(v, p.gain_abs[c], p.bias_abs[c]), 0.f), peak);
        }
    }
};

template <typename LD>
__global__ __launch_bounds__(256) void metrics_kernel(MetricsParams p)
{
    __shared__ float s_a[HT][HT + 1], s_b[HT][HT + 1];
    __shared__ float s_h[5][HT][MT + 1];          // horizontally blurred a, b, a*a, b*b, a*b
    __shared__ double s_red[3][256];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
    const int x = x0 + tx, y = y0 + ty;
    const bool in = x < p.W && y < p.H;
    double se = 0.0, ss = 0.0, de = 0.0;
    float ca[3], cb[3];
    for (int c = 0; c < 3; ++c) {
        __syncthreads();
        for (int e = tid; e < HT * HT; e += 256) {
            const int r = e / HT, q = e % HT;
            LD::load(p, c, reflect101(y0 - R + r, p.H), reflect101(x0 - R + q, p.W), s_a[r][q], s_b[r][q]);
        }
        __syncthreads();
        for (int e = tid; e < HT * MT; e += 256) {
            const int r = e / MT, q = e % MT;
            float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < 11; ++i) {
                const float a = s_a[r][q + i], b = s_b[r][q + i], k = c_gauss[i];
                h[0] += a * k; h[1] += b * k; h[2] += (a * a) * k; h[3] += (b * b) * k; h[4] += (a * b) * k;
            }
            for (int j = 0; j < 5; ++j) s_h[j][r][q] = h[j];
        }
        __syncthreads();
        ca[c] = s_a[ty + R][tx + R];
        cb[c] = s_b[ty + R][tx + R];
        if (in) {
            float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < 11; ++i)
                for (int j = 0; j < 5; ++j) v[j] += s_h[j][ty + i][tx] * c_gauss[i];
            const float mu_a = v[0], mu_b = v[1];
            const float sa = v[2] - mu_a * mu_a, sb = v[3] - mu_b * mu_b, sab = v[4] - mu_a * mu_b;
            const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
            const float num = (2.0f * mu_a * mu_b + c1) * (2.0f * sab + c2);
            const float den = (mu_a * mu_a + mu_b * mu_b + c1) * (sa + sb + c2);
            ss += (double)(num / (den + 1e-12f));
            const float d = ca[c] - cb[c];
            se += (double)(d * d);
        }
    }
    if (in) {
        float ra[3], rb[3], ia[3], ib[3];
        for (int c = 0; c < 3; ++c) {
            ra[c] = fminf(fmaxf(ca[c], 0.f), 1.f) * p.peak_nits;
            rb[c] = fminf(fmaxf(cb[c], 0.f), 1.f) * p.peak_nits;
        }
        if constexpr (LD::NORM) LD::abs_norm(p, y, x, ra);
        to_itp(ra, ia);
        to_itp(rb, ib);
        const float di = ia[0] - ib[0], dt = ia[1] - ib[1], dp = ia[2] - ib[2];
        de = (double)(720.0f * sqrtf(di * di + dt * dt + dp * dp + 1e-12f));
    }
    s_red[0][tid] = se; s_red[1][tid] = ss; s_red[2][tid] = de;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {          // fixed tree: the same sum every run
        if (tid < o)
            for (int j = 0; j < 3; ++j) s_red[j][tid] += s_red[j][tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        double *out = p.partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        out[0] = s_red[0][0]; out[1] = s_red[1][0]; out[2] = s_red[2][0];
    }
}

}  // namespace

int metrics_blocks(int H, int W) { return ((W + MT - 1) / MT) * ((H + MT - 1) / MT); }

static hipError_t gauss_init()
{
    static bool init = false;
    if (!init) {
        float k[11];
        double sum = 0.0, kd[11];
        for (int i = 0; i < 11; ++i) { const double x = i - 5.0; kd[i] = exp(-(x * x) / (2.0 * 1.5 * 1.5)); sum += kd[i]; }
        for (int i = 0; i < 11; ++i) k[i] = (float)(kd[i] / sum);
        hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_gauss), k, sizeof k);
        if (e != hipSuccess) return e;
        init = true;
    }
    return hipSuccess;
}

hipError_t metrics_launch(const MetricsParams &p, hipStream_t s)
{
    if (hipError_t e = gauss_init(); e != hipSuccess) return e;
    const dim3 grid((p.W + MT - 1) / MT, (p.H + MT - 1) / MT);
    if (p.is_f32) hipLaunchKernelGGL(metrics_kernel<PlanarLoad<float>>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(metrics_kernel<PlanarLoad<f16>>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t metrics_u16_launch(const MetricsParams &p, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.pitch < 3 * p.W) return hipErrorInvalidValue;
    if (hipError_t e = gauss_init(); e != hipSuccess) return e;
    const dim3 grid((p.W + MT - 1) / MT, (p.H + MT - 1) / MT);
    if (p.norm) hipLaunchKernelGGL(metrics_kernel<CodeLoad<true>>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(metrics_kernel<CodeLoad<false>>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}
