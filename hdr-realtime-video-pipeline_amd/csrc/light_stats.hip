// light_stats.hip -- the HDR10 content light level record of a frame on the device (gfx950): hdrtv_light_stats /
// hdrtv_rgb48_light_stats (include/hdrtv_mi355x.h states the rule).  A reduction, not a map: a 4096-bin histogram of
// m = max(R, G, B) over the u16 codes the sink receives, the three channel maxima, max m and the u64 sum of m, over a rectangle of
// the frame.  Two sources, as post_ycbcr.hip has: the model's planar f16 / f32 tensor (quantised with post_quant.h's quant_rgb, plain
// or PQ, so the codes are exactly hdrtv_post_rgb48's / hdrtv_post_pq_rgb48's) and RGB48 codes already in device memory.
//
// A fixed, capped grid of 256-lane workgroups; each strides over the eight-pixel groups of the rectangle's rows.  Groups start at
// frame columns that are multiples of 8, so a rectangle with an odd x0 still loads wide and masks its first and last group:
//   load     one 16-byte load per plane per lane (f16; two for f32; three for RGB48 codes) where the group lies inside the row and its
//            addresses are 16-byte aligned; element by element otherwise (W not a multiple of 8, plane starts that an odd H * W moves
//            off 16 bytes, the last group of a ragged row) -- only pixels inside the rectangle are read then, one per lane at a time.
//   bins     each pixel is quantised once; bin = m >> 4 into a u32 histogram in LDS (16 KiB).  Video is flat: letterbox bars and skies
//            put every lane of a wave on one bin, where one LDS add per pixel would serialise.  A lane first combines equal bins among
//            its eight pixels into one add with a count; and when all eight agree in every lane of the wave with the first lane's
//            bin (ballot + popcount) the wave issues ONE add.  The element-wise path takes one pixel of every lane at a time and
//            applies the same wave test to it.
//   maxima   the channel maxima, max m and the u64 sum stay in registers across the loop, are reduced in the wave (shuffles), across
//            the four waves through LDS, and leave the workgroup as one global atomic per quantity.
//   flush    the workgroup walks its 4096 bins (starting at a 256-bin block that rotates with the workgroup index, so the workgroups
//            of a wave front do not all knock on the same cache lines) and issues a no-return global add for non-zero bins only.
// The launcher zeroes the record on the same stream in front of the kernel.  Everything is integer arithmetic -- adds and maxima of
// integers commute -- so the record is identical from run to run and does not depend on the grid size or on the order in which
// lanes, waves and workgroups arrive.
// 16 KiB + 96 bytes of LDS; no scratch and at most 64 VGPRs, so the 32 waves of a CU (eight workgroups) fit
// (tests/test_isa_light_stats.py pins both from the kernel descriptors).
#include "launchers.h"
#include "post_quant.h"
#include "../../include/hdrtv_mi355x.h"

namespace {

constexpr int LS_BINS = HDRTV_LIGHT_BINS;
static_assert(LS_BINS == 4096 && HDRTV_LIGHT_WORDS == LS_BINS + 8, "bin = code >> 4; eight words behind the histogram");

__device__ __forceinline__ bool ls_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the model's planar tensor: the codes hdrtv_post_rgb48 (PQ = false) / hdrtv_post_pq_rgb48 (PQ = true) write
template <typename T, bool PQ>
struct LsTensorSrc {
    const T *in;
    size_t plane;
    int W;
    float peak;
    const float *bnd;

    __device__ __forceinline__ const T *at(int y, int x) const { return in + (size_t)y * W + x; }
    // pixels x .. x + 7 of row y lie inside the row and each plane's eight start at a 16-byte boundary
    __device__ __forceinline__ bool wide(int y, int x) const
    {
        const T *p = at(y, x);
        return x + 8 <= W && ls_aligned16(p) && ls_aligned16(p + plane) && ls_aligned16(p + 2 * plane);
    }
    __device__ __forceinline__ void load8(const T *p, float (&v)[8]) const
    {
        if (sizeof(T) == 2) {
            const f16x8 x = *reinterpret_cast<const f16x8 *>(p);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
        } else {
            const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
    }
    struct Raw { float v[3][8]; };
    __device__ __forceinline__ void raw8(int y, int x, Raw &w) const       // needs wide(y, x)
    {
        const T *p = at(y, x);
        load8(p, w.v[0]);
        load8(p + plane, w.v[1]);
        load8(p + 2 * plane, w.v[2]);
    }
    __device__ __forceinline__ void code(const Raw &w, int i, uint32_t (&q)[3]) const
    {
        quant_rgb<PQ>(w.v[0][i], w.v[1][i], w.v[2][i], peak, bnd, q[0], q[1], q[2]);
    }
    // PQ: the eight pixels go through ONE copy of the table walk (a rolled loop that takes pixel 0 and moves the others down);
    // eight inlined copies of it do not fit 64 VGPRs
    static constexpr bool ROLLED = PQ;
    __device__ __forceinline__ void shift(Raw &w) const
    {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int i = 0; i < 7; ++i) w.v[ch][i] = w.v[ch][i + 1];
        }
    }
    __device__ __forceinline__ void px1(int y, int x, uint32_t (&q)[3]) const
    {
        const T *p = at(y, x);
        quant_rgb<PQ>((float)p[0], (float)p[plane], (float)p[2 * plane], peak, bnd, q[0], q[1], q[2]);
    }
};

// RGB48 codes already in device memory: u16 [H][W][3]
struct LsRgb48Src {
    const uint16_t *in;
    int W;

    __device__ __forceinline__ const uint16_t *at(int y, int x) const { return in + ((size_t)y * W + x) * 3; }
    __device__ __forceinline__ bool wide(int y, int x) const { return x + 8 <= W && ls_aligned16(at(y, x)); }
    struct Raw { uint32_t w[12]; };
    __device__ __forceinline__ void raw8(int y, int x, Raw &r) const       // needs wide(y, x)
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(at(y, x));
        const uint4 a = p[0], b = p[1], c = p[2];
        r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w; r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
        r.w[8] = c.x; r.w[9] = c.y; r.w[10] = c.z; r.w[11] = c.w;
    }
    __device__ __forceinline__ void code(const Raw &r, int i, uint32_t (&q)[3]) const
    {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int e = 3 * i + ch;
            q[ch] = (e & 1) ? (r.w[e >> 1] >> 16) : (r.w[e >> 1] & 0xffffu);
        }
    }
    static constexpr bool ROLLED = false;
    __device__ __forceinline__ void shift(Raw &) const {}
    __device__ __forceinline__ void px1(int y, int x, uint32_t (&q)[3]) const
    {
        const uint16_t *p = at(y, x);
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
};

// `n` pixels of every lane that reaches this call (the wave's active lanes; control flow may have diverged) fall into that lane's bin
// `b`, valid or not as `ok` says.  When every such lane is ok and agrees with the first, the first adds for all of them.
__device__ __forceinline__ void hist_add(uint32_t *hist, uint32_t b, bool ok, uint32_t n, int lane)
{
    const unsigned long long act = __ballot(1);
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    if (__ballot(ok && b == first) == act) {
        if (lane == __ffsll(act) - 1) atomicAdd(&hist[first], n * (uint32_t)__popcll(act));
    } else if (ok) {
        atomicAdd(&hist[b], n);
    }
}

template <typename SRC>
__device__ __forceinline__ void light_body(const SRC &src, const LightStatsParams &p)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[LS_BINS];
    __shared__ uint32_t red[4][6];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < LS_BINS / 4; i += 256) reinterpret_cast<uint4 *>(hist)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    // groups of eight pixels at frame columns gx0 + 8 c: gpr per row of the rectangle, `total` in all (the launcher bounds it below 2^31)
    const int gx0 = p.x0 & ~7, x1 = p.x0 + p.rw;
    const uint32_t gpr = (uint32_t)(x1 - gx0 + 7) >> 3, total = gpr * (uint32_t)p.rh;
    uint32_t mr = 0, mg = 0, mb = 0, mm = 0;
    unsigned long long sum = 0;
    for (uint32_t g = blockIdx.x * 256u + (uint32_t)tid; g < total; g += gridDim.x * 256u) {
        const uint32_t r = g / gpr, c = g - r * gpr;
        const int x = gx0 + 8 * (int)c, y = p.y0 + (int)r;
        const int lo = max(p.x0 - x, 0), hi = min(x1 - x, 8);              // pixels lo .. hi - 1 of the group lie in the rectangle
        if (src.wide(y, x)) {
            typename SRC::Raw raw;
            uint32_t bin[8], s = 0;
            src.raw8(y, x, raw);
            // one pixel: its codes (0 outside the rectangle) into the maxima and the sum; returns its bin, outside the rectangle a
            // value no pixel and no other slot has
            auto pixel = [&](int k, int i) -> uint32_t {
                uint32_t q[3];
                src.code(raw, k, q);
                const bool ok = i >= lo && i < hi;
                const uint32_t r16 = ok ? q[0] : 0u, g16 = ok ? q[1] : 0u, b16 = ok ? q[2] : 0u;
                const uint32_t m = max(r16, max(g16, b16));
                mr = max(mr, r16);
                mg = max(mg, g16);
                mb = max(mb, b16);
                mm = max(mm, m);
                s += m;
                return ok ? (m >> 4) : (uint32_t)(LS_BINS + i);
            };
            if (SRC::ROLLED) {
                uint32_t bp[4] = {0, 0, 0, 0};                             // the bins so far, 16 bits each, the newest on top
#pragma unroll 1
                for (int i = 0; i < 8; ++i) {
                    const uint32_t b = pixel(0, i);
                    src.shift(raw);
                    bp[0] = (bp[0] >> 16) | (bp[1] << 16);
                    bp[1] = (bp[1] >> 16) | (bp[2] << 16);
                    bp[2] = (bp[2] >> 16) | (bp[3] << 16);
                    bp[3] = (bp[3] >> 16) | (b << 16);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) bin[i] = (i & 1) ? (bp[i >> 1] >> 16) : (bp[i >> 1] & 0xffffu);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) bin[i] = pixel(i, i);
            }
            sum += s;
            uint32_t same0 = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) same0 += bin[i] == bin[0];
            const bool uni = same0 == 8;                                   // eight pixels of the rectangle in one bin: the flat case
            if (__ballot(uni) == __ballot(1)) {
                hist_add(hist, bin[0], true, 8, lane);
            } else {
                // equal bins among the eight become one add with a count
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    uint32_t cnt = 1;
                    bool dup = false;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (j < i) dup |= bin[j] == bin[i];
                        if (j > i) cnt += bin[j] == bin[i];
                    }
                    if (bin[i] < (uint32_t)LS_BINS && !dup) atomicAdd(&hist[bin[i]], cnt);
                }
            }
        } else {
            // element by element, only what lies in the rectangle; one pixel of every lane at a time, so a flat frame still costs
            // one add per wave and pixel
#pragma unroll 1
            for (int i = lo; i < hi; ++i) {
                uint32_t q[3];
                src.px1(y, x + i, q);
                const uint32_t m = max(q[0], max(q[1], q[2]));
                mr = max(mr, q[0]);
                mg = max(mg, q[1]);
                mb = max(mb, q[2]);
                mm = max(mm, m);
                sum += m;
                hist_add(hist, m >> 4, true, 1, lane);
            }
        }
    }
    __syncthreads();

    // maxima and sum: the wave, then the four waves through LDS, then one global atomic each
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mr = max(mr, (uint32_t)__shfl_xor((int)mr, off));
        mg = max(mg, (uint32_t)__shfl_xor((int)mg, off));
        mb = max(mb, (uint32_t)__shfl_xor((int)mb, off));
        mm = max(mm, (uint32_t)__shfl_xor((int)mm, off));
        sum += __shfl_xor(sum, off);
    }
    if (lane == 0) {
        uint32_t *w = red[tid >> 6];
        w[0] = mr; w[1] = mg; w[2] = mb; w[3] = mm; w[4] = (uint32_t)sum; w[5] = (uint32_t)(sum >> 32);
    }
    __syncthreads();
    if (tid < 4) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) v = max(v, red[w][tid]);
        if (v) atomicMax(&p.stats[LS_BINS + tid], v);
    } else if (tid == 4) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += (unsigned long long)red[w][4] | ((unsigned long long)red[w][5] << 32);
        if (s) atomicAdd(reinterpret_cast<unsigned long long *>(p.stats + LS_BINS + 4), s);
    } else if (tid == 5 && blockIdx.x == 0) {
        p.stats[LS_BINS + 6] = (uint32_t)p.rw * (uint32_t)p.rh;
    }
    for (int i = 0; i < LS_BINS / 256; ++i) {
        const int b = ((i + (int)blockIdx.x) & (LS_BINS / 256 - 1)) * 256 + tid;
        const uint32_t v = hist[b];
        if (v) atomicAdd(&p.stats[b], v);
    }
}

template <typename T, bool PQ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void light_stats_kernel(LightStatsParams p)
{
    const LsTensorSrc<T, PQ> src{static_cast<const T *>(p.in), (size_t)p.H * p.W, p.W, p.peak, p.pq_bnd};
    light_body(src, p);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void rgb48_light_stats_kernel(LightStatsParams p)
{
    const LsRgb48Src src{static_cast<const uint16_t *>(p.in), p.W};
    light_body(src, p);
}

// the rectangle lies inside the frame, the record is 8-byte aligned (its u64 sum), and the pixel and group counts fit 32 bits:
// every load and every atomic of the kernel rests on these
bool light_params_ok(const LightStatsParams &p)
{
    if (!p.in || !p.stats || (reinterpret_cast<uintptr_t>(p.stats) & 7) || p.H < 1 || p.W < 1) return false;
    if (p.rw < 1 || p.rh < 1 || p.x0 < 0 || p.y0 < 0 || p.x0 > p.W - p.rw || p.y0 > p.H - p.rh) return false;
    return ((long long)p.rw / 8 + 2) * p.rh <= 0x7fffffffLL - 0x1000000LL && (long long)p.rw * p.rh <= 0xffffffffLL;
}

int light_grid(const LightStatsParams &p, int max_wgs)
{
    const long long gpr = ((p.x0 + p.rw) - (p.x0 & ~7) + 7) >> 3, wgs = (gpr * p.rh + 255) / 256;
    return (int)std::min<long long>(wgs, std::min(std::max(1, max_wgs), 0xffff));     // 0xffff * 256 < 2^24: the kernel's group index cannot wrap
}

}  // namespace

// Zeroes the record and launches; max_wgs caps the grid (the record does not depend on it).
hipError_t light_stats_launch(const LightStatsParams &p, int is_f32, int pq, int max_wgs, hipStream_t s)
{
    if (!light_params_ok(p) || (pq && !p.pq_bnd)) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(p.stats, 0, HDRTV_LIGHT_WORDS * sizeof(uint32_t), s)) return e;
    const dim3 g(light_grid(p, max_wgs));
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((light_stats_kernel<float, true>), g, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((light_stats_kernel<float, false>), g, dim3(256), 0, s, p);
    } else {
        if (pq) hipLaunchKernelGGL((light_stats_kernel<f16, true>), g, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((light_stats_kernel<f16, false>), g, dim3(256), 0, s, p);
    }
    return hipGetLastError();
}

hipError_t rgb48_light_stats_launch(const LightStatsParams &p, int max_wgs, hipStream_t s)
{
    if (!light_params_ok(p)) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(p.stats, 0, HDRTV_LIGHT_WORDS * sizeof(uint32_t), s)) return e;
    hipLaunchKernelGGL(rgb48_light_stats_kernel, dim3(light_grid(p, max_wgs)), dim3(256), 0, s, p);
    return hipGetLastError();
}
