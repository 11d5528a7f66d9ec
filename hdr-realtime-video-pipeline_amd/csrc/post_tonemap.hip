// post_tonemap.hip -- the tone map of frames at the size they are delivered at (gfx950): hdrtv_rgb48_tonemap (u16 RGB48 codes of
// BT.2020 PQ -> tone-mapped codes) and hdrtv_post_rgb48_tonemap (the model's tensor -> quant_rgb, plain or PQ -> tone-mapped codes,
// one launch, no codes in device memory in between).  include/hdrtv_mi355x.h states the pixel rule, tests/tonemap_ref.py restates
// it in NumPy:
//       m = max(R, G, B);  g = gain[m];  per channel c:  y = lin[c] * g (one float32 multiply);  out = pq_code_level(y)
// The curve is the caller's gain[65536]; lin[65536] (resample_tables.h pq_eotf_table) and the PQ code boundaries are the context's.
// The file is built with -ffp-contract=off like film_grain.hip: the rule's multiply stands alone.  quant_u16's multiply-add does not
// notice (tests/test_film_grain_host.py), so the fused kernel starts from post_rgb48_kernel's codes.
//
// Access: a lane takes eight neighbouring pixels of a row, 48 bytes of packed codes, as three 16-byte loads and three 16-byte stores
// where the row's addresses allow (a pitch of W * 6 bytes keeps 16-byte alignment on every row only when W % 8 == 0); code by code
// otherwise and at a row's ragged end.  A wave covers 512 consecutive pixels of one row, so its accesses are contiguous; a
// workgroup takes four rows, the grid strides over the rest.  A pixel depends on itself only: dst == src is allowed, each lane has
// read its 48 bytes (code by code: its pixel) before it writes them.  Per pixel 1 + 3 gathers from gain and lin and three table
// walks over the boundaries: three 256 KiB tables, L2-resident, and neighbouring pixels of video hit neighbouring entries.  The
// eight pixels of a lane go through ONE copy of the three walks: a rolled loop that takes the pixel in the low 48 bits of the lane's
// 384-bit register, shifts the register down by 48 and puts the result on top, so after eight turns the results stand where the
// sources stood.  Eight inlined copies would not fit the registers (light_stats.hip rolls its PQ form for the same reason).  No
// LDS, no scratch (tests/test_isa_tonemap.py).
#include "launchers.h"
#include "post_quant.h"

namespace {

constexpr int TM_ROWS = 4;                  // rows per workgroup: one wave each

__device__ __forceinline__ bool tm_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct ToneTables { const float *gain, *lin, *bnd; };

// the rule on one pixel's codes
__device__ __forceinline__ void tone_px(uint32_t &q0, uint32_t &q1, uint32_t &q2, const ToneTables &t)
{
    const float g = t.gain[max(q0, max(q1, q2))];
    q0 = pq_code_level(__fmul_rn(t.lin[q0], g), t.bnd);
    q1 = pq_code_level(__fmul_rn(t.lin[q1], g), t.bnd);
    q2 = pq_code_level(__fmul_rn(t.lin[q2], g), t.bnd);
}

// eight pixels' codes, pixel 0 in the low 48 bits: pixel 0 leaves, the others move down, (q0, q1, q2) becomes pixel 7
__device__ __forceinline__ void tm_rotate48(uint32_t (&w)[12], uint32_t q0, uint32_t q1, uint32_t q2)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) w[i] = (w[i + 1] >> 16) | (w[i + 2] << 16);
    w[10] = (w[11] >> 16) | (q0 << 16);
    w[11] = q1 | (q2 << 16);
}

__device__ __forceinline__ void tm_store8(uint16_t *d, const uint32_t (&w)[12])
{
    uint4 *d4 = reinterpret_cast<uint4 *>(d);
    d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
    d4[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// eight neighbouring values of a plane, 16-byte aligned
__device__ __forceinline__ void tm_plane8(const f16 *p, float (&v)[8])
{
    const f16x8 x = *reinterpret_cast<const f16x8 *>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)x[j];
}
__device__ __forceinline__ void tm_plane8(const float *p, float (&v)[8])
{
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// codes -> tone-mapped codes; src and dst may be the same frame (never __restrict__)
__global__ __launch_bounds__(256) void rgb48_tonemap_kernel(const uint16_t *src, uint16_t *dst, int H, int W, ToneTables t)
{
    const int x = 8 * (blockIdx.x * 64 + (threadIdx.x & 63));
    if (x >= W) return;
    const int n = min(8, W - x);
    for (int y = blockIdx.y * TM_ROWS + (threadIdx.x >> 6); y < H; y += gridDim.y * TM_ROWS) {
        const size_t o = ((size_t)y * W + x) * 3;
        const uint16_t *s = src + o;
        uint16_t *d = dst + o;
        if (n == 8 && tm_aligned16(s) && tm_aligned16(d)) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
            const uint4 a = s4[0], b = s4[1], c = s4[2];
            uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll 1
            for (int i = 0; i < 8; ++i) {
                uint32_t q0 = w[0] & 0xffffu, q1 = w[0] >> 16, q2 = w[1] & 0xffffu;
                tone_px(q0, q1, q2, t);
                tm_rotate48(w, q0, q1, q2);
            }
            tm_store8(d, w);
        } else {
#pragma unroll 1
            for (int i = 0; i < n; ++i) {
                uint32_t q0 = s[i * 3], q1 = s[i * 3 + 1], q2 = s[i * 3 + 2];
                tone_px(q0, q1, q2, t);
                d[i * 3] = (uint16_t)q0; d[i * 3 + 1] = (uint16_t)q1; d[i * 3 + 2] = (uint16_t)q2;
            }
        }
    }
}

// planar tensor [3][H][W] -> quant_rgb -> tone-mapped codes
template <typename T, bool PQ>
__global__ __launch_bounds__(256) void post_rgb48_tonemap_kernel(const T *__restrict__ in, uint16_t *__restrict__ rgb, int H, int W, float peak,
                                                                 ToneTables t)
{
    const int x = 8 * (blockIdx.x * 64 + (threadIdx.x & 63));
    if (x >= W) return;
    const int n = min(8, W - x);
    const size_t plane = (size_t)H * W;
    for (int y = blockIdx.y * TM_ROWS + (threadIdx.x >> 6); y < H; y += gridDim.y * TM_ROWS) {
        const size_t o = (size_t)y * W + x;
        const T *p = in + o;
        uint16_t *d = rgb + o * 3;
        if (n == 8 && tm_aligned16(p) && tm_aligned16(p + plane) && tm_aligned16(p + 2 * plane) && tm_aligned16(d)) {
            float r[8], g[8], b[8];
            tm_plane8(p, r);
            tm_plane8(p + plane, g);
            tm_plane8(p + 2 * plane, b);
            uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
            for (int i = 0; i < 8; ++i) {
                uint32_t q0, q1, q2;
                quant_rgb<PQ>(r[0], g[0], b[0], peak, t.bnd, q0, q1, q2);
#pragma unroll
                for (int j = 0; j < 7; ++j) { r[j] = r[j + 1]; g[j] = g[j + 1]; b[j] = b[j + 1]; }
                tone_px(q0, q1, q2, t);
                tm_rotate48(w, q0, q1, q2);
            }
            tm_store8(d, w);
        } else {
#pragma unroll 1
            for (int i = 0; i < n; ++i) {
                uint32_t q0, q1, q2;
                quant_rgb<PQ>((float)p[i], (float)p[plane + i], (float)p[2 * plane + i], peak, t.bnd, q0, q1, q2);
                tone_px(q0, q1, q2, t);
                d[i * 3] = (uint16_t)q0; d[i * 3 + 1] = (uint16_t)q1; d[i * 3 + 2] = (uint16_t)q2;
            }
        }
    }
}

// 64 groups of eight pixels per workgroup along x, TM_ROWS rows along y; at most 65535 workgroups along y, the rest by strides
inline dim3 tm_grid(int H, int W)
{
    const int gx = ((W + 7) / 8 + 63) / 64, gy = (H + TM_ROWS - 1) / TM_ROWS;
    return dim3(gx, gy < 65535 ? gy : 65535);
}

}  // namespace

// H, W >= 1 and every pointer given; hipErrorInvalidValue, nothing enqueued, otherwise
hipError_t rgb48_tonemap_launch(const uint16_t *src, uint16_t *dst, int H, int W, const float *gain, const float *lin, const float *pq_bnd,
                                hipStream_t s)
{
    if (!src || !dst || !gain || !lin || !pq_bnd || H < 1 || W < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rgb48_tonemap_kernel, tm_grid(H, W), dim3(256), 0, s, src, dst, H, W, ToneTables{gain, lin, pq_bnd});
    return hipGetLastError();
}

// the same conditions (the walk needs pq_bnd whatever pq is)
hipError_t post_rgb48_tonemap_launch(const void *in, int is_f32, int H, int W, uint16_t *rgb, int pq, float peak, const float *gain,
                                     const float *lin, const float *pq_bnd, hipStream_t s)
{
    if (!in || !rgb || !gain || !lin || !pq_bnd || H < 1 || W < 1) return hipErrorInvalidValue;
    const dim3 g = tm_grid(H, W), b(256);
    const ToneTables t{gain, lin, pq_bnd};
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((post_rgb48_tonemap_kernel<float, true>), g, b, 0, s, (const float *)in, rgb, H, W, peak, t);
        else hipLaunchKernelGGL((post_rgb48_tonemap_kernel<float, false>), g, b, 0, s, (const float *)in, rgb, H, W, peak, t);
    } else {
        if (pq) hipLaunchKernelGGL((post_rgb48_tonemap_kernel<f16, true>), g, b, 0, s, (const f16 *)in, rgb, H, W, peak, t);
        else hipLaunchKernelGGL((post_rgb48_tonemap_kernel<f16, false>), g, b, 0, s, (const f16 *)in, rgb, H, W, peak, t);
    }
    return hipGetLastError();
}
