// film_grain.hip -- the film grain on frames at the size they are delivered at (gfx950): hdrtv_rgb48_film_grain (u16 RGB48 codes ->
// grained codes) and hdrtv_post_rgb48_grain (the model's tensor -> quant_rgb, plain or PQ -> grained codes, one launch, no codes in
// device memory in between).  film_grain.h has the pixel rule (include/hdrtv_mi355x.h states it, tests/film_grain_ref.py restates
// it in NumPy); the file is built with -ffp-contract=off, as the rule is float32 operation by operation.  quant_u16's
// multiply-add does not notice: x * 65535 + 0.5 truncates to the same integer fused or not for every float32 x in [0, 1]
// (tests/test_film_grain_host.py), so the fused kernel's codes are post_rgb48_kernel's.
//
// Both kernels give a lane four neighbouring pixels of a row, 24 bytes of codes: three 8-byte accesses where the address allows
// (post_scale_tile.h's store packing; a row pitch of W * 6 bytes leaves 8-byte alignment to even rows or W % 4 == 0), code by code
// otherwise and at a row's ragged end.  A wave covers 256 consecutive pixels of one row, so its accesses are contiguous; a
// workgroup takes four rows, the grid strides over the rest.  A pixel depends on itself only: dst == src is allowed, each lane
// has read its 24 bytes before it writes them.  One g per pixel, three grain_code; a lane keeps its four columns' part of the rule
// (grain_col: two of g's five divisions) across the rows it walks, at least FG_WALK where the frame has them.  The tensor is read
// with one 8- / 16-byte load per plane where the address allows.
#include "launchers.h"
#include "post_quant.h"
#include "film_grain.h"

namespace {

constexpr int FG_ROWS = 4;                  // rows per workgroup: one wave each
constexpr int FG_WALK = 4;                  // rows a lane walks (stride: the grid's rows), sharing grain_col

// c[j][ch] of n <= 4 pixels -> d
__device__ __forceinline__ void fg_store4(uint16_t *d, int n, const uint32_t (&c)[4][3])
{
    if (n == 4 && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
        uint2 *d2 = reinterpret_cast<uint2 *>(d);
        d2[0] = make_uint2(c[0][0] | (c[0][1] << 16), c[0][2] | (c[1][0] << 16));
        d2[1] = make_uint2(c[1][1] | (c[1][2] << 16), c[2][0] | (c[2][1] << 16));
        d2[2] = make_uint2(c[2][2] | (c[3][0] << 16), c[3][1] | (c[3][2] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) d[j * 3 + ch] = (uint16_t)c[j][ch];
            }
        }
    }
}

__device__ __forceinline__ void fg_load4(const uint16_t *s, int n, uint32_t (&c)[4][3])
{
    if (n == 4 && (reinterpret_cast<uintptr_t>(s) & 7) == 0) {
        const uint2 *s2 = reinterpret_cast<const uint2 *>(s);
        const uint2 a = s2[0], b = s2[1], e = s2[2];
        const uint32_t w[6] = {a.x, a.y, b.x, b.y, e.x, e.y};
#pragma unroll
        for (int k = 0; k < 12; ++k) c[k / 3][k % 3] = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[j][ch] = j < n ? (uint32_t)s[j * 3 + ch] : 0u;
        }
    }
}

// n <= 4 neighbouring values of a plane
template <typename T>
__device__ __forceinline__ void fg_plane4(const T *p, int n, float (&v)[4]);
template <>
__device__ __forceinline__ void fg_plane4<f16>(const f16 *p, int n, float (&v)[4])
{
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
        const f16x4 x = *reinterpret_cast<const f16x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)x[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? (float)p[j] : 0.f;
    }
}
template <>
__device__ __forceinline__ void fg_plane4<float>(const float *p, int n, float (&v)[4])
{
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 x = *reinterpret_cast<const float4 *>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? p[j] : 0.f;
    }
}

// codes -> grained codes; src and dst may be the same frame (never __restrict__)
__global__ __launch_bounds__(256) void film_grain_kernel(const uint16_t *src, uint16_t *dst, int H, int W, float intensity, float seed)
{
    const int x = 4 * (blockIdx.x * 64 + (threadIdx.x & 63));
    if (x >= W) return;
    const int n = min(4, W - x);
    float col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = grain_col(x + j, W);
    for (int y = blockIdx.y * FG_ROWS + (threadIdx.x >> 6); y < H; y += gridDim.y * FG_ROWS) {
        const size_t o = ((size_t)y * W + x) * 3;
        const float row = grain_row(y, H);
        uint32_t c[4][3];
        fg_load4(src + o, n, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
                const float Ig = __fmul_rn(intensity, grain_at(col[j], row, seed));
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[j][ch] = grain_code(c[j][ch], Ig);
            }
        }
        fg_store4(dst + o, n, c);
    }
}

// planar tensor [3][H][W] -> quant_rgb -> grained codes
template <typename T, bool PQ>
__global__ __launch_bounds__(256) void post_rgb48_grain_kernel(const T *__restrict__ in, uint16_t *__restrict__ rgb, int H, int W, float peak,
                                                               const float *__restrict__ bnd, float intensity, float seed)
{
    const int x = 4 * (blockIdx.x * 64 + (threadIdx.x & 63));
    if (x >= W) return;
    const int n = min(4, W - x);
    const size_t plane = (size_t)H * W;
    float col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = grain_col(x + j, W);
    for (int y = blockIdx.y * FG_ROWS + (threadIdx.x >> 6); y < H; y += gridDim.y * FG_ROWS) {
        const size_t o = (size_t)y * W + x;
        const float row = grain_row(y, H);
        float r[4], g[4], b[4];
        fg_plane4<T>(in + o, n, r);
        fg_plane4<T>(in + plane + o, n, g);
        fg_plane4<T>(in + 2 * plane + o, n, b);
        uint32_t c[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j][0] = c[j][1] = c[j][2] = 0;
            if (j < n) {
                quant_rgb<PQ>(r[j], g[j], b[j], peak, bnd, c[j][0], c[j][1], c[j][2]);
                const float Ig = __fmul_rn(intensity, grain_at(col[j], row, seed));
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[j][ch] = grain_code(c[j][ch], Ig);
            }
        }
        fg_store4(rgb + o * 3, n, c);
    }
}

// 64 groups of four pixels per workgroup along x, FG_ROWS rows along y and FG_WALK strides of the grid's rows per lane: at most 2048
// workgroups along y (the rest by more strides)
inline dim3 fg_grid(int H, int W)
{
    const int gx = ((W + 3) / 4 + 63) / 64, gy = (H + FG_ROWS * FG_WALK - 1) / (FG_ROWS * FG_WALK);
    return dim3(gx, gy < 2048 ? gy : 2048);
}

inline bool fg_args_ok(int H, int W, float intensity, float seed)
{
    return H >= 1 && W >= 1 && intensity > 0.f && intensity <= 0.1f && seed >= 0.f && seed < 1.f;      // NaN fails the comparisons
}

}  // namespace

// 0 < intensity <= 0.1, 0 <= seed < 1, H, W >= 1; hipErrorInvalidValue, nothing enqueued, otherwise
hipError_t film_grain_launch(const uint16_t *src, uint16_t *dst, int H, int W, float intensity, float seed, hipStream_t s)
{
    if (!src || !dst || !fg_args_ok(H, W, intensity, seed)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(film_grain_kernel, fg_grid(H, W), dim3(256), 0, s, src, dst, H, W, intensity, seed);
    return hipGetLastError();
}

// the same conditions; pq != 0 needs pq_bnd
hipError_t post_rgb48_grain_launch(const void *in, int is_f32, int H, int W, uint16_t *rgb, int pq, float peak, const float *pq_bnd,
                                   float intensity, float seed, hipStream_t s)
{
    if (!in || !rgb || !fg_args_ok(H, W, intensity, seed) || (pq && !pq_bnd)) return hipErrorInvalidValue;
    const dim3 g = fg_grid(H, W), b(256);
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((post_rgb48_grain_kernel<float, true>), g, b, 0, s, (const float *)in, rgb, H, W, peak, pq_bnd, intensity, seed);
        else hipLaunchKernelGGL((post_rgb48_grain_kernel<float, false>), g, b, 0, s, (const float *)in, rgb, H, W, peak, pq_bnd, intensity, seed);
    } else {
        if (pq) hipLaunchKernelGGL((post_rgb48_grain_kernel<f16, true>), g, b, 0, s, (const f16 *)in, rgb, H, W, peak, pq_bnd, intensity, seed);
        else hipLaunchKernelGGL((post_rgb48_grain_kernel<f16, false>), g, b, 0, s, (const f16 *)in, rgb, H, W, peak, pq_bnd, intensity, seed);
    }
    return hipGetLastError();
}
