// post_deband.hip -- debanding of RGB48 codes on the device (gfx950): hdrtv_rgb48_deband, u16 [H][W][3] -> u16 [H][W][3], never in
// place (include/hdrtv_mi355x.h states the integer rule; tests/cleanup_ref.py restates it).  A per-pixel gather: four reference
// pixels at (x +- dx, y +- dy), the offsets hashed from the pixel's position, at most DB_HALO = 16 pixels away in either axis.
//
// A workgroup of 512 lanes owns DB_TH x DB_TW = 32 x 128 pixels and stages them ONCE, with a halo of 16 pixels on every side, as
// interleaved u16 codes: tile[64][160 * 3], 960 bytes per row, 61440 bytes in all -- two workgroups (16 waves, four per SIMD) per
// CU in the 160 KiB.
//   1. stage   a job is one 16-byte chunk (eight u16) of a staged row, 60 per row, 7 or 8 per lane: one 16-byte global load and one
//              ds_write_b128 when the chunk lies inside the frame row and its address is 16-byte aligned, eight element loads
//              otherwise.  A lane issues all its wide loads before it stores the first of them: with two workgroups per CU there
//              is little else to hide a load behind, and one load per loop turn left the kernel waiting for each in turn.
//              The frame-edge clamp of the rule is applied HERE (row index clamped, and in the element path the pixel index),
//              so tile[ly][lx] = src[clamp(y0 - 16 + ly)][clamp(x0 - 16 + lx)] and step 2 never clamps or tests a bound.
//   2. gather  a job is eight neighbouring pixels of a row, one per lane: three ds_read_b128 for its own 48 bytes, then per pixel
//              the hash, and 4 x 3 ds_read_u16 for the references; the result leaves as three 16-byte stores when the group is whole
//              and its address aligned, element by element otherwise (ragged right edge, W not a multiple of 8, offset buffers).
// LDS banks (MI355X_MICROARCH.md): the gathers go to hashed positions, up to 33 x 33 apart inside a wave, so their bank is random
// whatever the row pitch is (two lanes that meet in one dword broadcast) and no padding would help them; the pitch is chosen for the
// other two accesses.  960 bytes keeps every chunk 16-byte aligned (ds_write_b128, ds_read_b128) and rows contiguous, so the
// staging stores of eight neighbouring lanes cover 128 contiguous bytes; the 16 lanes of a row in step 2 read 48-byte groups that
// start 12 dwords apart, i.e. in banks 0 12 24 36 48 60 8 20 .. 52 -- sixteen different multiples of four, so the four-dword reads of
// one row never meet in a bank.  Global traffic: 1.9 x the frame in (64 x 160 staged per 32 x 128 owned, the halo mostly from L2)
// and 1 x out.  No scratch (tests/test_isa_cleanup.py).
#include "launchers.h"
#include "../../include/hdrtv_mi355x.h"

namespace {

constexpr int DB_LH = DB_TH + 2 * DB_HALO;      // staged rows: 64
constexpr int DB_LW = DB_TW + 2 * DB_HALO;      // staged pixels per row: 160
constexpr int DB_RS = DB_LW * 3;                // u16 per staged row: 960 bytes
constexpr int DB_CH = DB_RS / 8;                // 16-byte chunks per staged row: 60
constexpr int DB_GW = DB_TW / 8;                // eight-pixel groups per tile row: 16
constexpr int DB_LANES = 512;                   // lanes per workgroup: one gather job each
constexpr int DB_JOBS = (DB_LH * DB_CH + DB_LANES - 1) / DB_LANES;      // staging chunks per lane: 8 (the last turn: half the lanes)
static_assert(DB_RS % 8 == 0 && DB_LH * DB_RS * 2 <= 65536 && DB_GW == 16, "chunks tile a row; the tile fits static LDS");
static_assert(DB_TH * DB_GW == DB_LANES, "one gather job per lane");

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(DB_LANES) void rgb48_deband_kernel(DebandParams p)
{
    __shared__ __attribute__((aligned(16))) uint16_t tile[DB_LH][DB_RS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DB_TW, y0 = blockIdx.y * DB_TH;
    const long long rowlen = 3ll * p.W;                      // u16 per frame row

    // 1. stage: chunk k of staged row lr = u16 elements t .. t + 7 of the frame row, counted from pixel x0 - 16.  Three passes over
    // the lane's DB_JOBS chunks, so that all its 16-byte loads are in flight together: wide loads, element loads, LDS stores.
    uint4 v[DB_JOBS];
    const long long e0 = 3ll * (x0 - DB_HALO);               // may lie left of the row (< 0); a chunk may run past the row's end
#pragma unroll
    for (int it = 0; it < DB_JOBS; ++it) {
        const int job = tid + DB_LANES * it, lr = job / DB_CH, k = job - lr * DB_CH;
        const uint16_t *row = p.src + (size_t)min(max(y0 - DB_HALO + lr, 0), p.H - 1) * rowlen;
        const long long e = e0 + 8 * k;
        if (job < DB_LH * DB_CH && e >= 0 && e + 8 <= rowlen && aligned16(row + e)) v[it] = *reinterpret_cast<const uint4 *>(row + e);
    }
#pragma unroll
    for (int it = 0; it < DB_JOBS; ++it) {
        const int job = tid + DB_LANES * it, lr = job / DB_CH, k = job - lr * DB_CH;
        const uint16_t *row = p.src + (size_t)min(max(y0 - DB_HALO + lr, 0), p.H - 1) * rowlen;
        const long long e = e0 + 8 * k;
        if (job < DB_LH * DB_CH && !(e >= 0 && e + 8 <= rowlen && aligned16(row + e))) {
            uint32_t q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int t = 8 * k + i, lx = t / 3, ch = t - 3 * lx;                     // staged pixel and channel
                const int x = min(max(x0 - DB_HALO + lx, 0), p.W - 1);
                q[i] = row[(size_t)x * 3 + ch];
            }
            v[it] = make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
        }
    }
#pragma unroll
    for (int it = 0; it < DB_JOBS; ++it) {
        const int job = tid + DB_LANES * it, lr = job / DB_CH, k = job - lr * DB_CH;
        if (job < DB_LH * DB_CH) *reinterpret_cast<uint4 *>(&tile[lr][8 * k]) = v[it];
    }
    __syncthreads();

    // 2. gather: job = eight pixels (job & 15) of tile row (job >> 4)
    const uint32_t span = 2u * (uint32_t)p.range + 1u;
    const int T = p.threshold;
    {
        const int r = tid >> 4, g = tid & 15, x = x0 + 8 * g, y = y0 + r;
        if (y >= p.H || x >= p.W) return;
        const int n = min(8, p.W - x), ly = r + DB_HALO, lx0 = DB_HALO + 8 * g;
        const uint4 *own = reinterpret_cast<const uint4 *>(&tile[ly][lx0 * 3]);
        const uint4 a = own[0], b = own[1], c = own[2];
        const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t h0 = p.seed * 0x9E3779B9u + (uint32_t)y * (uint32_t)p.W + (uint32_t)x;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t h = h0 + (uint32_t)i;
            h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
            const int dx = (int)(((h & 0xffffu) * span) >> 16) - p.range, dy = (int)(((h >> 16) * span) >> 16) - p.range;
            const uint16_t *ra = &tile[ly + dy][0], *rb = &tile[ly - dy][0];
            const int ca = (lx0 + i + dx) * 3, cb = (lx0 + i - dx) * 3;
            bool flat = true;
            int s[3], m[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int e = 3 * i + ch;
                s[ch] = (int)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));
                const int r0 = ra[ca + ch], r1 = ra[cb + ch], r2 = rb[cb + ch], r3 = rb[ca + ch];
                // |r_k - s| < T for all four <=> the largest and the smallest reference are both within T of s
                const int hi = max(max(r0, r1), max(r2, r3)), lo = min(min(r0, r1), min(r2, r3));
                flat = flat & (hi - s[ch] < T) & (s[ch] - lo < T);
                m[ch] = (r0 + r1 + r2 + r3 + 2) >> 2;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int e = 3 * i + ch;
                o[e >> 1] |= (uint32_t)(flat ? m[ch] : s[ch]) << (16 * (e & 1));
            }
        }
        uint16_t *d = p.dst + ((size_t)y * p.W + x) * 3;
        if (n == 8 && aligned16(d)) {
            uint4 *d4 = reinterpret_cast<uint4 *>(d);
            d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
            d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
        } else {
#pragma unroll
            for (int e = 0; e < 24; ++e)
                if (e < 3 * n) d[e] = (uint16_t)((e & 1) ? (o[e >> 1] >> 16) : (o[e >> 1] & 0xffffu));
        }
    }
}

}  // namespace

// The bounds every access rests on: range <= DB_HALO keeps the references inside the staged tile, H, W >= 1 the clamps meaningful.
hipError_t rgb48_deband_launch(const DebandParams &p, hipStream_t s)
{
    if (!p.src || !p.dst || p.src == p.dst || p.H < 1 || p.W < 1 || p.range < 1 || p.range > DB_HALO || p.threshold < 1 ||
        p.threshold > 65535)
        return hipErrorInvalidValue;
    const dim3 g((p.W - 1) / DB_TW + 1, (p.H - 1) / DB_TH + 1);
    hipLaunchKernelGGL(rgb48_deband_kernel, g, dim3(DB_LANES), 0, s, p);
    return hipGetLastError();
}
