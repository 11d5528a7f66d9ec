// conv3x3_pglds.hip -- persistent version of the HG head's 3x3 convolutions (Cin multiple of 64,
// Cout multiple of 128, stride 1; Hallucination_arch.py:97-137 conv2..conv_code2, Up_conv1..5).
//
// Same GEMM view, LDS images and LDS-DMA pipeline as conv3x3_glds.hip (128 output channels x
// 16x16-pixel tile, K = 64-channel chunk x tap, halo tile staged once per chunk, weights in a 3-slot
// ring two taps ahead, one raw s_barrier per tap behind a counted s_waitcnt vmcnt), but one block
// per CU walks a run of tiles and the (tile, chunk, tap) iterations form ONE stream:
//   * the next tile's first halo chunk, its first weight taps and its 128 scale/shift pairs are
//     DMA'd during the current tile's last taps, so a tile costs no prologue latency and no block
//     launch (the K = 9 layers conv2 / Up_conv5 spent ~40 % of their time there);
//   * the epilogue runs out of the accumulator registers: scale/shift from LDS, pooling / pixel
//     shuffle / the fused 64->3 dot products in registers, then a transposition through a
//     wave-private strip of the halo buffer the tile has just released (LDS operations of one wave
//     execute in order: no barrier) so that global stores are 16 bytes per lane and 8 lanes cover a
//     pixel's 128-byte channel run; the other tile buffers stay free for the DMAs already in
//     flight.  Every wave issues the SAME number of stores per tile
//     (out-of-image lanes write a trash line instead of being masked): vmcnt counts loads, stores
//     and LDS-DMA together in issue order, so the counted wait after a tile boundary depends on it.
// MFMA shape 16x16x32 (lane = row & 15, k-group = lane >> 4): under load the chip holds a higher
// clock on it than on 32x32x16 (MI355X_MICROARCH.md, DVFS give-back item 7; measured here +4 %).
//
// Sparse launches (ConvParams::tile_list, the HG need lists of hg_need.hip; tile_run.h): the spatial tiles are the list's
// entries instead of all tiles_x * tiles_y.  The count is read once; every block copies the entries of ITS run into LDS in
// the prologue (in front of the prologue's barrier), so the tile loop's only new operation is one LDS read per tile.
#include "launchers.h"

namespace {

constexpr int TH = 16, TW = 16, HW = 18, NPIX = HW * HW;
constexpr int CT = 64, PIXB = CT * 2;                    // 64-channel chunk = 128 B per pixel
constexpr int BN = 128;
constexpr int A_PIECES_PER_WAVE = 6, A_BYTES = 8 * A_PIECES_PER_WAVE * 1024;   // 324 halo px -> 48 KiB
constexpr int B_BYTES = BN * PIXB, B_PIECES_PER_WAVE = 2;                       // 16 KiB
constexpr int SS_OFF = 2 * A_BYTES + 3 * B_BYTES;        // two 1-KiB {scale[128], shift[128]} slots
constexpr int DOTW_OFF = SS_OFF + 2048;                  // ST_PS_DOT3: 24 fragment pairs (hi, lo) of 32 B
constexpr int LIST_OFF = DOTW_OFF + 1024;                // ConvParams::tile_list: this block's run of spatial tiles (tile_run.h)
constexpr int SMEM = LIST_OFF + TILE_LIST_N * 4;         // 149 KiB

// stores per wave and tile, by store mode (see the epilogues)
template <int MODE> struct NStores { static constexpr int N = MODE == ST_POOL ? 2 : (MODE == ST_PS_DOT3 ? 1 : 8); };

// LDS-DMA (dma_rsrc, dma16, DMA_OOB), the counted wait_vm<N> and the tap's closing wait_tap<N>: common.h

struct Tile { int n0, oy0, ox0; };

template <int MODE>
__global__ __launch_bounds__(512) void conv_pglds_kernel(ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *sA = smem;
    char *sB = smem + 2 * A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kg = lane >> 4;

    // ---- this block's run of tiles (tile_run.h) ----------------------------------------------------------------
    const int ntn = p.CoutPad / BN;
    const int *const lst = p.tile_list;                      // null: every tile (dense)
    const int nsp = lst ? lst[0] : p.tiles_x * p.tiles_y;    // spatial tiles to compute
    const int total = nsp * ntn;
    const TileRun run = tile_run(total, gridDim.x, blockIdx.x);
    const int t_first = run.t_first, t_step = run.t_step, ntile = run.ntile;
    if (ntile == 0) return;
    // the list entries of this block's run (the launcher passes a list only when a run fits); visible behind the prologue's barrier
    const tile_list_lds_t s_list = (tile_list_lds_t)(smem + LIST_OFF);
    int sp_first = 0;                                        // the run's first entry: loaded beside the others, one trip to memory
    if (lst) {
        sp_first = lst[1 + (p.nt_slow ? t_first % nsp : t_first / ntn)];
        tile_list_stage(s_list, lst, run, tid, [&](int t) { return p.nt_slow ? t % nsp : t / ntn; });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // tile number k of the run (k = 0: the prologue, in front of the barrier, has the entry from the list itself)
    auto decode = [&](int k) {
        Tile o;
        const int t = t_first + k * t_step;
        const int nt_i = p.nt_slow ? t / nsp : t % ntn;
        int sp = p.nt_slow ? t - nt_i * nsp : t / ntn;
        if (lst) sp = k ? tile_list_at(s_list, k) : sp_first;
        const int ty = sp / p.tiles_x, tx = sp - ty * p.tiles_x;
        o.n0 = nt_i * BN; o.oy0 = ty * TH; o.ox0 = tx * TW;
        return o;
    };

    const int nchunk = (p.c0 + p.c1) / CT, nchunk0 = p.c0 / CT;
    const int nit = nchunk * 9;

    // ---- LDS-DMA issue helpers (wave-uniform LDS base, per-lane swizzled source) ------------
    const int l_row = lane >> 3, l_slot = lane & 7;
    auto issue_A = [&](int cc, int buf, const Tile &T) {
        const f16 *src;
        int cs, coff;
        if (cc < nchunk0) { src = p.src0; cs = p.s0_stride; coff = cc * CT; }
        else { src = p.src1; cs = p.s1_stride; coff = (cc - nchunk0) * CT; }
        const dma_rsrc_t rs = dma_rsrc(src, (unsigned)p.Hi * (unsigned)p.Wi * (unsigned)cs * 2u);
#pragma unroll
        for (int it = 0; it < A_PIECES_PER_WAVE; ++it) {
            const int piece = wave + it * 8;
            const int hp = piece * 8 + l_row;
            const int hy = hp / HW, hx = hp - hy * HW;
            const int iy = T.oy0 - 1 + hy, ix = T.ox0 - 1 + hx;
            const bool ok = (hp < NPIX) & ((unsigned)iy < (unsigned)p.Hi) & ((unsigned)ix < (unsigned)p.Wi);
            const unsigned off = ((unsigned)(iy * p.Wi + ix) * (unsigned)cs + (unsigned)(coff + ((l_slot ^ (hx & 7)) << 3))) * 2u;
            dma16(rs, sA + buf * A_BYTES + piece * 1024, ok ? off : DMA_OOB, 0);
        }
    };
    auto issue_B = [&](int it_i, int n0, int slot) {
        const int cc = it_i / 9, tap = it_i - cc * 9;
        const dma_rsrc_t rs = dma_rsrc(p.wpk, 9u * (unsigned)nchunk * (unsigned)p.CoutPad * (unsigned)PIXB);
        const unsigned so = (unsigned)((tap * nchunk + cc) * p.CoutPad + n0) * (unsigned)PIXB;
#pragma unroll
        for (int k = 0; k < B_PIECES_PER_WAVE; ++k) {
            const int piece = wave * B_PIECES_PER_WAVE + k;
            const int n = piece * 8 + l_row;
            dma16(rs, sB + slot * B_BYTES + piece * 1024, (unsigned)(n * CT + ((l_slot ^ (n & 7)) << 3)) * 2u, so);
        }
    };
    auto issue_SS = [&](int n0, int slot) {      // every wave writes the same 1 KiB: {scale[128], shift[128]}
        const char *sc = reinterpret_cast<const char *>(p.scale), *sh = reinterpret_cast<const char *>(p.shift);
        const char *lo = sc < sh ? sc : sh;                      // one (wave-uniform) resource over both arrays
        const dma_rsrc_t rs = dma_rsrc(lo, 0xffffffffu);
        dma16(rs, smem + SS_OFF + slot * 1024, (unsigned)((lane < 32 ? sc : sh) - lo) + (unsigned)(lane & 31) * 16u, (unsigned)n0 * 4u);
    };

    if constexpr (MODE == ST_PS_DOT3) {          // before any DMA is in flight (ordinary loads drain the queue)
        // The 64 -> 3 dot products run as conv_prw<ps_dot3> runs them (conv3x3_prw.hip: same table, same MFMA chain, same sums), so
        // that Up_conv5's partial sums do not depend on which of the two kernels a layer is routed to (variant prw).  Table entry
        // ((half * 3 + o) * 4 + kg): the A-operand fragment of output o over the channels 32 half .. 32 half + 31 for the lanes
        // of k-group kg, an fp32 weight as hi + lo * 2^-10 in two f16 values.
        if (tid < 24) {
            const int kgq = tid & 3, o = (tid >> 2) % 3, half = tid / 12;
            f16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float w = p.dotw[o * 64 + half * 32 + (e < 4 ? 4 * kgq + e : 16 + 4 * kgq + e - 4)];
                hi[e] = (f16)w;
                lo[e] = (f16)((w - (float)hi[e]) * 1024.f);
            }
            *reinterpret_cast<f16x8 *>(smem + DOTW_OFF + tid * 32) = hi;
            *reinterpret_cast<f16x8 *>(smem + DOTW_OFF + tid * 32 + 16) = lo;
        }
        __syncthreads();
    }

    // ---- wave tiling: 2 (channels) x 4 (pixel rows) waves, each 64 ch x 64 px = 4x4 tiles of 16x16
    const int wc = wave & 1, wp = wave >> 1;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ReLU or none (the launcher refuses anything else): one v_max against 0 or -inf instead of max(v, slope * v)
    // (A/B on one box, four builds: 6.89 -> 6.82 ms over the 14 launches)
    const float act_lb = p.act == ACT_RELU ? 0.f : -__builtin_inff();
    const int kw = l15 & 7;
    const int b_lane = (wc * 64 + l15) * PIXB;
    const int a_lane = (wp * 4 * HW + l15) * PIXB;

    // ---- prologue: first tile's halo, scale/shift and weights of taps 0 and 1 -----------------
    Tile cur = decode(0), nxt = cur;
    issue_A(0, 0, cur);
    issue_SS(cur.n0, 0);
    issue_B(0, cur.n0, 0);
    issue_B(1, cur.n0, 1);
    issue_B(2, cur.n0, 2);
    wait_vm<4>();
    __builtin_amdgcn_s_barrier();

    int gch = 0;                                  // chunks done so far: halo buffer parity
    for (int k = 0; k < ntile; ++k) {
        const bool has_next = k + 1 < ntile;
        if (has_next) nxt = decode(k + 1);
        for (int cc = 0; cc < nchunk; ++cc, ++gch) {
            const char *a = sA + (gch & 1) * A_BYTES;
            const bool last_chunk = cc + 1 == nchunk;
            const bool pfA = !last_chunk || has_next;    // a halo tile is staged during this chunk's tap 6
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int it_i = cc * 9 + tap;
                // stream index = 9 * gch + tap, so the ring slot of this iteration is tap % 3
                // (a tile's weights(2) are issued before the tile starts: prologue / end of the previous tile)
                bool pfB = true;
                if (tap == 0 && cc == 0) {}
                else if (it_i + 2 < nit) issue_B(it_i + 2, cur.n0, (tap + 2) % 3);
                else if (has_next) issue_B(it_i + 2 - nit, nxt.n0, (tap + 2) % 3);
                else pfB = false;
                if (tap == 6 && pfA) {
                    if (!last_chunk) issue_A(cc + 1, (gch + 1) & 1, cur);
                    else { issue_A(0, (gch + 1) & 1, nxt); issue_SS(nxt.n0, (k + 1) & 1); }
                }

                const char *bw = sB + (tap % 3) * B_BYTES + b_lane;
                const char *ax = a + a_lane + ((tap / 3) * HW + tap % 3) * PIXB;
                const int kx = (l15 + tap % 3) & 7;
                f16x8 wf[2][4], xf[2][4];
                auto ldw = [&](int ks, int i) {
                    wf[ks][i] = *reinterpret_cast<const f16x8 *>(bw + i * 16 * PIXB + (((ks * 4 + kg) ^ kw) << 4));
                };
                auto ldx = [&](int ks, int j) {
                    xf[ks][j] = *reinterpret_cast<const f16x8 *>(ax + j * HW * PIXB + (((ks * 4 + kg) ^ kx) << 4));
                };
                // program order IS the schedule of the LDS reads: sched_barrier(0) lets nothing cross, and the last one stands behind
                // the last read.  The k-step-1 MFMAs behind it are left to hipcc, which sinks them below the tap's barrier and into
                // the next tap's DMA issue (pinning them here cost 2 % of the kernel, NOTEBOOK.md); the waits for their operands
                // must not sink with them: wait_tap
#pragma unroll
                for (int i = 0; i < 4; ++i) { ldw(0, i); ldx(0, i); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    acc[g >> 2][g & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[0][g >> 2], xf[0][g & 3], acc[g >> 2][g & 3], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // k-step 1 fragments in the order its MFMAs want them: w0 x0 x1 x2 x3 w1 w2 w3
                    if (g == 0) ldw(1, 0); else if (g < 5) ldx(1, g - 1); else ldw(1, g - 4);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int m = 8; m < 16; ++m)
                    acc[m >> 2][m & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[0][m >> 2], xf[0][m & 3], acc[m >> 2][m & 3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 16; ++m)
                    acc[m >> 2][m & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[1][m >> 2], xf[1][m & 3], acc[m >> 2][m & 3], 0, 0, 0);

                // The next iteration reads weights(s+1), issued one iteration ago, and at a chunk boundary
                // the halo staged at tap 6.  Allow exactly the DMAs (and, right after a tile boundary, the
                // previous tile's stores) that are younger than those.
                if (!pfB) {
                    wait_tap<0>();
                } else if ((tap == 6 || tap == 7) && pfA) {
                    if (last_chunk) wait_tap<9>();        // halo (6) + scale/shift (1) + weights(s+2) (2)
                    else wait_tap<8>();
                } else if (tap <= 1 && cc == 0 && k > 0) {
                    wait_tap<NStores<MODE>::N + 2>();     // weights(s+1) are older than the last tile's stores
                } else {
                    wait_tap<2>();
                }
                __builtin_amdgcn_s_barrier();
            }
        }

        // weights(2) of the next tile go out BEFORE this tile's stores: vmcnt retires in issue order, so the
        // first DMA wait that has to see the stores complete is then three taps away instead of one
        if (has_next) issue_B(2, nxt.n0, 2);
        // ------------------------------------------------------------ epilogue, from registers
        // lane: pixel (row wp*4 + j, column l15), channels wc*64 + i*16 + 4*kg + {0..3}
        const float *ss = reinterpret_cast<const float *>(smem + SS_OFF + (k & 1) * 1024);
        char *trash = reinterpret_cast<char *>(p.trash) + lane * 16;
        const int cw = wc * 64 + 4 * kg;
        f16x4 o[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 sc = *reinterpret_cast<const float4 *>(ss + cw + i * 16);
            const float4 sh = *reinterpret_cast<const float4 *>(ss + 128 + cw + i * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[i][j][0] = (f16)fmaxf(acc[i][j][0] * sc.x + sh.x, act_lb);
                o[i][j][1] = (f16)fmaxf(acc[i][j][1] * sc.y + sh.y, act_lb);
                o[i][j][2] = (f16)fmaxf(acc[i][j][2] * sc.z + sh.z, act_lb);
                o[i][j][3] = (f16)fmaxf(acc[i][j][3] * sc.w + sh.w, act_lb);
                acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const int ox = cur.ox0 + l15;   // (ST_PS_DOT3)
        // NHWC / PS / POOL: transpose through a wave-private strip of the halo buffer this tile just finished
        // with (free until the next tile's tap 6), so that global stores are 16 bytes per lane and 8 lanes
        // cover a pixel's 128-byte channel run (8-byte quads straight from the accumulator layout cost ~25 %
        // of a K = 9 layer).  LDS operations of one wave execute in order: no barrier.
        constexpr int SP = 144;                                  // strip row pitch: 64 ch x 2 B + 16
        char *stg = sA + ((gch - 1) & 1) * A_BYTES + wave * (32 * SP);
        const int s_row = lane >> 3, s_chunk = lane & 7;
        if constexpr (MODE == ST_NHWC || MODE == ST_PS) {
            const int cps = p.dstC;
            const int chw = cur.n0 + wc * 64;
            const int sub = MODE == ST_PS ? chw / cps : 0;
            const int cbase = (MODE == ST_PS ? chw - sub * cps : chw) + s_chunk * 8;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        *reinterpret_cast<f16x4 *>(stg + (jj * 16 + l15) * SP + (i * 16 + 4 * kg) * 2) = o[i][2 * pass + jj];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const f16x8 v = *reinterpret_cast<const f16x8 *>(stg + (rr * 8 + s_row) * SP + s_chunk * 16);
                    const int oy = cur.oy0 + wp * 4 + 2 * pass + (rr >> 1);
                    const int oxx = cur.ox0 + (rr & 1) * 8 + s_row;
                    f16 *d;
                    if constexpr (MODE == ST_NHWC) {
                        const bool ok = oy < p.Ho && oxx < p.Wo;
                        d = ok ? p.dst + ((size_t)oy * p.Wo + oxx) * p.dstC + cbase : reinterpret_cast<f16 *>(trash);
                    } else {
                        // channels were permuted at pack time: ch = sub * dstC + c; the wave's 64 channels share one sub
                        const int Y = 2 * oy + (sub >> 1), X = 2 * oxx + (sub & 1);
                        const bool ok = oy < p.Ho && oxx < p.Wo && Y < p.Hd && X < p.Wd;
                        d = ok ? p.dst + ((size_t)Y * p.Wd + X) * cps + cbase : reinterpret_cast<f16 *>(trash);
                    }
                    *reinterpret_cast<f16x8 *>(d) = v;
                }
            }
        } else if constexpr (MODE == ST_POOL) {
            // 2x2 max: rows j, j+1 are in this lane; columns 2c, 2c+1 meet in the strip
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f16x4 m;
#pragma unroll
                    for (int r = 0; r < 4; ++r) m[r] = o[i][2 * jj][r] > o[i][2 * jj + 1][r] ? o[i][2 * jj][r] : o[i][2 * jj + 1][r];
                    *reinterpret_cast<f16x4 *>(stg + (jj * 16 + l15) * SP + (i * 16 + 4 * kg) * 2) = m;
                }
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                f16x8 v = *reinterpret_cast<const f16x8 *>(stg + (jj * 16 + 2 * s_row) * SP + s_chunk * 16);
                const f16x8 v1 = *reinterpret_cast<const f16x8 *>(stg + (jj * 16 + 2 * s_row + 1) * SP + s_chunk * 16);
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = v[r] > v1[r] ? v[r] : v1[r];
                const int py = (cur.oy0 >> 1) + wp * 2 + jj, px = (cur.ox0 >> 1) + s_row;
                const bool ok = py < p.Hd && px < p.Wd;
                f16 *d = ok ? p.dst + ((size_t)py * p.Wd + px) * p.dstC + cur.n0 + wc * 64 + s_chunk * 8 : reinterpret_cast<f16 *>(trash);
                *reinterpret_cast<f16x8 *>(d) = v;
            }
        } else {   // ST_PS_DOT3: pixel shuffle, then 64 -> 3 dot products; only 3 partial sums per pixel leave the CU
            // On the matrix pipe, per 32-channel half of the wave's 64 channels (= one wave of conv_prw): the f16 results of a
            // pixel row are the B operand, output rows 4 q + o carry output o of pixel row q, so after the four rows lane (kg, l15)
            // holds the three sums of pixel (kg, l15) in registers 0..2.  Half 0 + half 1 is the sum conv_prw's wave pair forms.
            const int orow = l15 & 3, qrow = l15 >> 2;
            const f16x8 zero8 = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const char *tb = smem + DOTW_OFF + (((half * 3 + (orow < 3 ? orow : 0)) * 4 + kg) << 5);
                f16x8 fh = *reinterpret_cast<const f16x8 *>(tb), fl = *reinterpret_cast<const f16x8 *>(tb + 16);
                if (orow == 3) { fh = zero8; fl = zero8; }
                f32x4 ah = {0.f, 0.f, 0.f, 0.f}, al = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const f16x4 o0 = o[2 * half][jj], o1 = o[2 * half + 1][jj];
                    const f16x8 bq = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
                    const bool mine = qrow == jj;
                    ah = __builtin_amdgcn_mfma_f32_16x16x32_f16(mine ? fh : zero8, bq, ah, 0, 0, 0);
                    al = __builtin_amdgcn_mfma_f32_16x16x32_f16(mine ? fl : zero8, bq, al, 0, 0, 0);
                }
                constexpr float k = 1.f / 1024.f;
                const float4 v = make_float4(ah[0] + al[0] * k, ah[1] + al[1] * k, ah[2] + al[2] * k, 0.f);
                if (half == 0) r = v;
                else { r.x += v.x; r.y += v.y; r.z += v.z; }
            }
            const int sub = cur.n0 / 64 + wc;
            const int oy = cur.oy0 + wp * 4 + kg;
            const int Y = 2 * oy + (sub >> 1), X = 2 * ox + (sub & 1);
            const bool ok = oy < p.Ho && ox < p.Wo && Y < p.Hd && X < p.Wd;
            float4 *d = ok ? reinterpret_cast<float4 *>(p.dst_dot + ((size_t)Y * p.Wd + X) * 4) : reinterpret_cast<float4 *>(trash);
            *d = make_float4(r.x, r.y, r.z, 0.f);
        }
        cur = nxt;
    }
}

template <int MODE>
hipError_t launch_mode(const ConvParams &p, int grid, hipStream_t stream)
{
    static DevOnce attr_once;
    auto kern = conv_pglds_kernel<MODE>;
    if (hipError_t e = allow_lds(attr_once, kern, SMEM)) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), SMEM, stream, p);
    return hipGetLastError();
}

}  // namespace

// 3x3, stride 1, pad 1, Cin (src0 [+ src1 concat]) multiple of 64, Cout == CoutPad multiple of 128, no residuals;
// store modes NHWC / PS / POOL / PS_DOT3.  One block per CU (n_cu), each walking tiles.  hipErrorInvalidValue otherwise.
// p.tile_list (16x16 tiles) is walked when a block's run fits the kernel's LDS block; *list_taken says whether it was.
hipError_t conv_pglds_launch(ConvParams p, int n_cu, hipStream_t stream, bool *list_taken)
{
    if (list_taken) *list_taken = false;
    if ((p.c0 % CT) || (p.c1 % CT) || p.c0 + p.c1 < CT || (p.CoutPad % BN) || p.Cout != p.CoutPad || p.res1 || p.res2 ||
        p.dst_full || !p.zeros || !p.trash || n_cu < 8 || (p.act != ACT_RELU && p.act != ACT_NONE) ||
        (p.mode != ST_NHWC && p.mode != ST_PS && p.mode != ST_POOL && p.mode != ST_PS_DOT3) ||
        (p.mode == ST_PS && (p.dstC % 64)) || (p.mode == ST_PS_DOT3 && (p.dstC != 64 || !p.dotw || !p.dst_dot)))
        return hipErrorInvalidValue;
    p.tiles_x = (p.Wo + TW - 1) / TW;
    p.tiles_y = (p.Ho + TH - 1) / TH;
    const int total = p.tiles_x * p.tiles_y * (p.CoutPad / BN);
    const int grid = total < n_cu ? total : n_cu;
    // the grid never depends on the list's count (device memory); a run too long for the LDS block: dense (a grid below eight keeps its list)
    if (!tile_list_fits(total, grid, 1)) p.tile_list = nullptr;
    if (list_taken) *list_taken = p.tile_list != nullptr;
    switch (p.mode) {
    case ST_NHWC: return launch_mode<ST_NHWC>(p, grid, stream);
    case ST_PS: return launch_mode<ST_PS>(p, grid, stream);
    case ST_POOL: return launch_mode<ST_POOL>(p, grid, stream);
    default: return launch_mode<ST_PS_DOT3>(p, grid, stream);
    }
}
