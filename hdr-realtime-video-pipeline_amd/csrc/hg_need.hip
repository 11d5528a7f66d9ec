// hg_need.hip -- which tiles of the Hallucination Generator can reach the output ("need lists").
//
// The head ends in out = mask * hg(img) + img with a 0/1 mask, cropped to H x W: an activation pixel matters only if a masked
// output pixel depends on it.  hg_prep leaves one flag per 16x16 full-resolution cell that holds a masked pixel inside H x W; this
// kernel carries that set backwards through the layer table (consumer -> producer) and leaves, per layer, the compacted list of
// kernel tiles to compute.  Everything stays in device memory: the launches behind it read the counts themselves, so the frame
// needs no host round trip and is capturable as a graph.
//
// Need is kept per tensor in units of u x u pixels of the tensor's level, u = 1 << HgNeedParams::lu[level] (launchers.h:
// hg_need_unit_log2; 16 at every level under hg_sparse = 1, 16 / 4 / 2 / 1 / 1 / 1 at levels 0 .. 5 under hg_sparse = 2).  A map is
// a set of bit rows, 64 units per 64-bit word; bits beyond a row's width are always 0.
//
// Rules (conservative: any superset of the per-pixel dependency set gives the same output), K = the units a layer must get right,
// every result rounded up to whole units of the map it lands in:
//   K(layer)          = need(out tensor) for a layer that writes at its own level,
//                       the 2x2 up-sampling of it for a pool-fused layer (a pooled pixel is made of its 2x2 pre-pool pixels),
//                       the any-of-2x2 down-sampling for a pixel-shuffle layer (a pixel at level l+1 writes 2x2 pixels at level l);
//                       between two maps whose units differ, a K unit is needed if an out unit it touches is;
//   need(in [, skip]) |= K dilated by one unit for a 3x3 layer (its halo is one pixel: one unit or less), K itself for a 1x1 layer.
// A tensor with two readers collects both (the layers run in reverse launch order, so every reader is seen before the producer).
// A layer's list holds the kernel tiles (16 x 16, 8 rows x 16 for conv_prw8, 8 rows x 32 for conv1 on conv_c3) with at least one
// unit of K, in ascending order.
//
// Why a computed tile may hold wrong pixels.  A listed tile is computed whole, but only its K units had their inputs computed:
// its other pixels are made from skipped or stale inputs -- another frame's values, after an overflow even non-finite ones.  They
// are never read by a pixel that matters, because the need set is closed: K(producer) holds every unit a K pixel of any reader
// reads (the rules above, applied to every reader), so by induction from the output a needed pixel is computed from needed pixels
// only.  The conv kernels have no cross-pixel term inside a tile besides the 3x3 window itself: the max-pool epilogue combines the
// 2x2 pre-pool pixels of one pooled pixel (the up-sampling rule makes all four K), the PixelShuffle epilogue moves channels of one
// pixel to its 2x2 output pixels, Up_conv5's fused dot products sum over the channels of one output pixel.  At the end the blend
// selects img at a mask-0 pixel and does not multiply, so what the head left there, finite or not, does not show.
//
// One workgroup; the loops run over rows and words, so no frame size is too large.  A lone workgroup waits about a microsecond for
// every dependent access to device memory, so what one layer hands to the next stays in LDS when it fits (a 3840x2160 frame: 272
// rows x 8 words per map): the layer's K, its tile bits, and the need map of its input, which is the output of the layer seen next.
// Device memory holds the lists, the skip tensors' maps (read many layers later) and every map that does not fit.
#include "launchers.h"

namespace {

constexpr int NT = 1024, LDS_WORDS = 2304;
using u64 = unsigned long long;

// the lowest bit of every field of 1, 2, 4, 8, 16 bits
__constant__ u64 k_tile_bits[5] = {~0ull, 0x5555555555555555ull, 0x1111111111111111ull, 0x0101010101010101ull, 0x0001000100010001ull};

struct Map {
    int h, w, nw;              // rows, units per row, words per row
};
__device__ __forceinline__ Map map_of(const HgNeedParams &p, int level)
{
    const int lu = p.lu[level], r = (1 << lu) - 1;
    Map m;
    m.h = ((p.Hp >> level) + r) >> lu;
    m.w = ((p.Wp >> level) + r) >> lu;
    m.nw = (m.w + 63) >> 6;
    return m;
}
// word wi of row y, 0 outside the map
__device__ __forceinline__ u64 word(const u64 *b, const Map &m, int y, int wi)
{
    return (unsigned)y < (unsigned)m.h && (unsigned)wi < (unsigned)m.nw ? b[y * m.nw + wi] : 0;
}
// the bits of word wi that lie inside a row of w units
__device__ __forceinline__ u64 row_mask(int w, int wi)
{
    const int n = w - 64 * wi;
    return n >= 64 ? ~0ull : (n <= 0 ? 0ull : (1ull << n) - 1);
}
// every bit of v twice: bit i -> bits 2 i, 2 i + 1
__device__ __forceinline__ u64 spread2(unsigned v)
{
    u64 x = v;
    x = (x | x << 16) & 0x0000FFFF0000FFFFull;
    x = (x | x << 8) & 0x00FF00FF00FF00FFull;
    x = (x | x << 4) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x << 2) & 0x3333333333333333ull;
    x = (x | x << 1) & 0x5555555555555555ull;
    return x | x << 1;
}
// any of every pair of bits: bits 2 i, 2 i + 1 -> bit i
__device__ __forceinline__ unsigned pairs_any(u64 v)
{
    u64 x = (v | v >> 1) & 0x5555555555555555ull;
    x = (x | x >> 1) & 0x3333333333333333ull;
    x = (x | x >> 2) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x >> 4) & 0x00FF00FF00FF00FFull;
    x = (x | x >> 8) & 0x0000FFFF0000FFFFull;
    x = (x | x >> 16) & 0x00000000FFFFFFFFull;
    return (unsigned)x;
}

__global__ __launch_bounds__(NT) void hg_need_kernel(HgNeedParams p)
{
    __shared__ u64 s_k[LDS_WORDS], s_t[LDS_WORDS], s_n[LDS_WORDS];
    __shared__ int s_wave[NT / 64];
    const int tid = threadIdx.x;
    // hg_prep's flags become the level-0 map and are consumed: hg_prep only ever sets them.  A wave turns 64 flags into a word with
    // one ballot; eight words per pass, so that a pass waits for device memory once
    {
        const Map m = map_of(p, 0);
        const HgNeedLayer &L = p.L[p.n_layers - 1];
        u64 *fb = L.out_chained && m.h * m.nw <= LDS_WORDS ? s_n : reinterpret_cast<u64 *>(p.base + p.map_off[p.flags_map]);
        unsigned char *fl = p.base + p.flags_off;
        constexpr int NW = NT / 64, B = 8;
        const int lane = tid & 63, n0 = m.h * m.nw;
        for (int i0 = tid >> 6; i0 < n0; i0 += B * NW) {
            int at[B];
            unsigned char c[B];
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int i = i0 + j * NW, y = i / m.nw, x = 64 * (i - y * m.nw) + lane;
                at[j] = i < n0 && x < m.w ? y * m.w + x : -1;
                c[j] = at[j] >= 0 ? fl[at[j]] : 0;
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const u64 v = __ballot(c[j] != 0);
                if (at[j] >= 0) fl[at[j]] = 0;
                if (lane == 0 && i0 + j * NW < n0) fb[i0 + j * NW] = v;
            }
        }
    }
    __syncthreads();
    for (int li = p.n_layers - 1; li >= 0; --li) {
        const HgNeedLayer L = p.L[li];
        const int olev = L.level + (L.mode == 1 ? 1 : 0) - (L.mode == 2 ? 1 : 0);
        const Map mk = map_of(p, L.level), mo = map_of(p, olev);
        const int lu = p.lu[L.level], nk = mk.h * mk.nw;
        // a K unit x lies in the out unit x >> sh (sh = 1), is it (0), or holds the out units 2 x and 2 x + 1 (-1)
        const int sh = p.lu[olev] - lu + olev - L.level;
        // the tiles: th rows x tw pixels = rows [r0, r0 + nr) x bw bits of the map
        const int lth = L.th == 8 ? 3 : 4, ltw = L.tw == 32 ? 5 : 4, lbw = ltw - lu;
        const int ty_n = ((p.Hp >> L.level) + L.th - 1) >> lth, tx_n = ((p.Wp >> L.level) + (1 << ltw) - 1) >> ltw, nt = ty_n * mk.nw;
        const bool lds = max(nk, nt) <= LDS_WORDS;
        u64 *km = lds ? s_k : reinterpret_cast<u64 *>(p.base + p.kbits_off);
        u64 *tm = lds ? s_t : reinterpret_cast<u64 *>(p.base + p.tbits_off);
        // The table is a chain: a layer's output is the input of the layer behind it, the one hg_need saw just before.  That map is
        // handed on in LDS (s_n) when it fits; only the skip tensors' maps, read many layers later, go through device memory.
        const u64 *om = L.out_chained && mo.h * mo.nw <= LDS_WORDS ? s_n : reinterpret_cast<const u64 *>(p.base + p.map_off[L.out]);
        // K: the units this layer must get right
        for (int i = tid; i < nk; i += NT) {
            const int y = i / mk.nw, wi = i - y * mk.nw;
            u64 k;
            if (sh == 0) {
                k = word(om, mo, y, wi);
            } else if (sh > 0) {
                k = spread2((unsigned)(word(om, mo, y >> 1, wi >> 1) >> (32 * (wi & 1))));
            } else {
                k = 0;
                for (int dy = 0; dy < 2; ++dy)
                    k |= (u64)pairs_any(word(om, mo, 2 * y + dy, 2 * wi)) | (u64)pairs_any(word(om, mo, 2 * y + dy, 2 * wi + 1)) << 32;
            }
            km[i] = k & row_mask(mk.w, wi);
        }
        __syncthreads();
        // what it reads
        u64 *ig = reinterpret_cast<u64 *>(p.base + p.map_off[L.in]), *im = L.in_chained && nk <= LDS_WORDS ? s_n : ig;
        u64 *sm = L.skip >= 0 ? reinterpret_cast<u64 *>(p.base + p.map_off[L.skip]) : nullptr;
        for (int i = tid; i < nk; i += NT) {
            const int y = i / mk.nw, wi = i - y * mk.nw;
            u64 v = km[i];
            if (L.ks == 3) {
                for (int dy = -1; dy <= 1; ++dy) {
                    const u64 c = word(km, mk, y + dy, wi);
                    v |= c | c << 1 | c >> 1 | word(km, mk, y + dy, wi - 1) >> 63 | word(km, mk, y + dy, wi + 1) << 63;
                }
                v &= row_mask(mk.w, wi);
            }
            im[i] = L.in_first ? v : (ig[i] | v);
            if (sm) sm[i] = L.skip_first ? v : (sm[i] | v);
        }
        // one bit per tile, at the lowest bit of the tile's bw bits: word wi of tile row ty is item ty * nw + wi
        const int r_sh = lth - lu;                    // tile row -> first map row: << r_sh, or >> -r_sh when the unit is taller
        for (int i = tid; i < nt; i += NT) {
            const int ty = i / mk.nw, wi = i - ty * mk.nw;
            const int r0 = r_sh >= 0 ? ty << r_sh : ty >> -r_sh, nr = r_sh >= 0 ? 1 << r_sh : 1;
            u64 v = 0;
            for (int r = r0; r < min(r0 + nr, mk.h); ++r) v |= km[r * mk.nw + wi];
            for (int s = 1; s < (1 << lbw); s <<= 1) v |= v >> s;
            tm[i] = v & k_tile_bits[lbw];
        }
        __syncthreads();
        // the list, ascending: thread t owns items [t * per, (t + 1) * per)
        const int per = (nt + NT - 1) / NT, c0 = tid * per, c1 = min(nt, c0 + per);
        int cnt = 0;
        for (int i = c0; i < c1; ++i) cnt += __popcll(tm[i]);
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if ((tid & 63) >= d) incl += v;
        }
        if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
        __syncthreads();
        int o = incl - cnt, total = 0;
        for (int w = 0; w < NT / 64; ++w) {
            const int v = s_wave[w];
            if (w < (tid >> 6)) o += v;
            total += v;
        }
        int *lst = reinterpret_cast<int *>(p.base + L.list_off);
        if (tid == 0) lst[0] = total;
        for (int i = c0; i < c1; ++i) {
            const int ty = i / mk.nw, wi = i - ty * mk.nw;
            for (u64 v = tm[i]; v; v &= v - 1) lst[1 + o++] = ty * tx_n + ((64 * wi + __ffsll(v) - 1) >> lbw);
        }
        // no barrier here: in front of its first barrier the next layer writes only K, which nobody has read since two barriers ago
    }
}

}  // namespace

hipError_t hg_need_launch(const HgNeedParams &p, hipStream_t s)
{
    if (!p.base || p.n_layers < 1 || p.n_layers > HG_NEED_MAX_LAYERS) return hipErrorInvalidValue;
    // what the kernel's word operations cover: units no larger than a tile, neighbouring levels' units within a factor 2 of the
    // same full-resolution size
    for (int i = 0; i < p.n_layers; ++i) {
        const HgNeedLayer &L = p.L[i];
        const int olev = L.level + (L.mode == 1 ? 1 : 0) - (L.mode == 2 ? 1 : 0);
        if (L.level < 0 || L.level >= HG_NEED_LEVELS || olev < 0 || olev >= HG_NEED_LEVELS) return hipErrorInvalidValue;
        const int sh = p.lu[olev] - p.lu[L.level] + olev - L.level;
        if (p.lu[L.level] < 0 || p.lu[L.level] > 4 || sh < -1 || sh > 1 || (L.th != 8 && L.th != 16) ||
            (L.tw != 0 && L.tw != 16 && L.tw != 32))
            return hipErrorInvalidValue;
    }
    if (p.lu[0] != 4) return hipErrorInvalidValue;      // hg_prep's flags are 16x16 cells
    hipLaunchKernelGGL(hg_need_kernel, dim3(1), dim3(NT), 0, s, p);
    return hipGetLastError();
}
