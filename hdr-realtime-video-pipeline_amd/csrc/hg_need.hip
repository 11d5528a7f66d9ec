// hg_need.hip -- which tiles of the Hallucination Generator can reach the output ("need lists").
//
// The head ends in out = mask * hg(img) + img with a 0/1 mask, cropped to H x W: an activation tile matters only if a masked
// output pixel depends on it.  hg_prep leaves one flag per 16x16 full-resolution cell that holds a masked pixel inside H x W; this
// kernel carries that set backwards through the layer table (consumer -> producer) at the granularity of 16x16-pixel cells of
// each level and leaves, per layer, the compacted list of kernel tiles to compute.  Everything stays in device memory: the
// launches behind it read the counts themselves, so the frame needs no host round trip and is capturable as a graph.
//
// Rules (conservative: any superset of the true dependency set gives the same output), K = the cells a layer computes:
//   K(layer)          = need(out tensor) for a layer that writes at its own level,
//                       the 2x2 up-sampling of it for a pool-fused layer (a 16x16 pre-pool tile lands in one cell one level down),
//                       the any-of-2x2 down-sampling for a pixel-shuffle layer (a tile at level l+1 writes 2x2 cells at level l);
//   need(in [, skip]) |= K dilated by one cell for a 3x3 layer (its halo), K itself for a 1x1 layer.
// A tensor with two readers collects both (the layers run in reverse launch order, so every reader is seen before the producer).
// One workgroup: the largest map of a 3840x2160 frame has 136 x 240 cells.
#include "launchers.h"

namespace {

constexpr int NT = 1024;

__device__ __forceinline__ int cells(int n) { return (n + 15) >> 4; }

__global__ __launch_bounds__(NT) void hg_need_kernel(HgNeedParams p)
{
    __shared__ int s_scan[NT];
    const int tid = threadIdx.x;
    // need maps of every tensor but the flags start empty
    for (int i = tid; i < p.maps_bytes; i += NT) p.base[p.maps_off + i] = 0;
    __syncthreads();
    for (int li = p.n_layers - 1; li >= 0; --li) {
        const HgNeedLayer L = p.L[li];
        const int gh = cells(p.Hp >> L.level), gw = cells(p.Wp >> L.level), n = gh * gw;
        const int olev = L.level + (L.mode == 1 ? 1 : 0) - (L.mode == 2 ? 1 : 0);
        const int oh = cells(p.Hp >> olev), ow = cells(p.Wp >> olev);
        const unsigned char *om = p.base + p.map_off[L.out];
        unsigned char *km = p.base + p.kmap_off;
        // K: the cells this layer computes
        for (int i = tid; i < n; i += NT) {
            const int y = i / gw, x = i - y * gw;
            int k;
            if (L.mode == 1) {
                k = om[min(y >> 1, oh - 1) * ow + min(x >> 1, ow - 1)];
            } else if (L.mode == 2) {
                k = 0;
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx)
                        if (2 * y + dy < oh && 2 * x + dx < ow) k |= om[(2 * y + dy) * ow + 2 * x + dx];
            } else {
                k = om[i];
            }
            km[i] = (unsigned char)(k != 0);
        }
        __syncthreads();
        // what it reads
        unsigned char *im = p.base + p.map_off[L.in], *sm = L.skip >= 0 ? p.base + p.map_off[L.skip] : nullptr;
        for (int i = tid; i < n; i += NT) {
            const int y = i / gw, x = i - y * gw;
            int v = km[i];
            if (L.ks == 3 && !v) {
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        if ((unsigned)(y + dy) < (unsigned)gh && (unsigned)(x + dx) < (unsigned)gw) v |= km[(y + dy) * gw + x + dx];
            }
            if (v) {
                im[i] = 1;
                if (sm) sm[i] = 1;
            }
        }
        // the list, in raster order of the cells: thread t owns cells [t * per, (t + 1) * per).  8-row kernel tiles: a cell is
        // the tiles (2 y, x) and (2 y + 1, x), the second only where the map has that tile row
        const int per = (n + NT - 1) / NT, c0 = tid * per, c1 = min(n, c0 + per);
        const int ty8 = ((p.Hp >> L.level) + 7) >> 3;
        int cnt = 0;
        for (int i = c0; i < c1; ++i)
            if (km[i]) cnt += (L.th == 8 && 2 * (i / gw) + 1 < ty8) ? 2 : 1;
        s_scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < NT; d <<= 1) {
            const int v = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        int *lst = reinterpret_cast<int *>(p.base + L.list_off);
        int o = s_scan[tid] - cnt;
        if (tid == NT - 1) lst[0] = s_scan[tid];
        for (int i = c0; i < c1; ++i) {
            if (!km[i]) continue;
            const int y = i / gw, x = i - y * gw;
            if (L.th == 8) {
                lst[1 + o++] = 2 * y * gw + x;
                if (2 * y + 1 < ty8) lst[1 + o++] = (2 * y + 1) * gw + x;
            } else {
                lst[1 + o++] = i;
            }
        }
        __syncthreads();
    }
    // the flags are consumed: hg_prep only ever sets them
    const int n0 = cells(p.Hp) * cells(p.Wp);
    for (int i = tid; i < n0; i += NT) p.base[p.flags_off + i] = 0;
}

}  // namespace

hipError_t hg_need_launch(const HgNeedParams &p, hipStream_t s)
{
    if (!p.base || p.n_layers < 1 || p.n_layers > HG_NEED_MAX_LAYERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hg_need_kernel, dim3(1), dim3(NT), 0, s, p);
    return hipGetLastError();
}
