// tile_run.h -- how the persistent convolutions hand `total` tiles to G workgroups, and how a workgroup walks an HG need list
// (ConvParams::tile_list, hg_need.hip) along its run.  The split is plain integer arithmetic, callable on host and device (a
// launcher asks it how long a run can get; tests/test_tile_run_host.py runs it on the CPU).
#pragma once

#if defined(__HIPCC__)
#define TILE_RUN_FN __host__ __device__ __forceinline__
#else
#define TILE_RUN_FN inline
#endif

// Workgroup b runs on XCD b & 7 (own L2).  XCD x owns a contiguous range of the tiles -- xcd_base(total, x) is its start, the
// first total & 7 ranges are one longer -- so that neighbours in the tile order share halos or weight slabs in one L2.
TILE_RUN_FN int xcd_base(int total, int xcd)
{
    const int q = total >> 3, r = total & 7;
    return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}
// one tile per workgroup (total == gridDim.x): the bijective remap
TILE_RUN_FN int xcd_tile(int total, int b) { return xcd_base(total, b & 7) + (b >> 3); }

// A persistent workgroup's run: tiles t_first + k * t_step, k < ntile.  The workgroups of an XCD interleave in its range.
// Precondition: every XCD with tiles has a workgroup, i.e. G >= 8 or G >= total -- the launchers take G = min(dense total, n_cu)
// and refuse n_cu < 8.  (With G < 8 and total > G the ranges of XCDs G .. 7 would be nobody's.)
struct TileRun { int t_first, t_step, ntile; };
TILE_RUN_FN TileRun tile_run(int total, int G, int b)
{
    const int xcd = b & 7, slot = b >> 3;
    const int nslots = (G - xcd + 7) >> 3;
    const int len = (total >> 3) + (xcd < (total & 7) ? 1 : 0);
    return {xcd_base(total, xcd) + slot, nslots, slot < len ? (len - slot + nslots - 1) / nslots : 0};
}

// The longest run of a launch with `total` tiles (all of them: a need list only shortens runs, and its count lies in device
// memory) on `grid` = min(total, n_cu) workgroups, n_cu >= 8 (tile_run's precondition): below eight workgroups grid == total,
// one tile each.
TILE_RUN_FN int tile_run_longest(int total, int grid) { return grid >= 8 ? (total / 8 + 1 + grid / 8 - 1) / (grid / 8) : 1; }

// ---- need lists.  list[0] = the count, list[1 ..] = spatial tile indices.  A kernel copies the entries of its run into an LDS
// block of TILE_LIST_N ints in its prologue; the tile loop's only new operation is then one LDS read per tile -- no scalar or
// vector memory load enters a stream whose vmcnt waits are counted by hand.
constexpr int TILE_LIST_N = 512;
// Whether a launcher may pass the list on: every run fits the LDS block.  min_grid = 8: the kernel takes no list on a grid
// below eight (conv_prw); min_grid = 1: it does (conv_pglds, conv_glds1p).
TILE_RUN_FN bool tile_list_fits(int total, int grid, int min_grid)
{
    return grid >= min_grid && tile_run_longest(total, grid) <= TILE_LIST_N;
}

#if defined(__HIPCC__)
// An LDS-space pointer: through a generic one the volatile accesses are FLAT operations, and the write a store vmcnt would count.
typedef volatile __attribute__((address_space(3))) int *tile_list_lds_t;
// Thread tid < run.ntile copies the entry of run step tid; pos(t) = the list position of tile t (the kernel's tile order).  A null
// list stages nothing: conv_glds1p calls this unconditionally, and where a caller has tested the list itself (conv_prw and
// conv_pglds, around their own wait) hipcc folds the second test away.  The block is valid behind the caller's next barrier.  A wait between the two, where the kernel counts, is the kernel's.
template <class Pos> __device__ __forceinline__ void tile_list_stage(tile_list_lds_t s, const int *list, const TileRun &run, int tid, Pos pos)
{
    if (list && tid < run.ntile) s[tid] = list[1 + pos(run.t_first + tid * run.t_step)];
}
// the spatial tile of run step k, wave-uniform
__device__ __forceinline__ int tile_list_at(tile_list_lds_t s, int k) { return __builtin_amdgcn_readfirstlane(s[k]); }
#endif

#undef TILE_RUN_FN
