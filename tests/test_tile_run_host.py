"""csrc/tile_run.h on the CPU: the split of a launch's tiles over the workgroups of eight XCDs, the longest run a launcher
reckons with, and the rule by which the three need-list launchers keep or drop a list.

The header's functions are plain integer arithmetic, callable on the host; a stand-alone program (its own main) runs them
against a mirror of the formula as the five persistent kernels each carried it before the header existed, so that "unchanged"
is pinned and not only "self-consistent".  Cases: n_cu in {8, 9, 15, 16, 37, 255, 256, 304}, dense totals 1 .. 699, grid =
min(total, n_cu), and the counts a need list can shrink the launch to: total, total - 1, total - 7, total / 2, 1, 0."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
# a host C++ compiler: the system's, else the clang++ that hipcc itself drives (the library cannot be built without it)
_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
_ROCM_CLANG = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_HIPCC))), "lib", "llvm", "bin", "clang++")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (_ROCM_CLANG if os.path.exists(_ROCM_CLANG) else None)

PROGRAM = r"""
#include <cstdio>
#include <vector>

#include "tile_run.h"

// the block conv_prw, conv_prw_i8, conv_pglds, conv_pglds_i8 and conv_glds1p each carried, character for character
static void mirror(int total, int gridDim_x, int blockIdx_x, int &t_first, int &t_step, int &ntile)
{
    const int G = gridDim_x, b = blockIdx_x, xcd = b & 7, slot = b >> 3;
    const int nslots = (G - xcd + 7) >> 3;
    const int q = total >> 3, r = total & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int len = q + (xcd < r ? 1 : 0);
    t_first = base + slot;
    t_step = nslots;
    ntile = slot < len ? (len - slot + nslots - 1) / nslots : 0;
}
// ... and conv_igemm's / conv_glds1's one tile per workgroup
static int mirror_one(int nwg, int b)
{
    const int q = nwg >> 3, r = nwg & 7, xcd = b & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}
// the launchers' expressions (a list is kept unless ...), LIST_N = 512
static bool prw_keeps(int total, int grid) { return !(grid < 8 || (total / 8 + 1 + grid / 8 - 1) / (grid / 8) > 512); }
static bool pglds_keeps(int total, int grid) { return !(grid >= 8 && (total / 8 + 1 + grid / 8 - 1) / (grid / 8) > 512); }

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main()
{
    const int ncus[] = {8, 9, 15, 16, 37, 255, 256, 304};
    long runs = 0, keeps = 0, drops = 0;
    std::vector<int> seen;
    for (int n_cu : ncus) {
        for (int total = 1; total <= 699; ++total) {
            const int grid = total < n_cu ? total : n_cu;
            const int bound = tile_run_longest(total, grid);
            const int counts[] = {total, total - 1, total - 7, total / 2, 1, 0};
            for (int cnt : counts) {
                if (cnt < 0) continue;
                seen.assign(cnt, 0);
                int longest = 0;
                for (int b = 0; b < grid; ++b) {
                    const TileRun r = tile_run(cnt, grid, b);
                    int mf, ms, mn;
                    mirror(cnt, grid, b, mf, ms, mn);
                    CHECK(r.t_first == mf && r.t_step == ms && r.ntile == mn, "(c) total %d grid %d b %d", cnt, grid, b);
                    CHECK(r.ntile >= 0, "ntile %d", r.ntile);
                    if (r.ntile > longest) longest = r.ntile;
                    for (int k = 0; k < r.ntile; ++k) {
                        const int t = r.t_first + k * r.t_step;
                        CHECK(t >= 0 && t < cnt, "(a) tile %d outside 0 .. %d (grid %d b %d)", t, cnt, grid, b);
                        if (t >= 0 && t < cnt) ++seen[t];
                    }
                    ++runs;
                }
                for (int t = 0; t < cnt; ++t) CHECK(seen[t] == 1, "(a) tile %d of %d covered %d times (grid %d)", t, cnt, seen[t], grid);
                if (grid >= 8) CHECK(longest <= bound, "(b) run of %d > bound %d (dense %d, count %d, grid %d)", longest, bound, total, cnt, grid);
                else CHECK(longest <= 1, "(b) run of %d on a grid of %d", longest, grid);
            }
            // one tile per workgroup: the base-only form is run step 0 of a grid as large as the launch, and a bijection
            seen.assign(total, 0);
            for (int b = 0; b < total; ++b) {
                const int t = xcd_tile(total, b);
                CHECK(t == mirror_one(total, b), "xcd_tile(%d, %d)", total, b);
                CHECK(t == tile_run(total, total, b).t_first && tile_run(total, total, b).ntile == 1, "xcd_tile vs tile_run (%d, %d)", total, b);
                if (t >= 0 && t < total) ++seen[t];
            }
            for (int t = 0; t < total; ++t) CHECK(seen[t] == 1, "xcd_tile: tile %d of %d covered %d times", t, total, seen[t]);
        }
        // (d) over the cases above, and on to the totals at which a run outgrows the LDS block (8 workgroups: 4088 tiles)
        for (int total = 1; total <= 160000; total += (total <= 699 || (total >= 4000 && total <= 4200)) ? 1 : 37) {
            const int grid = total < n_cu ? total : n_cu;
            const bool k8 = tile_list_fits(total, grid, 8), k1 = tile_list_fits(total, grid, 1);
            CHECK(k8 == prw_keeps(total, grid), "(d) min_grid 8: total %d grid %d", total, grid);
            CHECK(k1 == pglds_keeps(total, grid), "(d) min_grid 1: total %d grid %d", total, grid);
            keeps += k1; drops += !k1;
        }
    }
    CHECK(TILE_LIST_N == 512, "TILE_LIST_N %d", TILE_LIST_N);
    printf("runs %ld keeps %ld drops %ld fails %ld\n", runs, keeps, drops, fails);
    return fails ? 1 : 0;
}
"""


def test_tile_run_header_on_the_host(tmp_path):
    assert CXX is not None, "no host C++ compiler: neither c++, g++ nor clang++ on PATH, nor " + _ROCM_CLANG
    src = tmp_path / "tile_run_host.cpp"
    exe = tmp_path / "tile_run_host"
    src.write_text(PROGRAM)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    # the loops ran: one run per (n_cu, total, count >= 0, workgroup)
    want = 0
    for n_cu in (8, 9, 15, 16, 37, 255, 256, 304):
        for total in range(1, 700):
            counts = [c for c in (total, total - 1, total - 7, total // 2, 1, 0) if c >= 0]
            want += len(counts) * min(total, n_cu)
    words = r.stdout.split()
    assert int(words[words.index("runs") + 1]) == want
    # both answers of the predicate were seen
    assert int(words[words.index("keeps") + 1]) > 0 and int(words[words.index("drops") + 1]) > 0
