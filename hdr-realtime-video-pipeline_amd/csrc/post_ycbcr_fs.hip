// post_ycbcr_fs.hip -- the 10-bit Y'CbCr conversions of post_ycbcr.hip with Floyd-Steinberg error diffusion in place of the rounding
// (hdrtv_post_ycbcr10_fs / hdrtv_rgb48_to_ycbcr10_fs; include/hdrtv_mi355x.h states the integer rule) on the device (gfx950).
// Two launches on the caller's stream, through the caller's scratch:
//
//   1. samples   post_ycbcr_tile.h with MODE = YC_FS_SAMPLES: the tile code of the plain conversion, fully parallel, writing every
//                sample in 1/4096 code (u of the rule) as int32 into three planes of the scratch.  P010 and yuv420p10 share the
//                4:2:0 instances (the planes are not interleaved here).
//   2. diffusion fs_diffuse_kernel, three workgroups of FS_ROWS = 256 lanes: one independent chain per plane (P010: the Cb and Cr
//                chains write one interleaved plane, x stride 2).  Sample (x, y) needs the residuals of (x-1, y), (x-1, y-1),
//                (x, y-1) and (x+1, y-1), so a lane owns a row and the rows run as a skewed wavefront: at step t lane r works on
//                column  t - off(r),  off(r) = 2 r + FS_SKEW * (r / 64).
//
// Hand-off.  After column x a lane holds the complete error of column x - 1 of the row below (d of x-2, c of x-1, b of x, summed
// in the upper lane: `out`); the lane below takes it with one DPP wave shift (wave_shr:1) at the start of the next step, when it
// works on exactly that column.  No barrier inside a wave.  Lane 63 of a wave hands to lane 0 of the next wave through LDS: it
// collects its `out` of the 32 steps of a phase (v_readlane and a select into lane j, no divergence), the wave writes them to
// hand[wave][] at the end of the phase, and the stager adds hand[wave][j] to the sample the next wave's top row reads at slot j of the NEXT phase --
// that is why a wave trails the wave above it by FS_SKEW = FS_CHUNK - 1 further columns: off(64 w) = off(64 w - 1) + 2 + FS_SKEW puts
// the reader exactly FS_CHUNK steps, one phase, behind the writer.  The last lane's `out` (hand[3]) goes to the plane's carry row in
// the scratch; the next row group's top row gets it added the same way.  Every row beyond the first therefore sees a plain
// "u + E" in its LDS slot, and the step itself has no special lane.
//
// Staging.  A lane-per-row walk over global memory would touch 256 rows per access.  Instead a phase of FS_CHUNK = 32 steps works on
// buf[phase & 1][r][j] = the sample lane r needs at step j of the phase (the skew is taken out when the chunk is staged), and the
// 256 lanes stage it as 32 lanes x 8 rows per access: 32 neighbouring int32 of one row = 128 contiguous bytes in, 32 neighbouring
// u16 out.  The loads of phase p + 1 are issued before the steps of phase p and land in registers (32 per lane); the steps
// overwrite their slot with k; after the barrier the results of phase p are stored and the registers written to the other buffer.
// Two barriers per phase; every wave reaches both, whatever its rows (rows below the plane and columns outside it compute on zeros
// with the residual forced to zero, and are never stored).  Every loop bound (row groups, phases) is computed from h and w before
// the loop; no kernel waits on another workgroup.
//
// A row group takes w + FS_TAIL steps (the last lane starts off(255) = 603 steps late and runs one flush step past the last
// column), row groups of a plane follow each other in the same workgroup.
// LDS: rows are FS_CHUNK + 1 = 33 dwords apart, so the 32 lanes of a half wave hit 32 different banks in a step (ds_read_b32 /
// ds_write_b32: bank = dword address mod 32) and a staging access (32 columns of a row, two rows per wave) likewise.
//   buf 2 x 256 x 33 x 4 = 67584 bytes, hand 4 x 32 x 4 = 512 bytes: 68096 bytes, one workgroup per CU (three in the grid).
#include "post_ycbcr_tile.h"

namespace {

constexpr int FS_WAVES = FS_ROWS / 64;
constexpr int FS_SKEW = FS_CHUNK - 1;                                       // further columns a wave trails the wave above it by
constexpr int FS_LS = FS_CHUNK + 1;                                         // LDS row stride in dwords
constexpr int FS_TAIL = 2 * (FS_ROWS - 1) + FS_SKEW * (FS_WAVES - 1) + 1;   // off(FS_ROWS - 1) + the flush step
constexpr int FS_STAGE_ROWS = FS_ROWS / FS_CHUNK;                           // rows one staging access covers
static_assert(FS_ROWS == HDRTV_FS_ROWS && FS_CHUNK == HDRTV_FS_CHUNK, "the header states the two constants");
static_assert(FS_ROWS == 256 && FS_CHUNK == 32 && FS_STAGE_ROWS == 8, "the staging map (32 lanes x 8 rows, 32 accesses) and hand[] assume these");

__device__ __forceinline__ constexpr int fs_off(int r) { return 2 * r + FS_SKEW * (r >> 6); }

// lane l gets lane l - 1's value, lane 0 gets 0 (DPP wave_shr:1; all 64 lanes are active wherever this is called)
__device__ __forceinline__ int from_lane_above(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }

__global__ __launch_bounds__(FS_ROWS) void fs_diffuse_kernel(FsParams p)
{
    __shared__ int32_t buf[2][FS_ROWS][FS_LS];
    __shared__ int32_t hand[FS_WAVES][FS_CHUNK];
    FsPlane q = p.pl[0];
    if (blockIdx.x == 1) q = p.pl[1];
    if (blockIdx.x == 2) q = p.pl[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sj = tid & (FS_CHUNK - 1), sr = tid / FS_CHUNK;       // staging: this lane's slot, and its rows sr + 8 i
    const int my_off = fs_off(tid);
    const size_t u_step = (size_t)FS_STAGE_ROWS * q.w, d_step = (size_t)FS_STAGE_ROWS * q.pitch;
    const int n_groups = (q.h + FS_ROWS - 1) / FS_ROWS;
    const int n_phases = (q.w + FS_TAIL + FS_CHUNK - 1) / FS_CHUNK;

    for (int g = 0; g < n_groups; ++g) {
        const int row0 = g * FS_ROWS;
        const bool row_ok = row0 + tid < q.h;
        int pre[FS_CHUNK];
        // the samples phase `ph` reads, skew taken out, into registers; row 0 of a later row group with the carried error row added
        auto load = [&](int ph) {
            const int xs = ph * FS_CHUNK + sj - 2 * sr;
            const int32_t *urow = q.u + (size_t)(row0 + sr) * q.w;
#pragma unroll
            for (int i = 0; i < FS_CHUNK; ++i, urow += u_step) {
                const int x = xs - fs_off(FS_STAGE_ROWS * i), row = row0 + sr + FS_STAGE_ROWS * i;
                const bool ok = row < q.h && (unsigned)x < (unsigned)q.w;
                const int v = *(ok ? urow + x : q.u);           // no branch: a sample outside the plane reads u[0] and becomes 0
                pre[i] = ok ? v : 0;
                if (i == 0 && ok && sr == 0 && g > 0) pre[0] += q.carry[x];
            }
        };
        // the registers into buf[b]; the top row of waves 1 .. 3 with what lane 63 of the wave above handed over a phase ago
        auto fill = [&](int b, bool handed) {
#pragma unroll
            for (int i = 0; i < FS_CHUNK; ++i) {
                int v = pre[i];
                if (handed && i > 0 && i % (64 / FS_STAGE_ROWS) == 0 && sr == 0) v += hand[i / (64 / FS_STAGE_ROWS) - 1][sj];
                buf[b][sr + FS_STAGE_ROWS * i][sj] = v;
            }
        };
        load(0);
        fill(0, false);
        __syncthreads();

        int right = 0, part = 0, dprev = 0, out = 0;
        for (int ph = 0; ph < n_phases; ++ph) {
            int32_t(*cur)[FS_LS] = buf[ph & 1];
            load(ph + 1);
            const int x0 = ph * FS_CHUNK - my_off;
            int outs = 0;
#pragma unroll
            for (int j = 0; j < FS_CHUNK; ++j) {
                const bool act = row_ok && (unsigned)(x0 + j) < (unsigned)q.w;
                const int v = cur[tid][j] + from_lane_above(out) + right;
                const int k = min(max((v + 2048) >> 12, q.lo), q.hi);
                int r = min(max(v - (k << 12), -2048), 2047);
                r = act ? r : 0;
                const int a = (7 * r) >> 4, b = (3 * r) >> 4, c = (5 * r) >> 4, d = r - a - b - c;
                right = a;
                out = part + b;
                part = dprev + c;
                dprev = d;
                cur[tid][j] = k;
                const int out63 = __builtin_amdgcn_readlane(out, 63);
                outs = lane == j ? out63 : outs;
            }
            if (lane < FS_CHUNK) hand[wave][lane] = outs;
            __syncthreads();

            // the results of this phase, and the last lane's hand-over to the carry row
            {
                const int xs = ph * FS_CHUNK + sj - 2 * sr;
                uint16_t *drow = q.dst + (size_t)(row0 + sr) * q.pitch;
                int kk[FS_CHUNK];
#pragma unroll
                for (int i = 0; i < FS_CHUNK; ++i) kk[i] = cur[sr + FS_STAGE_ROWS * i][sj];       // all LDS reads first: one wait
#pragma unroll
                for (int i = 0; i < FS_CHUNK; ++i, drow += d_step) {
                    const int x = xs - fs_off(FS_STAGE_ROWS * i), row = row0 + sr + FS_STAGE_ROWS * i;
                    if (row < q.h && (unsigned)x < (unsigned)q.w) drow[(size_t)x * q.xstride] = (uint16_t)((q.base + kk[i]) << q.shl);
                }
                const int xc = ph * FS_CHUNK + tid - fs_off(FS_ROWS - 1) - 1;
                if (tid < FS_CHUNK && (unsigned)xc < (unsigned)q.w) q.carry[xc] = hand[FS_WAVES - 1][tid];
            }
            fill((ph + 1) & 1, true);
            __syncthreads();
        }
    }
}

template <typename T, bool PQ, int FMT>
__global__ __launch_bounds__(256) void post_ycc10_fs_samples_kernel(Ycbcr10Params p)
{
    const TensorSrc<T, PQ> src{static_cast<const T *>(p.in), (size_t)p.H * p.W, p.W, p.peak, p.pq_bnd};
    ycbcr_tile<TensorSrc<T, PQ>, FMT, YC_FS_SAMPLES>(src, p);
}

template <int FMT>
__global__ __launch_bounds__(256) void rgb48_ycc10_fs_samples_kernel(Ycbcr10Params p)
{
    const Rgb48Src src{static_cast<const uint16_t *>(p.in), p.W};
    ycbcr_tile<Rgb48Src, FMT, YC_FS_SAMPLES>(src, p);
}

template <typename T, bool PQ>
void launch_samples(const Ycbcr10Params &p, dim3 g, hipStream_t s)
{
    if (p.fmt == HDRTV_YCC_YUV422P10) hipLaunchKernelGGL((post_ycc10_fs_samples_kernel<T, PQ, HDRTV_YCC_YUV422P10>), g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((post_ycc10_fs_samples_kernel<T, PQ, HDRTV_YCC_YUV420P10>), g, dim3(256), 0, s, p);
}

// the scratch: int32 planes Y' [H][W], Cb and Cr [CH][W / 2], then one carry row per plane
struct FsScratch {
    int32_t *u[3], *carry[3];
    int ch, cw;
};

FsScratch fs_scratch(const Ycbcr10Params &p, void *scratch)
{
    FsScratch f;
    f.ch = p.fmt == HDRTV_YCC_YUV422P10 ? p.H : p.H / 2;
    f.cw = p.W / 2;
    int32_t *base = static_cast<int32_t *>(scratch);
    f.u[0] = base;
    f.u[1] = f.u[0] + (size_t)p.H * p.W;
    f.u[2] = f.u[1] + (size_t)f.ch * f.cw;
    f.carry[0] = f.u[2] + (size_t)f.ch * f.cw;
    f.carry[1] = f.carry[0] + p.W;
    f.carry[2] = f.carry[1] + f.cw;
    return f;
}

bool fs_args_ok(const Ycbcr10Params &p, const void *scratch)
{
    return ycbcr_params_ok(p) && scratch && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0;
}

// the parameters of the samples pass: the conversion's own, its planes the scratch's (pitches in int32), P010 as planar 4:2:0
Ycbcr10Params samples_params(const Ycbcr10Params &p, const FsScratch &f)
{
    Ycbcr10Params sp = p;
    sp.dst_y = reinterpret_cast<uint16_t *>(f.u[0]);
    sp.dst_u = reinterpret_cast<uint16_t *>(f.u[1]);
    sp.dst_v = reinterpret_cast<uint16_t *>(f.u[2]);
    sp.y_pitch = p.W;
    sp.c_pitch = f.cw;
    if (p.fmt == HDRTV_YCC_P010) sp.fmt = HDRTV_YCC_YUV420P10;
    return sp;
}

hipError_t diffuse_launch(const Ycbcr10Params &p, const FsScratch &f, hipStream_t s)
{
    const bool p010 = p.fmt == HDRTV_YCC_P010;
    const int shl = p010 ? 6 : 0;
    FsParams d;
    d.pl[0] = FsPlane{f.u[0], f.carry[0], p.dst_y, p.H, p.W, p.y_pitch, 1, 0, 876, 64, shl};
    d.pl[1] = FsPlane{f.u[1], f.carry[1], p.dst_u, f.ch, f.cw, p.c_pitch, p010 ? 2 : 1, -448, 448, 512, shl};
    d.pl[2] = FsPlane{f.u[2], f.carry[2], p010 ? p.dst_u + 1 : p.dst_v, f.ch, f.cw, p.c_pitch, p010 ? 2 : 1, -448, 448, 512, shl};
    hipLaunchKernelGGL(fs_diffuse_kernel, dim3(3), dim3(FS_ROWS), 0, s, d);
    return hipGetLastError();
}

}  // namespace

int64_t ycbcr10_fs_scratch_bytes(int fmt, int H, int W)
{
    if (H <= 0 || W <= 0 || (W & 1)) return -1;
    if (fmt != HDRTV_YCC_P010 && fmt != HDRTV_YCC_YUV420P10 && fmt != HDRTV_YCC_YUV422P10) return -1;
    if (fmt != HDRTV_YCC_YUV422P10 && (H & 1)) return -1;
    const int64_t ch = fmt == HDRTV_YCC_YUV422P10 ? H : H / 2, cw = W / 2;
    return 4 * ((int64_t)H * W + 2 * ch * cw + W + 2 * cw);
}

// the argument rules of post_ycbcr10_launch / rgb48_to_ycbcr10_launch, and a scratch of ycbcr10_fs_scratch_bytes bytes, 4-byte aligned
hipError_t post_ycbcr10_fs_launch(const Ycbcr10Params &p, int is_f32, int pq, void *scratch, int passes, hipStream_t s)
{
    if (!fs_args_ok(p, scratch) || (pq && !p.pq_bnd) || !(passes & 3)) return hipErrorInvalidValue;
    const FsScratch f = fs_scratch(p, scratch);
    if (passes & 1) {
        const Ycbcr10Params sp = samples_params(p, f);
        const dim3 g((p.W + YC_TW - 1) / YC_TW, (p.H + YC_TH - 1) / YC_TH);
        if (is_f32) {
            if (pq) launch_samples<float, true>(sp, g, s);
            else launch_samples<float, false>(sp, g, s);
        } else {
            if (pq) launch_samples<f16, true>(sp, g, s);
            else launch_samples<f16, false>(sp, g, s);
        }
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return (passes & 2) ? diffuse_launch(p, f, s) : hipSuccess;
}

hipError_t rgb48_to_ycbcr10_fs_launch(const Ycbcr10Params &p, void *scratch, int passes, hipStream_t s)
{
    if (!fs_args_ok(p, scratch) || !(passes & 3)) return hipErrorInvalidValue;
    const FsScratch f = fs_scratch(p, scratch);
    if (passes & 1) {
        const Ycbcr10Params sp = samples_params(p, f);
        const dim3 g((p.W + YC_TW - 1) / YC_TW, (p.H + YC_TH - 1) / YC_TH);
        if (sp.fmt == HDRTV_YCC_YUV422P10) hipLaunchKernelGGL((rgb48_ycc10_fs_samples_kernel<HDRTV_YCC_YUV422P10>), g, dim3(256), 0, s, sp);
        else hipLaunchKernelGGL((rgb48_ycc10_fs_samples_kernel<HDRTV_YCC_YUV420P10>), g, dim3(256), 0, s, sp);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return (passes & 2) ? diffuse_launch(p, f, s) : hipSuccess;
}
