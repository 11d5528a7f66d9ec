// post_fsr_grain.hip -- hdrtv_post_rgb48_fsr_grain with a nonzero intensity (gfx950): post_fsr.hip's kernel -- the same tile,
// staging, EASU and RCAS (post_fsr_body.h; post_fsr.hip, included here, has the functions it calls) -- with the film grain (film_grain.h; include/hdrtv_mi355x.h states the rule) applied to
// the final code of every output pixel at its own position over dH x dW: in the reference's chain EASU and RCAS hook MAIN first
// and enlarge it, and the grain shader comes after them.  The instances live in a file of their own so that post_fsr.hip keeps its
// eight kernels and their code: an intensity of 0 launches those, never these.  Built with -ffp-contract=off like post_fsr.hip.
// Intensity and seed are kernel arguments beside PostFsrParams and the sharpness, uniform over the launch (SGPRs).
#define POST_FSR_HELPERS_ONLY
#include "post_fsr.hip"

namespace {

template <typename T, bool PQ, bool RCAS>
__global__ __launch_bounds__(256) void post_fsr_grain_kernel(const PostFsrParams p, const float sharp, const float intensity, const float seed)
{
    constexpr bool GRAIN = true;
#include "post_fsr_body.h"
}

template <typename T, bool PQ>
void launch(const PostFsrParams &p, int rcas, float sharp, float intensity, float seed, dim3 g, hipStream_t s)
{
    if (rcas) hipLaunchKernelGGL((post_fsr_grain_kernel<T, PQ, true>), g, dim3(256), 0, s, p, sharp, intensity, seed);
    else hipLaunchKernelGGL((post_fsr_grain_kernel<T, PQ, false>), g, dim3(256), 0, s, p, 0.f, intensity, seed);
}

}  // namespace

// 0 < intensity <= 0.1, 0 <= seed < 1; otherwise post_fsr_launch's conditions.
hipError_t post_fsr_grain_launch(const PostFsrParams &p, int rcas, float sharp, float intensity, float seed, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || p.dH > 2 * (long long)p.H || p.dW > 2 * (long long)p.W || (pq && !p.pq_bnd) ||
        (rcas && !(sharp >= 0.25f && sharp <= 1.f)) || !(intensity > 0.f && intensity <= 0.1f) || !(seed >= 0.f && seed < 1.f))
        return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH);
    if (is_f32) {
        if (pq) launch<float, true>(p, rcas, sharp, intensity, seed, g, s);
        else launch<float, false>(p, rcas, sharp, intensity, seed, g, s);
    } else {
        if (pq) launch<f16, true>(p, rcas, sharp, intensity, seed, g, s);
        else launch<f16, false>(p, rcas, sharp, intensity, seed, g, s);
    }
    return hipGetLastError();
}
