// post_scale_ar.hip -- hdrtv_post_rgb48_scaled_ex with a nonzero strength (gfx950): post_scale.hip's kernel -- the same 32 x 64
// tile, staging, passes and stores (post_scale_tile.h) -- with each pass pulled towards the interval of its two inner taps
// (include/hdrtv_mi355x.h states the integer rule).  The instances live in a file of their own so that post_scale.hip keeps its
// four kernels and their code as they were: a strength of 0 launches those, never these.  The strength is a kernel argument beside
// PostScaleParams, uniform over the launch (an SGPR).
#include "launchers.h"
#include "post_scale_tile.h"

namespace {

template <typename T, bool PQ>
__global__ __launch_bounds__(256) void post_scale_ar_kernel(PostScaleParams p, int antiring)
{
    post_scale_tile<T, PQ, true>(p, antiring);
}

}  // namespace

// antiring 1 .. 256; otherwise post_scale_launch's conditions.
hipError_t post_scale_ar_launch(const PostScaleParams &p, int antiring, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || (pq && !p.pq_bnd) || antiring < 1 || antiring > 256) return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH), b(256);
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((post_scale_ar_kernel<float, true>), g, b, 0, s, p, antiring);
        else hipLaunchKernelGGL((post_scale_ar_kernel<float, false>), g, b, 0, s, p, antiring);
    } else {
        if (pq) hipLaunchKernelGGL((post_scale_ar_kernel<f16, true>), g, b, 0, s, p, antiring);
        else hipLaunchKernelGGL((post_scale_ar_kernel<f16, false>), g, b, 0, s, p, antiring);
    }
    return hipGetLastError();
}
