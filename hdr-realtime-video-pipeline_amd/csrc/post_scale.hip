// post_scale.hip -- RGB48 at the display size in one launch (gfx950): the u16 quantiser of post_rgb48 / post_pq_rgb48 and a
// separable six-tap Lanczos-3 upscale of its codes (hdrtv_post_rgb48_scaled; include/hdrtv_mi355x.h states the integer rule).
// Doing it as post_rgb48 + a resize kernel would write and re-read a frame of codes, and the PQ variant would run pq_code on
// dH x dW values rather than H x W.
//
// The tile body -- schedule, LDS layout, bank reasoning -- is post_scale_tile.h's post_scale_tile, shared with the anti-ringing
// instances of post_scale_ar.hip; here it is instantiated with AR = false, which compiles nothing of the anti-ringing.
#include "launchers.h"
#include "post_scale_tile.h"

namespace {

template <typename T, bool PQ>
__global__ __launch_bounds__(256) void post_scale_kernel(PostScaleParams p)
{
    post_scale_tile<T, PQ, false>(p, 0);
}

}  // namespace

// pq != 0 needs p.pq_bnd (hdrtv_api.hip pq_boundaries).  Needs dH >= H, dW >= W: the LDS footprint bound rests on it.
hipError_t post_scale_launch(const PostScaleParams &p, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || (pq && !p.pq_bnd)) return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH), b(256);
    if (is_f32) {
        if (pq) hipLaunchKernelGGL((post_scale_kernel<float, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((post_scale_kernel<float, false>), g, b, 0, s, p);
    } else {
        if (pq) hipLaunchKernelGGL((post_scale_kernel<f16, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((post_scale_kernel<f16, false>), g, b, 0, s, p);
    }
    return hipGetLastError();
}
