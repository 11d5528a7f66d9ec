// post_scale_cas.hip -- hdrtv_post_rgb48_scaled_cas with a nonzero CAS code (gfx950): post_scale.hip's kernel -- the same 32 x 64
// tile, passes and stores (post_scale_tile.h) -- with the staged codes sharpened before the passes read them: FidelityFX
// contrast-adaptive sharpening as ffmpeg's cas filter has it, restated in integers (include/hdrtv_mi355x.h).  The raw codes and
// their one-pixel halo lie in the storage of the horizontal sums, which are not live yet: the LDS of the plain form, one barrier
// more.  The passes come plain and anti-ringed (the strength acts on the sharpened codes); the instances live in a file of their
// own so that post_scale.hip and post_scale_ar.hip keep their kernels and their code: a CAS code of 0 launches those, never these.
// Both numbers are kernel arguments beside PostScaleParams, uniform over the launch (SGPRs).
#include "launchers.h"
#include "post_scale_tile.h"

namespace {

template <typename T, bool PQ, bool AR>
__global__ __launch_bounds__(256) void post_scale_cas_kernel(PostScaleParams p, int antiring, int cas)
{
    post_scale_tile<T, PQ, AR, true>(p, antiring, cas);
}

template <typename T, bool PQ>
void launch(const PostScaleParams &p, int antiring, int cas, dim3 g, hipStream_t s)
{
    if (antiring) hipLaunchKernelGGL((post_scale_cas_kernel<T, PQ, true>), g, dim3(256), 0, s, p, antiring, cas);
    else hipLaunchKernelGGL((post_scale_cas_kernel<T, PQ, false>), g, dim3(256), 0, s, p, 0, cas);
}

}  // namespace

// cas 1032 .. 4096, antiring 0 .. 256 (0: the plain passes); otherwise post_scale_launch's conditions.
hipError_t post_scale_cas_launch(const PostScaleParams &p, int antiring, int cas, int is_f32, int pq, hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || (pq && !p.pq_bnd) || antiring < 0 || antiring > 256 || cas < 1032 || cas > 4096)
        return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH);
    if (is_f32) {
        if (pq) launch<float, true>(p, antiring, cas, g, s);
        else launch<float, false>(p, antiring, cas, g, s);
    } else {
        if (pq) launch<f16, true>(p, antiring, cas, g, s);
        else launch<f16, false>(p, antiring, cas, g, s);
    }
    return hipGetLastError();
}
