// post_scale_grain.hip -- hdrtv_post_rgb48_scaled_grain with a nonzero intensity (gfx950): the kernels of post_scale.hip,
// post_scale_ar.hip and post_scale_cas.hip -- the same 32 x 64 tile, staging, passes and stores (post_scale_tile.h) -- with the film
// grain (film_grain.h; include/hdrtv_mi355x.h states the rule) applied to the staged codes, sharpened where CAS is on, before the
// passes read them: the reference's chain orders cas (an ffmpeg filter), the grain shader (MAIN at the processing size) and mpv's
// scaler that way.  The grain of a staged code is that of the clamped frame pixel it was read from, so a tap outside the frame reads
// the grained edge pixel.  The instances -- anti-ringing x CAS x PQ x {f16, f32} -- live in a file of their own so that the three
// files above keep their kernels and their code: an intensity of 0 launches those, never these.  The file is built with
// -ffp-contract=off (the rule is float32 operation by operation); the passes are integer arithmetic and do not notice.
// Strength, CAS code, intensity and seed are kernel arguments beside PostScaleParams, uniform over the launch (SGPRs).
#include "launchers.h"
#include "post_scale_tile.h"

namespace {

template <typename T, bool PQ, bool AR, bool CAS>
__global__ __launch_bounds__(256) void post_scale_grain_kernel(PostScaleParams p, int antiring, int cas, float intensity, float seed)
{
    post_scale_tile<T, PQ, AR, CAS, true>(p, antiring, cas, intensity, seed);
}

template <typename T, bool PQ>
void launch(const PostScaleParams &p, int antiring, int cas, float intensity, float seed, dim3 g, hipStream_t s)
{
    const dim3 b(256);
    if (cas) {
        if (antiring) hipLaunchKernelGGL((post_scale_grain_kernel<T, PQ, true, true>), g, b, 0, s, p, antiring, cas, intensity, seed);
        else hipLaunchKernelGGL((post_scale_grain_kernel<T, PQ, false, true>), g, b, 0, s, p, 0, cas, intensity, seed);
    } else {
        if (antiring) hipLaunchKernelGGL((post_scale_grain_kernel<T, PQ, true, false>), g, b, 0, s, p, antiring, 0, intensity, seed);
        else hipLaunchKernelGGL((post_scale_grain_kernel<T, PQ, false, false>), g, b, 0, s, p, 0, 0, intensity, seed);
    }
}

}  // namespace

// antiring 0 .. 256, cas 0 or 1032 .. 4096, 0 < intensity <= 0.1, 0 <= seed < 1; otherwise post_scale_launch's conditions.
hipError_t post_scale_grain_launch(const PostScaleParams &p, int antiring, int cas, float intensity, float seed, int is_f32, int pq,
                                   hipStream_t s)
{
    if (p.H < 1 || p.W < 1 || p.dH < p.H || p.dW < p.W || (pq && !p.pq_bnd) || antiring < 0 || antiring > 256 ||
        (cas != 0 && (cas < 1032 || cas > 4096)) || !(intensity > 0.f && intensity <= 0.1f) || !(seed >= 0.f && seed < 1.f))
        return hipErrorInvalidValue;
    const dim3 g((p.dW + PS_TW - 1) / PS_TW, (p.dH + PS_TH - 1) / PS_TH);
    if (is_f32) {
        if (pq) launch<float, true>(p, antiring, cas, intensity, seed, g, s);
        else launch<float, false>(p, antiring, cas, intensity, seed, g, s);
    } else {
        if (pq) launch<f16, true>(p, antiring, cas, intensity, seed, g, s);
        else launch<f16, false>(p, antiring, cas, intensity, seed, g, s);
    }
    return hipGetLastError();
}
