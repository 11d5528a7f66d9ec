// post_fsr_body.h -- the body of the fused quantise + FSR upscale kernel (gfx950), included INSIDE the __global__ function of
// post_fsr.hip (GRAIN = false) and of post_fsr_grain.hip (GRAIN = true): the tile's text exists once, and post_fsr.hip's kernels
// stay the functions they were (a shared __device__ function is inlined to other code).  No include guard on purpose.
// It expects, in scope: the template arguments T, PQ, RCAS; the kernel arguments p (PostFsrParams) and sharp =
// float32(2^-sharpness) (read only where RCAS); constexpr bool GRAIN, and intensity, seed -- the film grain's (read only where
// GRAIN: the final code of output pixel (dx + j, dy) is grained at that position over dH x dW, behind EASU and RCAS as in the
// reference's chain; film_grain.h).  post_fsr.hip's header describes the stages.
    constexpr int RG = RCAS ? 1 : 0;                                         // the ring of EASU pixels RCAS reads around the tile
    constexpr int SR = PS_TH + 2 * RG + 3, SC = PS_TW + 2 * RG + 3, SCP = SC + 1;
    __shared__ uint16_t codes[3][SR][SCP];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PS_TW, y0 = blockIdx.y * PS_TH;
    const int xa = max(x0 - RG, 0), xb = min(x0 + PS_TW - 1 + RG, p.dW - 1);
    const int ya = max(y0 - RG, 0), yb = min(y0 + PS_TH - 1 + RG, p.dH - 1);
    const int xs0 = p.xtab[xa].x - 1, ys0 = p.ytab[ya].x - 1;
    const int nc = min(p.xtab[xb].x + 3 - xs0, SC), nr = min(p.ytab[yb].x + 3 - ys0, SR);

    // 1. stage + quantise
    {
        const T *__restrict__ in = static_cast<const T *>(p.in);
        const size_t plane = (size_t)p.H * p.W;
        for (int i = tid; i < nr * nc; i += 256) {
            const int r = i / nc, c = i - r * nc;
            const int sy = min(max(ys0 + r, 0), p.H - 1), sx = min(max(xs0 + c, 0), p.W - 1);
            const size_t o = (size_t)sy * p.W + sx;
            const float cr = (float)in[o], cg = (float)in[plane + o], cb = (float)in[2 * plane + o];
            uint32_t q0, q1, q2;
            quant_rgb<PQ>(cr, cg, cb, p.peak, p.pq_bnd, q0, q1, q2);
            codes[0][r][c] = (uint16_t)q0;
            codes[1][r][c] = (uint16_t)q1;
            codes[2][r][c] = (uint16_t)q2;
        }
    }
    __syncthreads();

    if constexpr (RCAS) {
        // 2. EASU of the tile and its ring, row-major: ring pixel (ry, rx) is output pixel clamp(y0 - 1 + ry), clamp(x0 - 1 + rx)
        constexpr int ER = PS_TH + 2, EC = PS_TW + 2;
        __shared__ float easu[3][ER][EC];
        const int ery = min(PS_TH, p.dH - y0) + 2, erx = min(PS_TW, p.dW - x0) + 2;
#pragma unroll 1
        for (int i = tid; i < ery * erx; i += 256) {
            const int ry = i / erx, rx = i - ry * erx;
            const int2 yt = p.ytab[min(max(y0 - 1 + ry, 0), p.dH - 1)], xt = p.xtab[min(max(x0 - 1 + rx, 0), p.dW - 1)];
            float v[3];
            fsr_easu<SCP, SR * SCP>(&codes[0][yt.x - 1 - ys0][xt.x - 1 - xs0], __int_as_float(xt.y), __int_as_float(yt.y), v);
            easu[0][ry][rx] = v[0];
            easu[1][ry][rx] = v[1];
            easu[2][ry][rx] = v[2];
        }
        __syncthreads();

        // 3. RCAS + store: lane = four pixels (tid & 15) of output row (tid >> 4) and of the row 16 below
#pragma unroll 1
        for (int pass = 0; pass < PS_TH / 16; ++pass) {
            const int g = tid & 15, ly = (tid >> 4) + 16 * pass;
            const int dy = y0 + ly, dx = x0 + 4 * g;
            if (dy >= p.dH || dx >= p.dW) continue;
            uint64_t o[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ry = ly + 1, rx = 4 * g + j + 1;
                float b[3], d[3], e[3], f[3], h[3], v[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    b[ch] = easu[ch][ry - 1][rx];
                    d[ch] = easu[ch][ry][rx - 1];
                    e[ch] = easu[ch][ry][rx];
                    f[ch] = easu[ch][ry][rx + 1];
                    h[ch] = easu[ch][ry + 1][rx];
                }
                fsr_rcas(b, d, e, f, h, sharp, v);
                [[maybe_unused]] float Ig = 0.f;
                if constexpr (GRAIN) Ig = grain_term(intensity, dx + j, dy, p.dW, p.dH, seed);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    uint32_t code = quant_u16(v[ch]);
                    if constexpr (GRAIN) code = grain_code(code, Ig);
                    o[ch] |= (uint64_t)code << (16 * j);
                }
            }
            fsr_store(p, dy, dx, o);
        }
    } else {
        // 2. EASU + store: lane = four pixels (tid & 15) of output row (tid >> 4) and of the row 16 below, one after the other
#pragma unroll 1
        for (int pass = 0; pass < PS_TH / 16; ++pass) {
            const int g = tid & 15, dy = y0 + (tid >> 4) + 16 * pass, dx = x0 + 4 * g;
            if (dy >= p.dH || dx >= p.dW) continue;
            const int2 yt = p.ytab[dy];
            uint64_t o[3] = {0, 0, 0};
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int2 xt = p.xtab[min(dx + j, p.dW - 1)];
                float v[3];
                fsr_easu<SCP, SR * SCP>(&codes[0][yt.x - 1 - ys0][xt.x - 1 - xs0], __int_as_float(xt.y), __int_as_float(yt.y), v);
                [[maybe_unused]] float Ig = 0.f;
                if constexpr (GRAIN) Ig = grain_term(intensity, dx + j, dy, p.dW, p.dH, seed);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    uint32_t code = quant_u16(v[ch]);
                    if constexpr (GRAIN) code = grain_code(code, Ig);
                    o[ch] |= (uint64_t)code << (16 * j);
                }
            }
            fsr_store(p, dy, dx, o);
        }
    }
