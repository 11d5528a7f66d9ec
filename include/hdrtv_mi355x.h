/*
 * hdrtv_mi355x.h -- C ABI of libhdrtv_mi355x.so: the MI355X-native (gfx950) SDR->HDR
 * per-frame inference path of HDRTVNet++ (AGCM -> LE -> HG) with its pre/post stages.
 *
 * The reference (DanHelmy/hdr-realtime-video-pipeline) has no FFI: its AMD backend is the
 * Python class HDRTVNetTorch (src/models/hdrtvnet_torch.py:1513).  Each entry point below
 * names the reference method/lines it replaces; the Python mirror that binds them is
 * hdr-realtime-video-pipeline_amd/hdrtv_mi355x/processor.py.
 *
 * Conventions: plain pointers and sizes only.  Every "dev" pointer is device memory
 * (hipMalloc / torch CUDA tensor .data_ptr()); `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  All calls are stream-ordered and never synchronise, except
 * hdrtv_create / hdrtv_reserve / hdrtv_destroy and the hdrtv_ring_* host-side calls.
 * Return 0 on success, a negative HDRTV_E* code otherwise; hdrtv_last_error() describes it.
 * Not re-entrant per context (like the reference: one processor per worker thread).
 */
#ifndef HDRTV_MI355X_H
#define HDRTV_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDRTV_OK 0
#define HDRTV_EINVAL (-1)   /* bad argument / shape                      */
#define HDRTV_EWEIGHTS (-2) /* weight pack malformed or tensor missing   */
#define HDRTV_EHIP (-3)     /* a HIP runtime call failed                 */
#define HDRTV_ENOMEM (-4)
#define HDRTV_ESTATE (-5)   /* call order (e.g. infer before reserve)    */

typedef struct hdrtv_ctx hdrtv_ctx;

/* Output element type of hdrtv_infer's `out` and input type of the post kernels. */
#define HDRTV_F16 0
#define HDRTV_F32 1

/* Library / build info: "hdrtv_mi355x <ver> gfx950 ...".  Never NULL. */
const char *hdrtv_version(void);

/* Replaces HDRTVNetTorch.__init__/_load_model (hdrtvnet_torch.py:1532-1673, 2044-2169).
 * hr_pack: HDRW1 weight pack (hdrtv_mi355x/weights.py) holding the 264 AGCM+LE tensors of
 * HR.pt under their state_dict names.  hg_pack: HDRW1 pack of Hallucination_Generator's
 * state_dict (conv*.0.*, conv*.1.* BatchNorm, Up_conv*.0.*, conv6..conv10, conv_last) or
 * NULL/0 for the no-HG model (reference: use_hg=False).  Weights are repacked on the host
 * into MFMA operand layouts and uploaded to `device_id`. */
int hdrtv_create(const void *hr_pack, size_t hr_bytes, const void *hg_pack, size_t hg_bytes,
                 int device_id, hdrtv_ctx **out);

/* The same with the compute precision of HDRTVNetTorch(precision=...) (hdrtvnet_torch.py:1694-1712).
 * HDRTV_PREC_F16 (= hdrtv_create): f16 storage / fp32 accumulate on the MFMA kernels; tensors at the boundary are f16
 * (the HG head's output f32).  HDRTV_PREC_F32: the reference's fp32 preset -- the same graph on planar fp32 tensors with
 * vector-FMA kernels (csrc/fp32_ops.hip; no matrix path exists for fp32 on gfx950, so roughly 1/30 of the f16 frame rate):
 * hdrtv_preprocess writes f32 `rgb` / `cond`, hdrtv_infer takes them and writes f32 `out` / `agcm_out` (out_dtype must
 * be HDRTV_F32), the post kernels take dtype HDRTV_F32.  An INT8 checkpoint is refused (HDRTV_EWEIGHTS). */
#define HDRTV_PREC_F16 0
#define HDRTV_PREC_F32 1
int hdrtv_create_ex(const void *hr_pack, size_t hr_bytes, const void *hg_pack, size_t hg_bytes,
                    int device_id, int precision, hdrtv_ctx **out);
int hdrtv_destroy(hdrtv_ctx *ctx);

/* 1 if the context was created with HG weights. */
int hdrtv_has_hg(const hdrtv_ctx *ctx);

/* How hdrtv_preprocess derives the 0.25x condition map (hdrtvnet_torch.py:2262-2294): 0 = antialiased bicubic (default),
 * 1 = bilinear, the reference's fast_condition_resize=True / HDRTVNET_FAST_COND_RESIZE, 2 = zeros, HDRTVNET_ZERO_COND. */
int hdrtv_set_cond_mode(hdrtv_ctx *ctx, int mode);

/* HG_Composite(mask_r=0.75) (HG_Composite_arch.py:21, 78-84): the highlight mask is max_c(base) > r + 0.1 * (1 - r).
 * The reference fixes r at construction; 0 <= r < 1.  Takes effect at the next hdrtv_infer. */
int hdrtv_set_hg_mask_r(hdrtv_ctx *ctx, float r);

/* Replaces HDRTVNetTorch._ensure_buffers (hdrtvnet_torch.py:2198-2233): (re)allocates the
 * internal activation workspace for H x W frames.  No-op when the size is unchanged.
 * Synchronises the device when it reallocates. */
int hdrtv_reserve(hdrtv_ctx *ctx, int H, int W);

/* Replaces the device half of HDRTVNetTorch.preprocess (hdrtvnet_torch.py:2255-2294).
 * dev_bgr_hwc : u8  [H][W][3] BGR (the frame after the pinned H2D copy)
 * dev_rgb_chw : f16 [3][H][W]     RGB, fp16(float(u8) * fp32(1/255))
 * dev_cond    : f16 [3][H/4][W/4] 0.25x antialiased bicubic (a=-0.5), fp32 accumulate */
int hdrtv_preprocess(hdrtv_ctx *ctx, void *stream, const uint8_t *dev_bgr_hwc, int H, int W,
                     void *dev_rgb_chw, void *dev_cond);

/* Replaces HDRTVNetTorch.infer -> model((tensor, cond)) (hdrtvnet_torch.py:2301-2346;
 * Ensemble_AGCM_LE_arch.py:889-897, HG_Composite_arch.py:86-107).
 * dev_rgb_chw, dev_cond: as produced by hdrtv_preprocess.
 * dev_out      : [3][H][W] planar RGB; out_dtype HDRTV_F16 without HG.  With HG the reference's
 *                result is fp32 (the fp32 highlight mask promotes it): pass HDRTV_F32, or
 *                HDRTV_F16 to have it rounded once at the end.
 * dev_agcm_out : f16 [3][H][W], second element of the reference's result tuple; may be NULL. */
int hdrtv_infer(hdrtv_ctx *ctx, void *stream, const void *dev_rgb_chw, const void *dev_cond, int H,
                int W, void *dev_out, int out_dtype, void *dev_agcm_out);

/* Frames in flight (no reference counterpart: the reference's worker processes one frame at a time and hides its copies
 * behind streams, gui_pipeline_worker_feeders.py:125-249).  A context holds `lanes` activation workspaces (1 or 2, default
 * 1; weights are shared); hdrtv_infer_lane(ctx, l, stream_l, ...) is hdrtv_infer on workspace l, so calls with different
 * lanes on different streams may overlap on the device: the tail of one frame's kernel fills with the next frame's
 * workgroups (+3 .. 4.5 % frames/s at 3840x2160 with two lanes, +11 % at 1920x1080; a frame's own latency doubles).
 * Results do not depend on the lane (tests/test_gpu_lanes.py).  HDRTV_EINVAL for more than two lanes (three kernels running
 * at once is where rare wrong tiles were seen) and for two on an fp32 context.  hdrtv_set_lanes drops the
 * reservation when the count changes (call hdrtv_reserve again; it synchronises the device); hdrtv_infer is lane 0.  Calls on one context are made by one host thread at a time,
 * as before: lanes make the DEVICE work concurrent, not the entry points re-entrant.  hdrtv_get_tap addresses lane 0. */
int hdrtv_set_lanes(hdrtv_ctx *ctx, int lanes);
int hdrtv_get_lanes(const hdrtv_ctx *ctx);
int hdrtv_infer_lane(hdrtv_ctx *ctx, int lane, void *stream, const void *dev_rgb_chw, const void *dev_cond, int H,
                     int W, void *dev_out, int out_dtype, void *dev_agcm_out);

/* Replaces HDRTVNetTorch.postprocess's device half (hdrtvnet_torch.py:2357-2361):
 * trunc(clamp(x,0,1)*255 + 0.5) in the tensor's dtype semantics, RGB planar -> u8 [H][W][3] BGR. */
int hdrtv_post_u8(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W,
                  uint8_t *dev_bgr_hwc);

/* Replaces _tensor_to_rgb48_bytes' GPU branch (gui_pipeline_worker_feeders.py:223-227):
 * fp32(x) -> clamp(0,1) -> *65535 -> +0.5 (two fp32 roundings) -> trunc u16, planar ->
 * [H][W][3] RGB little-endian (mpv "rgb48le").  dst is device memory (e.g. a ring slot's dev_ptr;
 * hdrtv_ring_commit then moves it to the slot's pinned host buffer as the reference's host.copy_ does, :228). */
int hdrtv_post_rgb48(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W,
                     uint16_t *dst);

/* North-star display variant with no counterpart on the reference's playback path
 * (SURVEY.md 8a-14/15): treats x as linear-light BT.709 with 1.0 = peak_nits, applies the
 * BT.709->BT.2020 matrix (ITU-R BT.2087), the ST.2084 PQ OETF
 * (gui_objective_metrics.py:486-491 constants) and the u16 quantiser, same output layout. */
int hdrtv_post_pq_rgb48(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W,
                        float peak_nits, uint16_t *dst);

/* RGB48 at the display size: hdrtv_post_rgb48 (pq = 0; peak_nits ignored) or hdrtv_post_pq_rgb48 (pq != 0) and a Lanczos-3
 * upscale of its codes to [dH][dW][3], in one kernel without a frame-sized intermediate.  The reference's "lower-resolution
 * processing" mode leaves this resize to mpv's scalers (gui_scaling.py:13-15, 42-43, 67-162) or, on its CPU path, to
 * cv2.resize(INTER_LANCZOS4) (gui_pipeline_worker_frame_processing.py:100-116); a headless sink has neither in front of it.
 * Parity with mpv's or OpenCV's scalers is UNPINNED (neither is part of the reference tree, and their float paths are not
 * reproducible); the resampling is this integer rule, restated in tests/rgb48_scale_ref.py, which the GPU tests hold this entry
 * point to bit for bit.  Enlarging only (dH >= H, dW >= W); the whole frame maps onto the whole output (black bars of a
 * letterboxed input are scaled with it), the axes are independent, aspect is the caller's business.  Anti-ringing is
 * hdrtv_post_rgb48_scaled_ex's (below); no shrinking, no crop rectangle.
 *  1. codes: s[c][y][x] = the u16 code hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 writes for that source value; the resampling sees
 *     nothing but these integers.
 *  2. per axis, source extent n, destination extent m, for d = 0..m-1, in double:
 *       c = (d + 0.5) * n / m - 0.5;  i0 = floor(c);  t = c - i0;  six taps k = -2..3 at source index clamp(i0 + k, 0, n-1)
 *       w_k = L(t - k), L(x) = sinc(x) * sinc(x/3) for |x| < 3, else 0, sinc(x) = sin(pi x)/(pi x), L(0) = 1;  w_k /= sum(w)
 *       q_k = floor(w_k * 16384 + 0.5);  then 16384 - sum(q) is added to the largest q_k (the lowest k on a tie): sum(q) = 16384.
 *     m == n gives q = {0, 0, 16384, 0, 0, 0}; exact 2x has the two phases {121, -1114, 4440, 14628, -2184, 493} (first tap
 *     i0 - 2 = -3 at d = 0) and its mirror image.
 *  3. two passes: hor[y][dx] = sum_k s[y][.] * qx_k (exact in int32: sum |q| <= 25290);
 *     out = clamp((sum_k hor[.][dx] * qy_k + 2^27) >> 28, 0, 65535) with a flooring shift (the sum needs 46 bits).
 * With dH == H and dW == W the bytes equal the unscaled entry point's.  Stream-ordered, needs no reservation; the tap tables are
 * built on the host in double at the first call with a geometry (H, W, dH, dW) -- that call allocates and copies -- and kept in the
 * context, so later calls only launch.  HDRTV_EINVAL for a NULL pointer, a non-positive size, dH < H or dW < W, an unknown dtype,
 * or pq with peak_nits <= 0; dst is not touched then. */
int hdrtv_post_rgb48_scaled(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W,
                            int pq, float peak_nits, uint16_t *dst, int dH, int dW);

/* hdrtv_post_rgb48_scaled with anti-ringing of strength antiring / 256, antiring = 0..256 (256 = full strength).  Lanczos overshoots
 * at a hard edge; on PQ codes the halo of a 0.25 / 0.75 step reaches 3382 codes (5.2 % of the range) and enters everything
 * behind the scaler (the Y'CbCr conversion, deband, the content light level record).  The reference never shows an upscaled HDR
 * frame without it: in its lower-resolution processing mode it sets mpv's scale-antiring from the processing size
 * (_select_hdr_scale_antiring, gui_scaling.py:82-111).  Modelled on that separable form -- each pass is clamped to the two samples
 * that bracket the sampling position and blended by the strength -- but mpv is not part of the reference tree: parity with it is
 * UNPINNED, and the device is held to this integer rule, restated in tests/rgb48_antiring_ref.py, bit for bit.  Codes, tables and
 * taps are steps 1 and 2 of hdrtv_post_rgb48_scaled; with a = antiring, tap_k the source index clamp(i0 - 2 + k), k = 0..5:
 *  3a. horizontal, per source row y, channel and dx:
 *        raw = sum_k s[y][tap_k] * qx_k                               (int32, as in step 3)
 *        lo  = min(s[y][tap_2], s[y][tap_3]) << 14;   hi = max(s[y][tap_2], s[y][tap_3]) << 14
 *        d   = clamp(raw, lo, hi) - raw
 *        hor[y][dx] = raw + ((d * a + 128) >> 8)                      (flooring shift; d * a needs 64 bits; |hor| < 2^31)
 *  3b. vertical, taps at rows tap_k = clamp(j0 - 2 + k) of hor:
 *        raw = sum_k hor[tap_k][dx] * qy_k                            (int64)
 *        lo  = min(hor[tap_2][dx], hor[tap_3][dx]) << 14;   hi = max(hor[tap_2][dx], hor[tap_3][dx]) << 14
 *        d   = clamp(raw, lo, hi) - raw
 *        v   = raw + ((d * a + 128) >> 8)
 *        out = clamp((v + 2^27) >> 28, 0, 65535)
 * a = 0 is hdrtv_post_rgb48_scaled exactly: the same launches (the delegation to the unscaled kernel at dH == H && dW == W
 * included) and the same bytes.  An axis with m == n is untouched by any a (raw = the inner tap << 14 lies in [lo, hi]), so with a
 * nonzero strength equal sizes delegate too.  a = 256 puts every output inside the min / max of the 2 x 2 source codes around it.
 * A strength s in [0, 1] maps to a = floor(s * 256 + 0.5).  Shares the tap tables of hdrtv_post_rgb48_scaled; HDRTV_EINVAL for
 * antiring outside 0..256 and for everything hdrtv_post_rgb48_scaled refuses; dst is not touched then. */
int hdrtv_post_rgb48_scaled_ex(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W,
                               int pq, float peak_nits, uint16_t *dst, int dH, int dW, int antiring);

/* hdrtv_post_rgb48_scaled_ex with contrast-adaptive sharpening of the codes in front of the scaler.  For any upscale that does not go
 * through its FSR shader the reference appends cas=<strength> to the video filter chain of its HDR frames
 * (_select_mpv_cas_strength, gui_scaling.py:114-138; 0.22 / 0.20 / 0.16 by processing size): FidelityFX CAS as ffmpeg's cas filter,
 * in vf, so on the PQ-coded RGB48 frame at the processing size, before the display scaler and its anti-ringing.  A headless sink
 * has no such chain in front of it.  ffmpeg is not part of the reference tree: parity with its float filter is UNPINNED, and the
 * device is held to this integer rule, restated in tests/rgb48_cas_ref.py, bit for bit.  cas = 0 is off; otherwise cas = K, the
 * CAS code 1032..4096; a strength s in (0, 1] maps to K = 4096 - ((c * 3064 + 128) >> 8) with c = floor(s * 256 + 0.5), 1032..4084
 * (K / 256 = ffmpeg's lerp(16, 4.03, s); 0.22 -> 3426, 0.20 -> 3486, 0.16 -> 3605).
 *  1s. between steps 1 and 2 of hdrtv_post_rgb48_scaled, per channel, on the u16 codes s of the FRAME: for e = s[y][x] with the
 *      3 x 3 neighbourhood a b c / d e f / g h i, the frame's edge pixels repeated (row y - 1 is row max(y - 1, 0), ...):
 *        mn  = min(b,d,e,f,h) + min(a..i);   mx = max(b,d,e,f,h) + max(a..i)
 *        q   = min(mn, 131070 - mx)                                   (0 <= q <= mx)
 *        r   = floor((q << 15) / mx), 0 for mx = 0                    (r <= 32768; q << 15 < 2^32)
 *        A   = floor(sqrt(r << 9))                                    (0..4096: the amplitude in Q12)
 *        den = 16 * K - 4 * A                                         (> 0, as K >= 1032)
 *        t   = 4 * e - (b + d + f + h)
 *        s'[y][x] = clamp(e + floor((A * t + (den >> 1)) / den), 0, 65535)     (floor towards minus infinity; |A * t| < 2^30)
 *      This is ffmpeg's (e + w * (b+d+f+h)) / (1 + 4w), w = -amp / lerp(16, 4.03, s), amp = sqrt(clip(min(mn, 2*max - mx) / mx, 0, 1)),
 *      written as e + A * t / den.  A flat neighbourhood returns e.
 *  Steps 2, 3 / 3a, 3b then run on s': a tap outside the frame reads the SHARPENED edge pixel (whose neighbourhood was clamped from
 *  the edge pixel), and anti-ringing of strength antiring acts on the sharpened codes, as in the reference's chain.
 * cas = 0 is hdrtv_post_rgb48_scaled_ex exactly: the same launches and the same bytes.  Equal sizes (dH == H && dW == W) delegate to
 * the unscaled kernel and are NOT sharpened, whatever cas: the reference sharpens only when it upscales.  With one axis at identity
 * the filter applies in full (it is two-dimensional on the source).  Shares the tap tables; the LDS of the plain form.
 * HDRTV_EINVAL for a cas that is neither 0 nor in 1032..4096 and for everything hdrtv_post_rgb48_scaled_ex refuses, before any
 * device call; dst is not touched then. */
int hdrtv_post_rgb48_scaled_cas(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W,
                                int pq, float peak_nits, uint16_t *dst, int dH, int dW, int antiring, int cas);

/* RGB48 at the display size through FSR, the reference's DEFAULT upscaler (UPSCALER_CHOICES / DEFAULT_UPSCALER = "FSR",
 * gui_scaling.py:42-43): hdrtv_post_rgb48 (pq = 0; peak_nits ignored) or hdrtv_post_pq_rgb48 (pq != 0), then EASU and, with
 * rcas = 1, RCAS, in one kernel without a frame-sized intermediate.  For this branch the reference selects cas = 0 and
 * scale-antiring = 0 and lets its shader do the whole enlargement: assets/shaders/FSR.glsl, FidelityFX FSR 1.0.2 on RGB (EASU
 * de-ringing on, full analysis, no early exit; RCAS with sharpness 0.20 and the denoise term).  Unlike mpv's Lanczos or ffmpeg's cas
 * that arithmetic IS part of the reference tree, so this rule is the shader's, operation by operation, in float32: every multiply,
 * add, subtract and divide is rounded on its own (no fused multiply-add), divisions are correctly rounded, denormals are kept.
 * tests/rgb48_fsr_ref.py restates it in NumPy and the GPU tests hold this entry point to it bit for bit.  What the GLSL compiler of
 * a display makes of the shader (fused operations, approximate divisions) is UNPINNED.
 *  1. codes: c = exactly what hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 writes at the processing size; the rule sees only these integers.
 *  2. samples: s = float32(c) / float32(65535), one correctly rounded division (a unorm16 texture fetch); indices outside the frame
 *     read the clamped pixel.
 *  3. positions, per axis, source extent n, destination extent m, for d = 0..m-1, in double on the host:
 *       p = (d + 0.5) * n / m - 0.5;  fp[d] = floor(p) (int32);  pp[d] = float32(p - fp[d])
 *     exact 2x gives pp = 0.75, 0.25, 0.75, ... with fp[0] = -1; m == n gives pp = 0, fp[d] = d.
 *  4. EASU, per output pixel with (fx, fy) = fp and (ppx, ppy) = pp of its column and row.  Twelve taps b c / e f g h / i j k l / n o
 *     at (fx, fy) + (0,-1) (1,-1) / (-1,0) (0,0) (1,0) (2,0) / (-1,1) (0,1) (1,1) (2,1) / (0,2) (1,2); luma L = (0.2126 r + 0.7152 g)
 *     + 0.0722 b.  rcp~(a) = the float32 whose bits are 0x7ef07ebb - bits(a), rsq~(a) = bits 0x5f347d74 - (bits(a) >> 1), on the u32
 *     pattern; sat(x) = min(max(x, 0), 1).  dir = (0, 0), len = 0, then four analyses with the bilinear weights
 *     w = (1-ppx)(1-ppy), ppx (1-ppy), (1-ppx) ppy, ppx ppy on the luma crosses (A / B C D / E) = (b / e f g / j), (c / f g h / k),
 *     (f / i j k / n), (g / j k l / o):
 *       dirX = D - B;  lenX = sat(|dirX| * rcp~(max(|D - C|, |C - B|)));  lenX = lenX * lenX;  Y alike with E - A, E - C, C - A
 *       dir = dir + (dirX, dirY) * w;  len = len + ((w * lenX) + (w * lenY))
 *     then  dirR = dir.x dir.x + dir.y dir.y;  zro = dirR < 1 / 32768;  dirR = zro ? 1 : rsq~(dirR);  dir.x = zro ? 1 : dir.x;
 *       dir = dir * dirR;  len = len * 0.5;  len = len * len
 *       stretch = (dir.x dir.x + dir.y dir.y) * rcp~(max(|dir.x|, |dir.y|))
 *       len2 = (1 + (stretch - 1) * len, 1 + (-0.5) * len);  lob = 0.5 + float32((0.25 - 0.04) - 0.5) * len;  clp = rcp~(lob)
 *     and the taps accumulate in the order b c i j f e k l h g o n, for a tap at offset (ox, oy) with colour c:
 *       off = (ox - ppx, oy - ppy);  v = ((off.x dir.x + off.y dir.y) * len2.x, (off.x * -dir.y + off.y dir.x) * len2.y)
 *       d2 = min(v.x v.x + v.y v.y, clp);  wB = float32(2/5) d2 + (-1);  wA = lob d2 + (-1);  wB = wB wB;  wA = wA wA
 *       wB = (25/16) wB + (-(25/16 - 1));  w = wB * wA;  aC = aC + c * w;  aW = aW + w
 *     pix = aC / aW (correctly rounded), clamped to the min / max of f g j k per channel, then sat.  A flat frame returns its code.
 *  5. RCAS (rcas = 1), on the float32 EASU image at the output size, no quantisation in between; neighbours b d f h at (0,-1) (-1,0)
 *     (1,0) (0,1), clamped to the image; per channel, mn / mx = min / max of b d f h, eps = float32(1e-6):
 *       hitMin = min(mn, e) / max(4 mx, eps);  hitMax = (1 - max(mx, e)) / min(4 mn - 4, -eps)
 *       lobe = max(-(0.25 - 1/16), min(max(-hitMin, hitMax), 0)) * float32(2^-sharpness)      (the factor in double on the host)
 *       nz = |0.25 * (((b + d) + f) + h) - e| / max(max(mx, e) - min(mn, e), eps)
 *     lobe = lobe * (-0.5 * sat(max over the three channels of nz) + 1);  rcp = 1 / (4 lobe + 1) (correctly rounded)
 *     pix = sat(((((lobe b + lobe d) + lobe h) + lobe f) + e) * rcp)
 *  6. output code: (int)(x * 65535 + 0.5), the quantiser of the unscaled entry point, both operations float32.
 * Sizes: H <= dH <= 2H and W <= dW <= 2W.  The shader's EASU stage scales to min(OUTPUT, 2 * MAIN) per axis and leaves the rest to
 * mpv's scaler; that residual pass is not part of this entry point, and a larger ratio is refused.  The reference's headline case,
 * 1080p -> 2160p, is exactly 2x.  Equal sizes (dH == H && dW == W) delegate to the unscaled kernel and write its bytes, whatever rcas
 * (the shader runs only when the output area is larger); with one axis at identity the filter applies in full.  rcas is 0 (EASU
 * alone, sharpness ignored) or 1; sharpness is in [0, 2], 0 the sharpest, the reference's value 0.20.  Stream-ordered, needs no
 * reservation; the position tables are built at the first call with a geometry -- that call allocates and copies -- and kept in the
 * context beside the tap tables.  HDRTV_EINVAL, before any device call and with dst untouched, for everything
 * hdrtv_post_rgb48_scaled refuses, for dH > 2H or dW > 2W, for rcas outside {0, 1} and, with rcas = 1, for a sharpness that is NaN,
 * infinite or outside [0, 2]. */
int hdrtv_post_rgb48_fsr(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                         uint16_t *dst, int dH, int dW, int rcas, float sharpness);

/* RGB48 BELOW the processing size: hdrtv_post_rgb48 (pq = 0; peak_nits ignored) or hdrtv_post_pq_rgb48 (pq != 0), then the
 * reference's downscaling chain, in one kernel without a frame at the processing size in device memory.  For an output smaller than
 * the source the reference has a fixed, default-on path: dscale=mitchell, correct-downscaling=yes, linear-downscaling=no,
 * dscale-antiring=0.20 (_apply_presentation_scaler_defaults, gui_mpv_widget.py) and assets/shaders/SSimDownscaler.glsl first in
 * every shader chain (_build_shader_paths), whose passes run exactly when the output is smaller.  Stage A is mpv's part: mpv is not
 * in the reference tree, parity with its own Mitchell arithmetic is UNPINNED, and the device is held to the integer rule below.
 * Stage B (ssim = 1) is the shader's, which IS in the reference tree: its arithmetic in float32, operation by operation (every
 * multiply, add, subtract, divide and square root rounded on its own, no fused multiply-add, denormals kept); what a display's GLSL
 * compiler makes of the shader is UNPINNED.  tests/rgb48_down_ref.py restates both in NumPy and the GPU tests hold this entry
 * point to it bit for bit.
 *  1. codes: c = exactly what hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 writes at the processing size, [H][W][3]; the rule sees only
 *     these integers.  Indices outside the frame read the clamped pixel.
 *  2. footprint, per axis, source extent n, destination extent m, n / 4 <= m <= n, in double on the host for d = 0..m-1:
 *       ctr = (d + 0.5) * n / m;  hw = 2.0 * n / m;  k_lo = ceil(ctr - hw - 0.5);  k_hi = floor(ctr + hw - 0.5)
 *       tap k lies at x_k = (k + 0.5 - ctr) * m / n, in destination pixels;  k2 = floor(ctr - 0.5)
 *     The kernel is stretched by the ratio (correct-downscaling; also the low / high / rel of the shader's L2 passes): at most
 *     floor(4 n / m) + 1 <= 17 taps.  An axis with m == n is one tap, k = d, weight one, in stage A and stage B alike.
 *  3. stage A, Mitchell (B = C = 1/3) with w(x), x = |x_k|, in double:
 *       x < 1: ((7 x - 12) x x + 16/3) / 6;   x < 2: ((((-7/3) x + 12) x - 20) x + 32/3) / 6;   else 0
 *     summed in tap order to s; q_k = floor(w_k / s * 16384 + 0.5), the remainder 16384 - sum q to the largest coefficient (the
 *     lowest k on a tie).  With a = antiring and the shapes of hdrtv_post_rgb48_scaled_ex's steps 3a / 3b:
 *       horizontal, per source row y, channel and dx:  raw = sum_k c[y][clamp(k)] * qx_k   (int32)
 *         lo / hi = min / max(c[y][clamp(k2)], c[y][clamp(k2 + 1)]) << 14;  d = clamp(raw, lo, hi) - raw
 *         hor[y][dx] = raw + ((d * a + 128) >> 8)                           (flooring shift, 64 bits; |hor| < 2^31)
 *       vertical, on rows clamp(k) of hor:  raw = sum_k hor[clamp(k)][dx] * qy_k   (int64); lo / hi from hor[clamp(k2)],
 *         hor[clamp(k2 + 1)] likewise;  v = raw + ((d * a + 128) >> 8);  M = clamp((v + 2^27) >> 28, 0, 65535)
 *     M are the Mitchell codes; with ssim = 0 they are the output.  a = 0 is the plain passes, a = 256 puts every output inside the
 *     min / max of the 2 x 2 source codes that bracket it; the reference's 0.20 is a = floor(0.20 * 256 + 0.5) = 51.
 *  4. stage B, samples: s = float32(c) / float32(65535), Ms = float32(M) / float32(65535), one correctly rounded division each (the
 *     shader's POSTKERNEL is a 16-bit texture: the quantised Mitchell codes), so stage B is a pure function of (c, M).
 *  5. L2, the Catmull-Rom mean of squares on the footprint of step 2: weight cr(|x_k|) in double, cr(x) = (1.5 x - 2.5) x x + 1 for
 *     x < 1, else ((-0.5 x + 2.5) x - 4) x + 2, divided by the sum of the axis' weights (double, tap order), then rounded to float32
 *     (the shader's division by W folded into the table).  Pass 1, vertical, on s * s (one rounded multiply):
 *     acc = acc + wy_k * (s * s) for k ascending from acc = 0; pass 2, horizontal, on pass 1's float32 values, likewise.
 *  6. mean3(v), at the output size: taps -1, 0, 1 with the weights 0.5, 1, 0.5, neighbours clamped to the image; inside each row
 *     h = ((0.5 v[-1] + v[0]) + 0.5 v[1]) / 2, then over the rows ((0.5 h[-1] + h[0]) + 0.5 h[1]) / 2.
 *  7. MR: mM = mean3(Ms), mQ = mean3(Ms * Ms), mL = mean3(L2) per channel;  Sl = Luma(max(mQ - mM * mM, 0)),
 *     Sh = Luma(max(mL - mM * mM, 0)),  Luma = (0.2126 r + 0.7152 g) + 0.0722 b;  sigma = float32(10 / (255 * 255));
 *       R = Sl > Sh ? min(max(Sh / Sl, 0), 1) : sqrt((Sh + sigma) / (Sl + sigma))           (a select; oversharp = 0 drops out)
 *  8. final: a0 = mean3(R * mM), a1 = mean3(mM), a2 = mean3(R);  pix = sat((a1 + a2 * Ms) - a0);  the output code is
 *     (int)(pix * 65535 + 0.5), the quantiser of the unscaled entry point.  A flat frame returns its code: the sums are exact,
 *     Sl = Sh = 0, R = 1.
 * Sizes: H / 4 <= dH <= H and W / 4 <= dW <= W (4 dH >= H, 4 dW >= W).  Equal sizes (dH == H && dW == W) delegate to the unscaled
 * kernel and write its bytes, whatever the options; with one axis at identity both stages apply in full.  Out of scope: more than
 * 4x, one axis up and one down, linear-light downscaling (the reference sets linear-downscaling=no).  Stream-ordered, needs no
 * reservation; the tables are built at the first call with a geometry -- that call allocates and copies -- and kept in the context
 * beside the tap tables.  HDRTV_EINVAL, before any device call and with dst untouched, for a NULL pointer, an unknown dtype, H, W, dH
 * or dW < 1, pq with peak_nits <= 0, dH > H or dW > W, 4 dH < H or 4 dW < W, antiring outside 0..256, ssim outside {0, 1}. */
int hdrtv_post_rgb48_down(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                          uint16_t *dst, int dH, int dW, int antiring, int ssim);

/* RGB48 enlarged by the reference's third upscaler: hdrtv_post_rgb48 (pq = 0; peak_nits ignored) or hdrtv_post_pq_rgb48 (pq != 0),
 * then spline36 and the SSimSuperRes shader, in one kernel without a frame-sized intermediate in device memory.  For the choice
 * "SSimSuperRes" of UPSCALER_CHOICES (gui_scaling.py:42-43) the reference hands mpv scale=spline36 with scale-antiring = 0 and
 * cas = 0 (gui_mpv_widget.py:589-590, gui_scaling.py:101-102, 128-129) and appends assets/shaders/SSimSuperRes.glsl to the shader
 * chain (_build_shader_paths).  Stage A is mpv's part: mpv is not in the reference tree, parity with its own spline36 arithmetic is
 * UNPINNED, and the device is held to the integer rule below.  Stage B (ssim = 1) is the shader's, which IS in the reference tree:
 * its arithmetic in float32, operation by operation (every multiply, add, subtract, divide and square root rounded on its own, no
 * fused multiply-add, denormals kept).  UNPINNED there: the 16-bit float textures mpv keeps the shader's intermediates in (the rule
 * keeps float32), a texture unit's fixed-point filter weights, what a display's GLSL compiler makes of the shader.
 * tests/rgb48_ssimsr_ref.py restates both stages in NumPy and the GPU tests hold this entry point to it bit for bit.
 * Sq(v) = (0.2126 (r r) + 0.7152 (g g)) + 0.0722 (b b), each square one rounded multiply: the shader's Luma, which squares first.
 *  1. codes: c = exactly what hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 writes at the processing size, [H][W][3]; the rule sees only
 *     these integers.  Indices outside a frame read the clamped pixel, in every step below.
 *  2. stage A, spline36: steps 2 and 3 of hdrtv_post_rgb48_scaled with another kernel and no anti-ringing.  Six taps k = -2..3,
 *     c = (d + 0.5) n / m - 0.5, i0 = floor(c), t = c - i0, w_k = S(t - k) in double, summed in tap order to s,
 *     q_k = floor(w_k / s * 16384 + 0.5), the remainder to the largest q_k (the lowest k on a tie); the horizontal pass (int32), the
 *     vertical pass (int64), P = clamp((sum + 2^27) >> 28, 0, 65535).  S(x), x = |x|:
 *       x < 1: ((13/11 x - 453/209) x - 3/209) x + 1;   x < 2, y = x - 1: ((-6/11 y + 270/209) y - 156/209) y;
 *       x < 3, y = x - 2: ((1/11 y - 45/209) y + 26/209) y;   else 0
 *     P [dH][dW][3] are the spline36 codes; with ssim = 0 they are the output.
 *  3. samples: s = float32(c) / float32(65535), Ps = float32(P) / float32(65535), one correctly rounded division each (the shader's
 *     POSTKERNEL is taken as a 16-bit texture, as hdrtv_post_rgb48_down takes it), so stage B is a pure function of (c, P).
 *  4. low-resolution footprint, per axis with low extent n (H or W) and high extent m (dH or dW), in double for j = 0..n-1:
 *       ctr = (j + 0.5) m / n;  hw = 2 m / n;  k_lo = ceil(ctr - hw - 0.5);  k_hi = floor(ctr + hw - 0.5);  x_k = (k + 0.5 - ctr) n / m
 *     at most 9 taps, with the weight mn(|x_k|), B = 0.334, C = 0.333:
 *       x < 1: ((2 - 1.5 B - C) x + (-3 + 2 B + C)) x x + (1 - B / 3);   else (((-B / 6 - C) x + (B + 5 C)) x + (-2 B - 8 C)) x + (4/3 B + 4 C)
 *     summed in tap order, each divided by the sum in double, then rounded to float32 (the shader's division by W folded in).
 *  5. pass I, vertical, to [H][dW], k ascending from acc = 0, acc = acc + wy_k * v:  A.rgb = sum wy_k Ps[k][x],
 *     A.q = sum wy_k Sq(Ps[k][x]);  e1 = max(|A.q - Sq(A.rgb)|, float32(5e-7)).
 *  6. pass II, horizontal, on A.rgb, to [H][W]:  Lr.rgb = sum wx_k A.rgb[y][k],  q2 = sum wx_k Sq(A.rgb[y][k]),
 *     e2 = max(|q2 - Sq(Lr.rgb)|, 5e-7).  The linear fetch of pass I's fourth component at this pixel: u = (i + 0.5) dW / W - 0.5,
 *     b0 = floor(u), f = float32(u - b0) in double on the host;  e1i = ((1 - f) * e1[y][b0]) + (f * e1[y][b0 + 1]);  Lr.a = e2 + e1i.
 *  7. var, at [H][W], the cross neighbours in the order (x-1, y), (x+1, y), (x, y-1), (x, y+1):
 *       mL = ((((s0 + 0.25 s1) + 0.25 s2) + 0.25 s3) + 0.25 s4) / 2 per channel, mH the same on Lr.rgb;
 *       vL = max(((((Sq(s0 - mL) + 0.25 Sq(s1 - mL)) + 0.25 Sq(s2 - mL)) + 0.25 Sq(s3 - mL)) + 0.25 Sq(s4 - mL)) / 2, float32(1e-6)),
 *       vH likewise from Lr.rgb and mH.
 *  8. final, per output pixel.  Per axis, in double on the host: p = (d + 0.5) n / m - 0.5, ip = floor(p + 0.5) (GLSL's round leaves
 *     the tie open; the rule takes it up), off = p - ip, kern[d][t] = float32(cos(pi (t - off) / 3)) for t = -1, 0, 1 (the Hann
 *     window; no cosine is evaluated on the device).  c0 = Ps at the pixel.  With X outer and Y inner, both -1..1, w = 1, 0.5 for
 *     offset 0, +-1 and accumulation from 0:  mV = (sum (wX wY) * Lr.a[ip_y + Y][ip_x + X]) / 4.  Then, in the same order, at the
 *     low-resolution pixel g = (ip_y + Y, ip_x + X):
 *       R = -1.5 * sqrt(vL[g] / (vH[g] + mV))                                   (oversharp = 0.5)
 *       wt = (kx[X] * ky[Y]) / (Sq(c0 - Lr.rgb[g]) + Lr.a[g])
 *       term = (s[g] + Lr.rgb[g] * R) + ((-1 - R) * c0);   D = D + wt * term;   Ws = Ws + wt
 *     pix = sat(c0 + D / Ws); the output code is (int)(pix * 65535 + 0.5), the quantiser of the unscaled entry point.  Every
 *     denominator is positive: Lr.a >= 1e-6 (up to the roundings of the linear fetch), vH + mV >= 2e-6, the centre Hann weight at
 *     least cos^2(pi / 6).  A flat frame returns its code.
 * Sizes: equal sizes (dH == H && dW == W) delegate to the unscaled kernel and write its bytes, whatever ssim.  Otherwise both axes
 * are strictly enlarged, by at most 2x: H < dH <= 2 H and W < dW <= 2 W (the reference calls it an upscale only when both axes grow,
 * _is_upscale_required).  Out of scope: more than 2x and the residual mpv pass behind it, the shader's partial chains when only one
 * axis grows.  Stream-ordered, needs no reservation; the tables are built at the first call with a geometry -- that call allocates
 * and copies -- and kept in the context beside the other tap tables.  HDRTV_EINVAL, before any device call and with dst untouched,
 * for a NULL pointer, an unknown dtype, H, W, dH or dW < 1, pq with peak_nits <= 0, one axis at identity, a smaller axis, more than
 * 2x on an axis, ssim outside {0, 1}. */
int hdrtv_post_rgb48_ssimsr(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                            uint16_t *dst, int dH, int dW, int ssim);

/* Film grain, the last shader of every chain the reference builds (assets/shaders/filmgrain.glsl: its "Film grain" checkbox,
 * --film-grain 1, _build_shader_paths), as a rule on u16 RGB48 codes: a sink that takes these frames is not mpv and runs no GLSL
 * hook.  The rule is this project's restatement of the shader, operation by operation in float32: every multiply, add, subtract and
 * divide is rounded on its own (no fused multiply-add; GLSL parses x * 1.0/289.0 as (x * 1.0) / 289.0, a division, and likewise by
 * 41), fract(v) = v - floor(v).  tests/film_grain_ref.py restates it in NumPy and the GPU tests hold every entry point below to
 * it bit for bit.  For H x W grain positions, the position (x, y) and a per-frame seed in [0, 1) (the shader's `random`):
 *       px = (float32(x) + 0.5) / float32(W);  py = (float32(y) + 0.5) / float32(H);  mx = px + 1;  my = py + 1;  mz = seed + 1
 *       permute(v):  t = (34 v + 1) v;  return fract(t / 289) * 289
 *       state = permute(permute(mx) + my) + mz;  state = permute(state);  rnd = fract(state / 41)
 *       p = 0.95 rnd + 0.025;  q = p - 0.5;  r = q q;  num = a1 r + a0;  den = (r r + b1 r) + b0
 *       g = q (a2 + num / den);  g = g * 0.255121822830526
 *   with a0 = 0.151015505647689, a1 = -0.5303572634357367, a2 = 1.365020122861334, b0 = 0.132089632343748, b1 = -0.7607324991323768,
 *   each rounded once to float32.  |g| <= 0.50000006; no intermediate is denormal and den >= 0.011, so a flush-to-zero mode does not
 *   enter.  The grained code G of a code c, with the same g for the three channels of a pixel and the intensity I:
 *       s = float32(c) / 65535;  v = sat(s + I * g);  G = (int)(v * 65535 + 0.5)        (the quantiser of the unscaled entry point)
 *   The reference's I is 0.01 (a code moves by at most +-328); I * g = 0 returns c for every code.
 * The seed of frame `frame_index` of a stream is an integer hash, so that two sinks (two lanes, two devices) agree on a frame:
 *       h = (frame_index * 0x9E3779B1 + stream_seed * 0x85EBCA77) mod 2^32;  h ^= h >> 16;  h = h * 0x21F0AAAD mod 2^32;
 *       h ^= h >> 15;  h = h * 0x735A2D97 mod 2^32;  h ^= h >> 15;  seed = float32((h >> 8) * 2^-24)
 *   hdrtv_film_grain_seed computes it on the host (no context, no device).
 * UNPINNED: mpv's own `random` sequence; the texture format mpv keeps a hooked MAIN in (this rule requantises to u16); what the
 * GLSL compiler of a display makes of the divisions.
 * Where the grain sits, as _build_shader_paths orders the chain:
 *   hdrtv_rgb48_film_grain        G of the codes at src_rgb48, positions over H x W.  dst == src is allowed (a pixel depends on itself
 *                                 only); any other overlap is the caller's error.
 *   hdrtv_post_rgb48_grain        the codes hdrtv_post_rgb48 (pq = 0; peak_nits ignored) / hdrtv_post_pq_rgb48 (pq != 0) would write,
 *                                 grained, in one launch: a frame delivered at the processing size.
 *   hdrtv_post_rgb48_scaled_grain the Lanczos chain of hdrtv_post_rgb48_scaled_cas (antiring 0 .. 256, cas 0 or 1032 .. 4096): cas is
 *                                 an ffmpeg filter in front of mpv, the grain hooks MAIN at the processing size, mpv scales last.  So:
 *                                 codes, CAS where asked, G with positions over H x W, then the integer passes on the grained codes.
 *                                 A tap outside the frame reads the grained edge pixel: G at the clamped position.
 *   hdrtv_post_rgb48_fsr_grain    EASU and RCAS hook MAIN first and enlarge it, the grain comes after: G of the codes
 *                                 hdrtv_post_rgb48_fsr would write, positions over dH x dW.
 *   Every fused result is thus its twin's rule composed with this one; the three fused forms keep no codes in device memory in
 *   between.  The grain in front of the spline36 / SSimSuperRes and Mitchell / SSimDownscaler scalers is not provided.
 * intensity == 0 delegates to the twin without grain and writes its bytes (hdrtv_rgb48_film_grain copies the codes); equal sizes
 * (dH == H && dW == W) in the two scaled forms delegate to hdrtv_post_rgb48_grain.  Stream-ordered; no reservation beyond the
 * twin's tables.  HDRTV_EINVAL, before any device call and with dst untouched, for everything the twin refuses (hdrtv_post_rgb48 /
 * hdrtv_post_pq_rgb48, hdrtv_post_rgb48_scaled_cas, hdrtv_post_rgb48_fsr; for hdrtv_rgb48_film_grain a NULL pointer or H, W < 1), for
 * an intensity that is NaN, infinite or outside [0, 0.1], and for a seed that is NaN or outside [0, 1). */
float hdrtv_film_grain_seed(uint32_t stream_seed, uint32_t frame_index);
int hdrtv_rgb48_film_grain(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, float intensity, float seed,
                           uint16_t *dst);
int hdrtv_post_rgb48_grain(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                           uint16_t *dst, float intensity, float seed);
int hdrtv_post_rgb48_scaled_grain(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                                  uint16_t *dst, int dH, int dW, int antiring, int cas, float intensity, float seed);
int hdrtv_post_rgb48_fsr_grain(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                               uint16_t *dst, int dH, int dW, int rcas, float sharpness, float intensity, float seed);

/* Tone mapping of the delivered frames to the sink's peak, the last step of the reference's display chain (gui_mpv_widget.py
 * _MPV_TONE_MAPPING: mpv's tone-mapping=spline, tone-mapping-param=0.45), as a rule on full-range u16 RGB48 codes of BT.2020 PQ -- what
 * hdrtv_post_rgb48 writes for the model's output.  The curve reaches the device as one table, gain[65536] of float32, built on the
 * host (hdrtv_mi355x/tonemap.py has clip, BT.2390 and a spline); the device is held bit for bit to this pixel rule
 * (tests/tonemap_ref.py restates it in NumPy):
 *       m = max(R, G, B)                         (u16 codes)
 *       g = gain[m]
 *       for c in (R, G, B):   y = lin[c] * g     one float32 multiply, rounded to nearest: no FMA, no reassociation
 *                             y = min(max(y, 0), 1)
 *                             out = code(y)
 *   code(y) = floor(pq(y) * 65535 + 0.5) with the ST.2084 OETF in double precision and 1.0 = 10000 nits: the exact code
 *   hdrtv_post_pq_rgb48 is defined by, without its lin * peak / 10000 in front.  lin[c] = the float32 nearest to the ST.2084 EOTF of
 *   c / 65535 (1.0 = 10000 nits), then moved along the float32 grid until code(lin[c]) == c.  That round trip holds for all 65536
 *   codes and is part of the rule: a gain of exactly 1.0f is the identity on every byte.  hdrtv_pq_eotf_table writes lin (host
 *   only: no context, no device), so that a caller or a test reads the rule's table instead of deriving it with another libm.
 *   The maximum channel carries the curve and the other two are scaled by the same linear-light factor: hue is kept and, for a
 *   non-increasing gain-times-level, no channel exceeds the target (mpv's "max" tone-mapping mode).  A NaN product counts as 0.
 * Out of scope: desaturation, gamut mapping, an SDR (BT.709 / gamma) target, and a measured per-scene source peak (mpv's
 * hdr-compute-peak).  UNPINNED: parity with mpv / libplacebo's own curves and its peak detection; the rule above is this library's.
 *   hdrtv_rgb48_tonemap       the rule on the codes at src_rgb48.  dst == src is allowed (a pixel depends on itself only); any other
 *                             overlap is the caller's error.
 *   hdrtv_post_rgb48_tonemap  the codes hdrtv_post_rgb48 (pq = 0; peak_nits ignored) / hdrtv_post_pq_rgb48 (pq != 0) would write,
 *                             tone-mapped, in one launch; no codes go to device memory in between.
 * dev_gain: 65536 floats in device memory, owned by the caller and read by the launch (keep it until the stream has passed it).
 * Stream-ordered; no reservation (the context keeps lin and the code boundaries, uploaded by its first tone-map call).
 * HDRTV_EINVAL, before any device call and with dst untouched, for a NULL pointer, for H or W < 1 and, in the fused form, for
 * everything the twin refuses (a dtype that is neither HDRTV_F16 nor HDRTV_F32, pq without peak_nits > 0). */
int hdrtv_pq_eotf_table(float *dst65536);
int hdrtv_rgb48_tonemap(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, const float *dev_gain, uint16_t *dst);
int hdrtv_post_rgb48_tonemap(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                             const float *dev_gain, uint16_t *dst);

/* 10-bit limited-range Y'CbCr for an encoder (HEVC Main10, hardware encoders, ProRes): P010 and yuv420p10le are 3 bytes per pixel,
 * yuv422p10le 4, against the 6 of RGB48.  The reference's export converts on the CPU: it pipes rgb48le into ffmpeg, zscale goes to
 * BT.2020nc limited range and format=yuv422p10le feeds prores_ks (gui_export.py:948-1005).  The network's output is PQ-encoded BT.2020
 * R'G'B' (what the reference tags its rgb48le stream as), so the matrix is BT.2020 non-constant luminance, the range limited, and
 * there is no matrix parameter.  Parity with zscale / swscale is UNPINNED (ffmpeg is not part of the reference tree); the conversion
 * is this integer rule, restated in tests/ycbcr10_ref.py, which the GPU tests hold both entry points to bit for bit.
 *  1. codes: R, G, B in [0, 65535] = exactly what hdrtv_post_rgb48 (pq = 0; peak_nits ignored) or hdrtv_post_pq_rgb48 (pq != 0)
 *     writes for that pixel; the conversion sees nothing but these integers.
 *  2. coefficients, in double with rnd(v) = floor(v + 0.5), scale 2^20, Kr = 0.2627, Kb = 0.0593, sY = 876 * 2^20 / 65535,
 *     sC = 896 * 2^20 / 65535:  A = rnd(sY) = 14016;  YR = rnd(Kr sY) = 3682, YB = rnd(Kb sY) = 831, YG = A - YR - YB = 9503;
 *     Hc = rnd(sC / 2) = 7168;  UR = rnd(-Kr / (2 (1 - Kb)) sC) = -2002, UG = -Hc - UR = -5166, UB = Hc;
 *     VR = Hc, VB = rnd(-Kb / (2 (1 - Kr)) sC) = -577, VG = -Hc - VB = -6591.  Green is the remainder: the luma row sums to A,
 *     each chroma row to 0, every grey gives Cb = Cr = 512 exactly.
 *  3. luma, per pixel (fits int32):  Y = 64 + ((YR R + YG G + YB B + 2^19) >> 20).
 *  4. chroma: per pixel u = UR R + UG G + UB B, v likewise, unrounded; a sample is 512 + ((sum(w u) + (Wt << 19)) >> (20 + log2 Wt))
 *     with a flooring shift, in int64 (the sum needs 36 bits); neighbour indices are clamped to the frame (edge repeat):
 *       4:2:2 (horizontally co-sited):  columns 2i-1, 2i, 2i+1 with weights 1 2 1, every row; Wt = 4
 *       4:2:0, HDRTV_SITING_LEFT (MPEG-2 / H.264; what ffmpeg and x265 assume when nothing is said; the siting of the 4:2:0 input
 *              path):  the same columns, rows 2j, 2j+1 with weights 1 1; Wt = 8
 *       4:2:0, HDRTV_SITING_TOPLEFT (BT.2100 / HDR10 delivery):  the same columns, rows 2j-1, 2j, 2j+1 with weights 1 2 1; Wt = 16
 *     The weights are non-negative: luma stays in [64, 940], chroma in [64, 960] without a clamp.
 *     Known answers (R, G, B) -> Y, Cb, Cr on a constant frame: black 64 512 512; 65535^3 940 512 512; 32768^3 502 512 512;
 *     red 294 387 960; green 658 189 100; blue 116 960 476.  Against the exact double formula the per-pixel values differ by at most
 *     0.533 code (200 000 random triples).
 * Layouts, all little-endian u16; W even, H even for the two 4:2:0 layouts; pitches in bytes and even, y_pitch >= 2 W; no other
 * alignment of a base or a pitch is required:
 *   HDRTV_YCC_P010      dst_y, then dst_u = ONE interleaved CbCr plane (Cb at u16 2i, Cr at 2i+1; H/2 rows), dst_v = NULL; the value in
 *                       the HIGH ten bits (v << 6); c_pitch >= 2 W
 *   HDRTV_YCC_YUV420P10 dst_y, dst_u (Cb), dst_v (Cr); H/2 rows of W/2 samples; the value in the low ten bits; c_pitch >= W
 *   HDRTV_YCC_YUV422P10 as above with chroma planes of H rows; siting must be HDRTV_SITING_LEFT
 * hdrtv_post_ycbcr10 goes from the model's planar tensor to the planes in one kernel, without an RGB48 intermediate.
 * hdrtv_rgb48_to_ycbcr10 applies the same rule to RGB48 codes already in device memory ([H][W][3]): a scaled frame becomes Y'CbCr in
 * two launches, hdrtv_post_rgb48_scaled and this one.  hdrtv_ycbcr10_bytes: the bytes of a frame with its planes back to back at their
 * minimum pitches (3 H W, 4:2:2: 4 H W), or a negative value for a bad argument.  Dithering is the business of the entry points
 * below (ordered: _ex; Floyd-Steinberg error diffusion: _fs).  Out of scope: full range, 12 bits, 4:4:4, bitstream / SEI writing (hdrtv_light_stats measures the content light level an HDR10 SEI carries), and fusing the Lanczos pass with the conversion.
 * Stream-ordered, no reservation needed.  HDRTV_EINVAL, with dst untouched, for a NULL pointer, a non-positive size, an odd W, an odd H
 * with 4:2:0, a short or odd pitch, an unknown fmt, siting or dtype, P010 with a non-NULL dst_v, a siting other than LEFT with 4:2:2, or
 * pq with peak_nits <= 0. */
#define HDRTV_YCC_P010 0
#define HDRTV_YCC_YUV420P10 1
#define HDRTV_YCC_YUV422P10 2
#define HDRTV_SITING_LEFT 0
#define HDRTV_SITING_TOPLEFT 1
int hdrtv_post_ycbcr10(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                       int fmt, int siting, uint16_t *dst_y, int y_pitch, uint16_t *dst_u, uint16_t *dst_v, int c_pitch);
int hdrtv_rgb48_to_ycbcr10(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, int fmt, int siting,
                           uint16_t *dst_y, int y_pitch, uint16_t *dst_u, uint16_t *dst_v, int c_pitch);
int64_t hdrtv_ycbcr10_bytes(int fmt, int H, int W);

/* Output cleanup: debanding of the RGB48 codes and dither of the 10-bit Y'CbCr conversion, ordered or by error diffusion.  The
 * reference's export never hands its encoder a bare 16 -> 10 bit rounding: its ffmpeg chain is deband,
 * zscale=...:dither=error_diffusion, format=yuv422p10le (gui_export.py:948-962), on the CPU.  zscale's dither=ordered and a debanding
 * gather are per-pixel integer rules; error diffusion is a chain through the whole plane, run here as a skewed wavefront (the
 * Floyd-Steinberg rule further below).  Parity with ffmpeg's deband and zscale's dithers is UNPINNED (ffmpeg is not part of the
 * reference tree; zimg diffuses in float); all three steps are the integer rules below, restated in tests/cleanup_ref.py (deband,
 * ordered dither) and tests/fs_ref.py (error diffusion), which the GPU tests hold every entry point to bit for bit.  All are off
 * unless asked for, and deband can be used with either dither or alone.
 *
 * Deband rule (hdrtv_rgb48_deband): u16 RGB48 codes [H][W][3] in, [H][W][3] out, never in place.  range R in 1..16 (default 16),
 * threshold T in 1..65535 u16 code units (default 1311 = rnd(0.02 * 65535), the share ffmpeg's deband defaults to), seed S any u32
 * (default 0; the pattern is the same in every frame).  Per pixel (x, y), all arithmetic in u32 unless said otherwise:
 *   h = S * 0x9E3779B9 + y * W + x;  h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;  h *= 0x846ca68b;  h ^= h >> 16
 *   dx = (((h & 0xffff) * (2R + 1)) >> 16) - R;  dy = (((h >> 16) * (2R + 1)) >> 16) - R      (each in [-R, R])
 *   four reference pixels ref_0..3 at (x + dx, y + dy), (x - dx, y + dy), (x - dx, y - dy), (x + dx, y - dy), every coordinate
 *   clamped to the frame; the three channels use the same four positions.
 *   If |ref_k,c - src_c| < T for all four references and all three channels, every channel c becomes
 *   (ref_0,c + ref_1,c + ref_2,c + ref_3,c + 2) >> 2; otherwise the pixel is copied unchanged (all or nothing: hue is kept).
 * Any H, W >= 1.  HDRTV_EINVAL, with dst untouched, for a NULL pointer, H or W < 1, src == dst or overlapping buffers, a range
 * outside 1..16 or a threshold outside 1..65535.
 *
 * Ordered-dither rule (hdrtv_post_ycbcr10_ex / hdrtv_rgb48_to_ycbcr10_ex, dither = HDRTV_DITHER_ORDERED): the Y'CbCr rule above with
 * its rounding constants replaced by a 16 x 16 Bayer threshold.  M(x, y) in 0..255: with a = (x ^ y) & 15 and b = y & 15, bit i of a
 * goes to bit 7 - 2i of M and bit i of b to bit 6 - 2i, i = 0..3 (the recursive matrix built from [[0, 2], [3, 1]]; a permutation
 * of 0..255 over every aligned 16 x 16 block; no table).
 *   luma:    Y = 64 + ((YR R + YG G + YB B + t) >> 20),  t = (2 M(x, y) + 1) << 11  (the mean of t over a block is exactly 2^19)
 *   chroma:  the sums and the shift SH = 20 + log2 Wt stay; the constant Wt << 19 becomes (2 M(i, j) + 1) << (SH - 9), where (i, j)
 *            is the sample's column and row in the chroma plane.
 * Luma stays in [64, 940] (the largest sum is 14016 * 65535 < 876 * 2^20) and chroma in [64, 960] without a clamp, in the integer
 * widths of the undithered rule; over an aligned 16 x 16 block of one colour the mean of Y is within 1/512 code of the unrounded
 * value.  P010 shifts left by 6 as before.  dither = HDRTV_DITHER_NONE launches the kernels of hdrtv_post_ycbcr10 /
 * hdrtv_rgb48_to_ycbcr10 and writes their bytes; any other value of dither is HDRTV_EINVAL, as is everything those refuse.
 * Out of scope: random or blue-noise dither, temporal variation of either pattern, dithering the u8 or RGB48
 * outputs, debanding the model's float tensor, grain synthesis, and fusing deband with the conversion or the Lanczos pass. */
#define HDRTV_DITHER_NONE 0
#define HDRTV_DITHER_ORDERED 1
int hdrtv_rgb48_deband(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, int range, int threshold,
                       uint32_t seed, uint16_t *dst_rgb48);
int hdrtv_post_ycbcr10_ex(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                          int fmt, int siting, uint16_t *dst_y, int y_pitch, uint16_t *dst_u, uint16_t *dst_v, int c_pitch,
                          int dither);
int hdrtv_rgb48_to_ycbcr10_ex(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, int fmt, int siting,
                              uint16_t *dst_y, int y_pitch, uint16_t *dst_u, uint16_t *dst_v, int c_pitch, int dither);

/* Floyd-Steinberg error diffusion of the 10-bit Y'CbCr conversion (hdrtv_post_ycbcr10_fs / hdrtv_rgb48_to_ycbcr10_fs): what the
 * reference's export asks zscale for (dither=error_diffusion), as an integer rule of this library's own -- parity with zimg, which
 * diffuses in float, is UNPINNED.  tests/fs_ref.py restates the rule in numpy, twice (a raster loop and a skewed wavefront); the GPU
 * tests hold both entry points to it bit for bit.  The rule works on the RGB48 codes of step 1 of the Y'CbCr rule above and on each
 * of the three planes (Y', Cb, Cr) alone; P010's interleaved plane is two chains.
 *   For a plane of w x h samples, S(i, j) is the integer sum the Y'CbCr rule forms for that sample, before its rounding constant:
 *     luma    S = YR R + YG G + YB B,          SH = 20, base 64,  k in [0, 876]
 *     chroma  S = sum(w u) of the siting,      SH = 20 + log2 Wt (22, 23 or 24), base 512, k in [-448, 448]
 *   The sample in 1/4096 code:  u = (S + (1 << (SH - 13))) >> (SH - 12), an arithmetic shift.
 *   Then in raster order (rows top to bottom, each left to right, not serpentine), with E = 0 everywhere at the start:
 *     v = u(i, j) + E(i, j)
 *     k = clamp((v + 2048) >> 12, lo, hi)
 *     r = clamp(v - 4096 k, -2048, 2047)
 *     a = (7 r) >> 4;  b = (3 r) >> 4;  c = (5 r) >> 4;  d = r - a - b - c          (arithmetic shifts)
 *     E(i+1, j) += a;  E(i-1, j+1) += b;  E(i, j+1) += c;  E(i+1, j+1) += d        (terms outside the plane are dropped)
 *     sample = base + k                                                            (P010: << 6)
 * Everything fits 32-bit integers; |E| stays within 2047 + 3, luma in [64, 940], chroma in [64, 960].  (u + 2048) >> 12 is not
 * the undithered rule's rounding -- it rounds twice, once to 1/4096 code and once to the code --: this is a rule of its own, and
 * a frame converted with it differs from the undithered one even where no error has arrived yet.  Over a flat plane the mean of
 * k is within 32/4096 code of u (the loss is what falls off the right and bottom edges).
 * `scratch`: device memory of hdrtv_ycbcr10_fs_scratch_bytes(fmt, H, W) bytes (4 (H W + 2 ch cw + W + 2 cw), ch x cw the chroma
 * plane; negative for a bad argument), 4-byte aligned, the caller's: its contents on entry do not matter and nothing is kept in
 * it between calls.  A call is two launches on `stream` -- the samples u of all three planes into the scratch, fully parallel, then
 * one workgroup per plane that runs the chain as a wavefront of HDRTV_FS_ROWS rows (a lane per row), staging HDRTV_FS_CHUNK columns
 * at a time -- so the calls are stream-ordered, need no reservation, and are safe on two lanes (two streams) with two scratches;
 * two calls in flight must not share one.  The cost is the chain's latency, not bandwidth: measured 6.7 ms at 3840x2160 and
 * 2.1 ms at 1920x1080 on one MI355X, for 4:2:0 and 4:2:2 alike (profiles/fs_dither_timing.txt), against 20 us
 * for the ordered dither.
 * The argument rules are those of hdrtv_post_ycbcr10 / hdrtv_rgb48_to_ycbcr10, plus HDRTV_EINVAL for a NULL or misaligned scratch;
 * on refusal nothing is written.  hdrtv_*_ex(..., dither = 2) stays HDRTV_EINVAL: error diffusion is reached through these entry
 * points only.  Out of scope: serpentine scanning, other kernels (Sierra, Stucki), spreading one chain over several CUs. */
#define HDRTV_FS_ROWS 256
#define HDRTV_FS_CHUNK 32
int64_t hdrtv_ycbcr10_fs_scratch_bytes(int fmt, int H, int W);
int hdrtv_post_ycbcr10_fs(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                          int fmt, int siting, uint16_t *dst_y, int y_pitch, uint16_t *dst_u, uint16_t *dst_v, int c_pitch,
                          void *scratch);
int hdrtv_rgb48_to_ycbcr10_fs(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, int fmt, int siting,
                              uint16_t *dst_y, int y_pitch, uint16_t *dst_u, uint16_t *dst_v, int c_pitch, void *scratch);

/* HDR10 content light level (CTA-861.3 MaxCLL / MaxFALL; x265 max-cll=, HEVC SEI 144): the per-frame record those two numbers are
 * made from, measured on the device from exactly the codes the sink receives.  The reference has no counterpart: its export tags the
 * stream as PQ / BT.2020 (gui_export.py:957-977) and carries no light level.  The statistic is this integer rule, restated in
 * tests/lightlevel_ref.py, which the GPU tests hold both entry points to bit for bit.
 *  1. codes: R, G, B in [0, 65535] = exactly what hdrtv_post_rgb48 (pq = 0; peak_nits ignored) or hdrtv_post_pq_rgb48 (pq != 0)
 *     writes for that pixel; the statistic sees nothing but these integers, so it describes the Y'CbCr outputs too (they are derived
 *     from the same codes).
 *  2. per pixel of the rectangle x0 <= x < x0 + rw, y0 <= y < y0 + rh (the active picture, which CTA-861.3 measures; the full frame
 *     is 0, 0, W, H):  m = max(R, G, B).
 *  3. the record, HDRTV_LIGHT_WORDS = 4104 little-endian u32 words, HDRTV_LIGHT_BINS = 4096:
 *       [0 .. 4095]            hist[b] = the number of pixels with m >> 4 == b
 *       [4096] [4097] [4098]   the largest R, G and B code (MaxSCL)
 *       [4099]                 the largest m
 *       [4100] [4101]          low and high word of the u64 sum of m over the rectangle
 *       [4102]                 rw * rh  (= the sum of hist)
 *       [4103]                 0
 *     Every call overwrites the record (it is zeroed on `stream` in front of the kernel); nothing accumulates across calls.  Integer
 *     adds and maxima only: the record is identical from run to run.
 *  4. host side (hdrtv_mi355x/lightlevel.py), in double, the ST.2084 EOTF with the constants of gui_objective_metrics.py:486-491:
 *       nits(c) = 10000 * (max(p - c1, 0) / (c2 - c3 p))^(1/m1),  p = (c / 65535)^(1/m2)
 *     nits(0) = 0, nits(65535) = 10000, nits(33297) = 100.0012.., nits(49271) within 0.3 of 1000.
 *       frame CLL  = nits(word 4099), exact;
 *       frame FALL = sum_b hist[b] * nits(16 b + 8) / (rw * rh): off the exact per-pixel mean of nits(m) by at most the widest
 *                    deviation inside a bin, max_c |nits(c) - nits(16 (c >> 4) + 8)|;
 *       MaxCLL / MaxFALL of a stream = the largest frame CLL / FALL, reported as floats and as integers floor(v + 0.5).
 * hdrtv_light_stats reads the model's planar tensor (what hdrtv_post_rgb48 / hdrtv_post_ycbcr10 read); hdrtv_rgb48_light_stats reads
 * RGB48 codes already in device memory ([H][W][3]: a scaled frame, a ring slot's device buffer).  dev_stats: HDRTV_LIGHT_WORDS u32 of
 * device memory, 8-byte aligned.  Both are stream-ordered, need no reservation and never synchronise; the PQ table is the context's
 * (hdrtv_post_pq_rgb48's).  Out of scope: writing SEI / bitstream bytes (the encoder's job), mastering-display primaries, HDR10+
 * dynamic metadata, and fusing the statistic into the post kernels.  HDRTV_EINVAL, with the record untouched, for a NULL pointer, a
 * non-positive size, an empty rectangle or one that leaves the frame, dev_stats not 8-byte aligned, an unknown dtype, or pq with
 * peak_nits <= 0. */
#define HDRTV_LIGHT_BINS 4096
#define HDRTV_LIGHT_WORDS 4104
int hdrtv_light_stats(hdrtv_ctx *ctx, void *stream, const void *dev_out, int dtype, int H, int W, int pq, float peak_nits,
                      int x0, int y0, int rw, int rh, uint32_t *dev_stats);
int hdrtv_rgb48_light_stats(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W,
                            int x0, int y0, int rw, int rh, uint32_t *dev_stats);

/* The host step in front of preprocess, on the device: _letterbox_bgr
 * (src/gui_scaling.py:228-244), i.e. cv2.resize preserving the aspect ratio -- INTER_AREA when shrinking,
 * INTER_CUBIC when enlarging -- centred on a black [dh][dw] canvas.  src / dst are device u8 BGR HWC.
 * Parity with cv2 itself is UNPINNED (OpenCV is not part of the reference tree); the arithmetic is the
 * restatement in oracle/letterbox_oracle.py, which the GPU tests hold this entry point to bit for bit. */
int hdrtv_letterbox_u8(hdrtv_ctx *ctx, void *stream, const uint8_t *dev_src_bgr, int sh, int sw,
                       uint8_t *dev_dst_bgr, int dh, int dw);

/* 8-bit 4:2:0 Y'CbCr input, the host step in front of preprocess on the device: what decoders hand out (ffmpeg yuv420p = I420,
 * a hardware decoder's NV12), 1.5 bytes per pixel.  H and W even; chroma planes Hc = H/2 rows by Wc = W/2 samples.
 *   I420: dev_y, dev_u (Cb), dev_v (Cr); y_pitch >= W, c_pitch >= W/2 (both planes share c_pitch).
 *   NV12: dev_y and dev_u = the interleaved CbCr plane (Cb at byte 2i, Cr at 2i+1), dev_v = NULL; c_pitch >= W.
 * Pitches are in bytes; no plane start or pitch needs any alignment.  matrix: 601, 709 or 2020 (BT.2020 non-constant
 * luminance); full_range: 0 limited (Y' 16..235), 1 full.  BT.709 limited is the usual choice for HD / UHD SDR video.
 * Parity with a decoder's own conversion (swscale behind cv2.VideoCapture) is UNPINNED; the conversion is this integer rule:
 *  1. chroma upsampling, MPEG-2 / H.264 siting (horizontally co-sited, vertically centred), per chroma plane C:
 *       luma row y:    j = y>>1; n = (y odd) ? min(j+1, Hc-1) : max(j-1, 0); V4[i] = 3*C[j][i] + C[n][i]
 *       luma column x: i = x>>1; i2 = (x odd) ? min(i+1, Wc-1) : i;          C8 = V4[i] + V4[i2]   (8 x chroma)
 *  2. offsets: y = Y - 16 (limited) or Y (full); cb = C8_U - 1024; cr = C8_V - 1024
 *  3. matrix, int32 with arithmetic (flooring) shifts, each result clamped to [0, 255]:
 *       R = (A*y + RV*cr + 32768) >> 16;  G = (A*y - GU*cb - GV*cr + 32768) >> 16;  B = (A*y + BU*cb + 32768) >> 16
 *     with rnd(v) = floor(v + 0.5) in double, Kg = 1 - Kr - Kb, sY = 255/219 and sC = 255/224 (limited) or 1 and 1 (full):
 *       A = rnd(sY*2^16), RV = rnd(2(1-Kr)*sC*2^13), GU = rnd(2(1-Kb)*Kb/Kg*sC*2^13), GV = rnd(2(1-Kr)*Kr/Kg*sC*2^13),
 *       BU = rnd(2(1-Kb)*sC*2^13);  (Kr, Kb) = (0.299, 0.114) BT.601, (0.2126, 0.0722) BT.709, (0.2627, 0.0593) BT.2020.
 *     BT.709 limited: A 76309, RV 14686, GU 1747, GV 4366, BU 17305.
 * hdrtv_yuv420_to_bgr_u8 writes the result as u8 [H][W][3] B, G, R (the frame hdrtv_preprocess and hdrtv_letterbox_u8 read);
 * needs no reservation.  hdrtv_preprocess_yuv420 equals hdrtv_preprocess of that frame bit for bit, in both outputs, for fp16
 * and fp32 contexts and every condition mode, in one pass over the planes (fp16); same reservation rule as hdrtv_preprocess.
 * HDRTV_EINVAL for a NULL pointer, odd H or W, a pitch below its plane's width, an unknown layout, matrix or range, or NV12
 * with a non-NULL dev_v; HDRTV_ESTATE (preprocess) before hdrtv_reserve(H, W). */
#define HDRTV_YUV_I420 0
#define HDRTV_YUV_NV12 1
int hdrtv_yuv420_to_bgr_u8(hdrtv_ctx *ctx, void *stream, const uint8_t *dev_y, int y_pitch,
                           const uint8_t *dev_u, const uint8_t *dev_v, int c_pitch, int layout,
                           int matrix, int full_range, int H, int W, uint8_t *dev_bgr_hwc);
int hdrtv_preprocess_yuv420(hdrtv_ctx *ctx, void *stream, const uint8_t *dev_y, int y_pitch,
                            const uint8_t *dev_u, const uint8_t *dev_v, int c_pitch, int layout,
                            int matrix, int full_range, int H, int W, void *dev_rgb_chw, void *dev_cond);

/* 10-bit Y'CbCr input: a ProRes / DNxHR mezzanine (yuv422p10le), a broadcast master, a 10-bit HEVC / AV1 SDR stream (a hardware
 * decoder's P010).  The rule above at ten bits; the ten source bits reach the network's fp16 tensor (all 1024 values
 * fp16(float(c) * fp32(1/1023)) are distinct), four times the levels of u8 / 255.  10-bit 4:2:0 is 3 bytes per pixel, as bgr24:
 * the gain is precision and a removed host pass, not PCIe bytes.  Layouts, planes and pitches are those of the output side
 * (HDRTV_YCC_P010 / _YUV420P10 / _YUV422P10 above), samples little-endian u16:
 *   HDRTV_YCC_P010      dev_y, dev_u = the interleaved CbCr plane (Cb at u16 2i, Cr at 2i+1; H/2 rows), dev_v = NULL;
 *                       v = word >> 6 (the low six bits are ignored); c_pitch >= 2 W
 *   HDRTV_YCC_YUV420P10 dev_y, dev_u (Cb), dev_v (Cr); H/2 rows of W/2 samples; v = word & 0x3ff; c_pitch >= W
 *   HDRTV_YCC_YUV422P10 as above with chroma planes of H rows
 * Pitches are in bytes and even, y_pitch >= 2 W; no base or pitch needs more than two-byte alignment.  W even; H even for the two
 * 4:2:0 layouts.  matrix and full_range as for the 8-bit entry points.  Chroma planes Hc rows by Wc = W/2 samples:
 *  1. chroma upsampling to 8 x chroma, per chroma plane C (4:2:0: MPEG-2 siting only, the 8-bit rule's integers):
 *       4:2:0, luma row y: j = y>>1; n = (y odd) ? min(j+1, Hc-1) : max(j-1, 0); V4[i] = 3*C[j][i] + C[n][i]
 *       4:2:2, luma row y: V4[i] = 4*C[y][i]
 *       luma column x:     i = x>>1; i2 = (x odd) ? min(i+1, Wc-1) : i;          C8 = V4[i] + V4[i2]
 *  2. offsets: y = Y - 64 (limited) or Y (full); cb = C8_U - 4096; cr = C8_V - 4096
 *  3. matrix, int32 with arithmetic (flooring) shifts, each result clamped to [0, 1023]:
 *       R = (A*y + RV*cr + 32768) >> 16;  G = (A*y - GU*cb - GV*cr + 32768) >> 16;  B = (A*y + BU*cb + 32768) >> 16
 *     the coefficients by the 8-bit formulas with sY = 1023/876 and sC = 1023/896 (limited) or 1 and 1 (full).
 *     BT.709 limited: A 76533, RV 14729, GU 1752, GV 4378, BU 17356.  Every intermediate stays below 2^28; the result is within
 *     0.57 code of the exact formula (0.5 rounding + 0.0073 from A + 2 x 0.031 from the chroma coefficients).
 * tests/ycbcr10_in_ref.py restates the rule in numpy; the GPU tests hold both entry points to it bit for bit.
 * hdrtv_ycbcr10_to_rgb10 writes the codes as u16 [H][W][3] R, G, B in 0..1023 and needs no reservation.
 * hdrtv_preprocess_ycbcr10 writes the tensor fp16(float(code) * fp32(1/1023)) of those codes (the same expression in fp32 for an
 * fp32 context) and its condition map, in one pass over the planes (fp16; two launches in an fp32 context); same reservation rule
 * as hdrtv_preprocess.  HDRTV_EINVAL, the destinations untouched, for a NULL pointer, a non-positive or odd W, an odd H with
 * 4:2:0, a short or odd pitch, an unknown fmt, matrix or range, P010 with a non-NULL dev_v or a planar layout with a NULL dev_v;
 * HDRTV_ESTATE (preprocess) before hdrtv_reserve(H, W). */
int hdrtv_ycbcr10_to_rgb10(hdrtv_ctx *ctx, void *stream, const uint16_t *dev_y, int y_pitch,
                           const uint16_t *dev_u, const uint16_t *dev_v, int c_pitch, int fmt,
                           int matrix, int full_range, int H, int W, uint16_t *dev_rgb_hwc);
int hdrtv_preprocess_ycbcr10(hdrtv_ctx *ctx, void *stream, const uint16_t *dev_y, int y_pitch,
                             const uint16_t *dev_u, const uint16_t *dev_v, int c_pitch, int fmt,
                             int matrix, int full_range, int H, int W, void *dev_rgb_chw, void *dev_cond);

/* Letterbox of a 10-bit Y'CbCr frame at ten bits: the reference's "lower-resolution processing" (a 3840x2160 source letterboxed to a
 * 1920x1080 processing size, _letterbox_bgr(frame, proc_w, proc_h) in src/gui_pipeline_worker_frame_processing.py:207-210) without
 * a pass through 8 bits.  The planes (layouts, pitches, matrix and range as above) are read at the SOURCE size sh x sw and the result
 * is written at dh x dw by one kernel; no source-sized RGB frame exists in device memory.  The rule is the reference's order of
 * operations, decode then letterbox:
 *  1. the R, G, B codes 0..1023 of every source pixel by the rule of hdrtv_ycbcr10_to_rgb10, chroma clamps at the edges of the
 *     source frame;
 *  2. the geometry of hdrtv_letterbox_u8 (oracle/letterbox_oracle.py geometry: new_w x new_h centred at (x0, y0), Python's round());
 *     pixels outside that rectangle are code 0 in all three channels;
 *  3. the resize of the codes by hdrtv_letterbox_u8's algorithms with 1023 in the place of 255:
 *       new == source size: the codes themselves;
 *       shrinking, integer ratio ix x iy: int32 box sums; 2 x 2 is (sum + 2) >> 2, any other ratio
 *         rint(float32(sum) * (float32(1) / float32(ix * iy))), half to even, clamped to [0, 1023];
 *       shrinking, fractional ratio: computeResizeAreaTab's float32 weights; the horizontal sums of a source row accumulated from 0
 *         in table order, multiply and add separate; vertically beta * buf for the first entry and sum + beta * buf after it; rint,
 *         then the clamp;
 *       enlarging: the 11-bit Keys coefficients (A = -0.75) and offsets of the 8-bit path, horizontal then vertical integer passes
 *         with replicated borders in 64 bits, (v + 2^21) >> 22, clamped to [0, 1023].
 * Parity with OpenCV's own 16-bit resize is UNPINNED and not claimed: OpenCV is not part of the reference tree and its u16 cubic path
 * is a float one.  tests/letterbox10_ref.py restates the rule in numpy; the GPU tests hold both entry points to it bit for bit.
 * A shrink beyond 4x on an axis (sw > 4 new_w or sh > 4 new_h) is HDRTV_EINVAL, the cap of hdrtv_post_rgb48_down; enlargement has
 * no cap.
 * hdrtv_letterbox_ycbcr10 writes the codes as u16 [dh][dw][3] R, G, B and needs no reservation.
 * hdrtv_preprocess_ycbcr10_letterboxed writes the tensor fp16(float(code) * fp32(1/1023)) of those codes at H x W (the same
 * expression in fp32 for an fp32 context), then the condition map of that tensor in a second launch; same reservation rule as
 * hdrtv_preprocess: HDRTV_ESTATE before hdrtv_reserve(H, W).  With sh x sw == H x W the tensor is that of hdrtv_preprocess_ycbcr10.
 * HDRTV_EINVAL, the destinations untouched, for a NULL pointer, a non-positive size, a shrink beyond 4x on an axis and everything
 * hdrtv_ycbcr10_to_rgb10 refuses at the source size. */
int hdrtv_letterbox_ycbcr10(hdrtv_ctx *ctx, void *stream, const uint16_t *dev_y, int y_pitch,
                            const uint16_t *dev_u, const uint16_t *dev_v, int c_pitch, int fmt,
                            int matrix, int full_range, int sh, int sw, uint16_t *dev_rgb10_hwc, int dh, int dw);
int hdrtv_preprocess_ycbcr10_letterboxed(hdrtv_ctx *ctx, void *stream, const uint16_t *dev_y, int y_pitch,
                                         const uint16_t *dev_u, const uint16_t *dev_v, int c_pitch, int fmt,
                                         int matrix, int full_range, int sh, int sw, int H, int W,
                                         void *dev_rgb_chw, void *dev_cond);

/* Objective metrics of the reference's metrics dict between two device images [3][H][W]
 * (R, G, B planes, unit range, f16 or f32): out3 = { PSNR dB, SSIM, dE-ITP } as _psnr_bgr / _ssim_bgr /
 * _delta_e_itp_bgr compute them (src/gui_objective_metrics.py:438-528; peak_nits = HDRTVNET_OBJECTIVE_HDR_PEAK_NITS,
 * 1000).  Synchronises `stream` (the three numbers come back to the host).  Parity UNPINNED: that module needs
 * cv2; the arithmetic is oracle/metrics_oracle.py's restatement. */
int hdrtv_metrics(hdrtv_ctx *ctx, void *stream, const void *dev_a, const void *dev_b, int dtype, int H, int W,
                  float peak_nits, double *out3);

/* Full-reference metrics as the reference reports them (_compute_full_reference_metrics, src/gui_objective_metrics.py:617-677; its
 * live path, gui_pipeline_worker_objective.py:60-73, is the same without CROP and NORMALIZED): between two RGB48 frames in device
 * memory, u16 [H][W][3] R, G, B -- the codes hdrtv_post_rgb48* writes -- of the same size.  Bringing the ground truth to that size
 * and layout is the caller's.  Integer stages are rules the device meets bit for bit (tests/metrics_full_ref.py restates them in
 * numpy); the float stages are hdrtv_metrics' arithmetic.
 *  R1 (flag HDRTV_FR_CROP) shared border bounds.  A pixel is signal when max(R, G, B) >= 132 (the reference's threshold
 *     max(2, 65535 * 0.002) = 131.07, compared with >).  hdrtv_rgb48_border_counts writes u32 [2][H + W]: per frame the signal
 *     pixels of each row, then of each column (the record is zeroed on `stream` first; integer adds only).  On the host, with
 *     round() Python's (half to even): a row has signal when its count >= max(4, round(0.01 * W)), a column when >=
 *     max(4, round(0.01 * H)); a frame's bounds are its first and last such row and column, or none when there is none or fewer
 *     than 2 remain on an axis; both present: the intersection, one: that one, neither: no crop.  The crop applies when the largest
 *     of the four margins is >= 8 and at least 2 x 2 remains.
 *  R2 evaluation size.  (h, w) the size after the crop; if max(h, w) > max_side: scale = max_side / max(h, w),
 *     nw = max(2, round(w * scale)), nh = max(2, round(h * scale)); else the frames are read as they are.  The reference's
 *     max_side is 512.
 *  R3 16-bit INTER_AREA, hdrtv_rgb48_area_reduce: the rectangle (x0, y0, rw, rh) of src -> dst u16 [nh][nw][3]; the crop is an
 *     offset into the source, no cropped copy exists.  It is oracle/letterbox_oracle.resize_area on 16-bit codes:
 *       both ratios exactly 2: (a + b + c + d + 2) >> 2;
 *       both ratios another integer: rint(float32(sum) * float32(1 / area)), clipped to 65535;
 *       anything else (one integer and one fractional axis included): computeResizeAreaTab's float32 weights, built in double;
 *         horizontal sums buf = buf + s * alpha from 0 in table order, vertically out = beta * buf for the first entry and
 *         out = out + beta * buf after it, float32 with multiply and add separate; rint (half to even), clipped to 0 .. 65535.
 *     1 <= nh <= rh <= 16 nh and 1 <= nw <= rw <= 16 nw (7680 -> 512 is 15x; up to 16x an integer block sum stays below 2^24 and
 *     is the same number in int and in float32); anything else is HDRTV_EINVAL with nothing written.  Parity with OpenCV's own
 *     16-bit resize is UNPINNED, as for the 8-bit rule: OpenCV is not part of the reference tree.
 *  R4 raw metrics: hdrtv_metrics' three formulas on float32(code) / 65535.0f (a true division, _to_unit_float), read from the
 *     interleaved evaluation frames -> out6[0..2].
 *  R5 (flag HDRTV_FR_NORMALIZED) channel statistics, hdrtv_rgb48_grade_match: six exact histograms (2 frames x 3 channels x 65536
 *     u32 bins, integer atomics); per histogram of N samples, in float64 and ascending code order,
 *       mean = sum(h[c] * x_c) / N,  std = sqrt(sum(h[c] * (x_c - mean)^2) / N)
 *     with x_c = c (codes) or x_c = v(c) = float32(clip(float32(c) / 65535, 0, 1) * peak_nits) (absolute RGB); per channel and
 *     domain gain = 1 if std_pred < 1e-6 else std_ref / std_pred, bias = mean_ref - gain * mean_pred, both then rounded to
 *     float32.  out12 = gain[3], bias[3] (codes), gain[3], bias[3] (absolute RGB).  This replaces the reference's float32
 *     np.mean / np.std, whose pairwise summation order is numpy's own (DESIGN.md has the measured distance).
 *  R6 normalised metrics -> out6[3..5] (zero without the flag): for PSNR and SSIM the prediction's code becomes
 *     trunc(clip(float32(code) * gain + bias, 0, 65535)) (float32, multiply and add separate; the reference's .astype(uint16)),
 *     then R4; for dE-ITP its absolute RGB becomes clip(v * gain + bias, 0, max(1, peak_nits)) with the second pair, before PQ.
 *     Both happen where the metric kernel loads: one more launch, no normalised frame in memory.
 * info = {top, bottom, left, right, eval_h, eval_w}: the rows [top, bottom) and columns [left, right) that were scored -- the whole
 * frame when nothing was cropped -- and the evaluation size.  hdrtv_full_reference_metrics and hdrtv_rgb48_grade_match bring
 * numbers to the host and synchronise `stream` (the bounds, the histograms and the partial sums each cost a round trip);
 * hdrtv_rgb48_border_counts and hdrtv_rgb48_area_reduce are stream-ordered.  None needs a reservation; scratch and the area tables
 * of a geometry are allocated in the context on first use.  HDRTV_EINVAL, with nothing written, for a NULL pointer, a non-positive
 * size, max_side < 2, peak_nits <= 0, unknown flags, a rectangle that leaves the frame, or a shrink beyond 16x.  Out of scope:
 * HDR-VDP3, pairing and resizing the ground truth, error bars over a stream. */
#define HDRTV_FR_CROP 1
#define HDRTV_FR_NORMALIZED 2
int hdrtv_full_reference_metrics(hdrtv_ctx *ctx, void *stream, const uint16_t *pred_rgb48, const uint16_t *ref_rgb48, int H, int W,
                                 int max_side, float peak_nits, int flags, double *out6, int *info);
int hdrtv_rgb48_border_counts(hdrtv_ctx *ctx, void *stream, const uint16_t *pred_rgb48, const uint16_t *ref_rgb48, int H, int W,
                              uint32_t *dev_counts);
int hdrtv_rgb48_area_reduce(hdrtv_ctx *ctx, void *stream, const uint16_t *src_rgb48, int H, int W, int x0, int y0, int rw, int rh,
                            uint16_t *dst_rgb48, int nh, int nw);
int hdrtv_rgb48_grade_match(hdrtv_ctx *ctx, void *stream, const uint16_t *pred_rgb48, const uint16_t *ref_rgb48, int H, int W,
                            float peak_nits, float *out12);

/* ---- pinned host RGB48 ring: replaces _pinned_u16_host_ring / _acquire_pinned_u16_slot /
 * _PinnedMpvFrame (gui_pipeline_worker_feeders.py:38-70, 125-170).  `slots` in [2,8]
 * (HDRTVNET_FEEDER_GPU_RGB48_RING_FRAMES).  A slot cycles free -> acquired -> (kernel writes its device
 * buffer; commit = hipMemcpyAsync to the pinned host buffer + event) -> waited -> released. */
int hdrtv_ring_create(hdrtv_ctx *ctx, int slots, int H, int W);
/* Returns the slot index (>=0), its pinned host buffer and its device staging buffer, or HDRTV_ESTATE when no
 * slot frees up within timeout_ms (reference: 250 ms, feeders.py:166). */
int hdrtv_ring_acquire(hdrtv_ctx *ctx, int timeout_ms, uint16_t **host_ptr, uint16_t **dev_ptr);
/* After hdrtv_post_rgb48 into the slot's dev_ptr: enqueues the device -> pinned-host copy on `stream` and records
 * the slot's ready event behind it. */
int hdrtv_ring_commit(hdrtv_ctx *ctx, int slot, void *stream);
/* hdrtv_ring_commit copying only the first `bytes` of the slot: a Y'CbCr frame (hdrtv_ycbcr10_bytes) fits an RGB48 slot, and only its
 * bytes cross PCIe.  0 < bytes <= H * W * 6 of hdrtv_ring_create, else HDRTV_EINVAL (the slot stays acquired). */
int hdrtv_ring_commit_bytes(hdrtv_ctx *ctx, int slot, void *stream, size_t bytes);
/* Blocks the calling host thread until the slot's contents are complete (wait_ready). */
int hdrtv_ring_wait(hdrtv_ctx *ctx, int slot);
/* Marks the slot free again (payload.release()). */
int hdrtv_ring_release(hdrtv_ctx *ctx, int slot);
int hdrtv_ring_destroy(hdrtv_ctx *ctx);

/* ---- introspection for parity tests and profiling (no reference counterpart) ----------
 * Looks up an internal activation by name after hdrtv_infer (e.g. "le.cond1", "hg.conv4_2").
 * layout: 0 = NHWC f16, 1 = planar CHW f16, 2 = planar CHW f32, 3 = f32 vector.
 * An hg.* tensor always comes back whole.  With variant hg_sparse (the default) a frame computes only the tiles of the HG head that
 * its highlight mask lets reach the output; when lane 0's last frame ran that way, hdrtv_get_tap first runs the head's layers
 * once more over every tile (from the hg.img still in the workspace, without the blend, on that frame's stream; synchronise
 * before reading) and then returns the pointer.  Taps are a debugging surface: the frame path never takes them. */
int hdrtv_get_tap(hdrtv_ctx *ctx, const char *name, void **dev_ptr, int *C, int *H, int *W,
                  int *layout);
/* Number of kernel launches one hdrtv_infer issues at the reserved size, and the algorithmic
 * multiply-accumulates of Conv2d/Linear layers per frame. */
int hdrtv_infer_stats(hdrtv_ctx *ctx, int *launches, double *macs);

/* Per-launch timing of hdrtv_infer with HIP events on the launch stream (bench.py roofline).
 * While enabled, every hdrtv_infer records one event after each kernel launch; interval i is
 * launch i (plus its launch gap).  hdrtv_profile_get(ctx, -1, ...) returns the number of launches
 * recorded by the last hdrtv_infer; index i returns the layer name, the kernel (template
 * instance) name, its duration in ms, its algorithmic MACs and its algorithmic bytes
 * (activations in + out + residuals + weights, each counted once). */
int hdrtv_profile_enable(hdrtv_ctx *ctx, int on);
int hdrtv_profile_get(hdrtv_ctx *ctx, int i, const char **layer, const char **kernel, float *ms, double *macs,
                      double *bytes);
/* Launch i of the last profiled hdrtv_infer: the tiles it computed (the count of its need list, variant hg_sparse, read back
 * from the device once the frame has finished) and the tiles of a dense launch.  *total = 0: the launch had no list, or its
 * list was dropped and it ran every tile.  hdrtv_profile_get scales the MACs and bytes of a conv_prw launch by executed /
 * total; for the other listed kernels (conv1 on conv_c3<64,dot3>, conv_pglds, conv_glds1) it keeps the dense layer's, and this
 * is their executed work. */
int hdrtv_profile_tiles(hdrtv_ctx *ctx, int i, int *executed, int *total);

/* Developer / test switch with no reference counterpart: selects which of several equivalent kernels or schedules a
 * layer runs on (e.g. "le_rows": 1 = the fused row-streaming LE kernels, 0 = one launch per layer).  The table is
 * filled at hdrtv_create (defaults, then the creating process's HDRTV_VARIANTS="name=value,..."); the launch path never
 * reads the environment.  Takes effect at the next hdrtv_infer; HDRTV_EINVAL for an unknown name.
 * "hg_sparse" (default 2; fp16 HG, hdrtv_infer and hdrtv_infer_lane alike): every layer of the HG head, conv1 to Up_conv5 (conv1 on
 * conv_c3<64,dot3>, conv_prw, conv_pglds and the 1x1 fuse convs on conv_glds1), computes only the tiles a masked output pixel
 * depends on -- the lists are built on the device from the frame's mask (no host round trip; the launch
 * grids do not depend on frame content) -- and the blend takes img where the mask is 0.  2 tracks the dependency in sub-tile
 * units with a one-pixel halo per 3x3 layer, 1 in 16x16 cells of every level (coarser: more tiles).  Output bit-identical to 0
 * (every tile) for finite HG values; see hdrtv_get_tap for the taps.  hdrtv_infer_stats keeps reporting the dense model's MACs. */
int hdrtv_set_variant(hdrtv_ctx *ctx, const char *name, int value);
int hdrtv_get_variant(hdrtv_ctx *ctx, const char *name, int *value);

const char *hdrtv_last_error(const hdrtv_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* HDRTV_MI355X_H */
