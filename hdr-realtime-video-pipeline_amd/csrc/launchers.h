// launchers.h -- host-callable launch wrappers defined in the .hip kernel files.
#pragma once
#include "common.h"

// One-time per-kernel setup (hipFuncSetAttribute) is a property of (function, device), not of the process: a process
// that holds contexts on several devices must repeat it on each.  Races are benign (the setup is idempotent).
struct DevOnce {
    unsigned char set[64] = {};
    static int cur() { int d = 0; return hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64 ? d : 0; }
    bool need() const { return !set[cur()]; }
    void done() { set[cur()] = 1; }
};
// A kernel with more than 64 KiB of dynamic LDS has to be told so once.  `once` is the call site's own static DevOnce: one per
// kernel instantiation.
template <class K> hipError_t allow_lds(DevOnce &once, K kern, int bytes)
{
    if (!once.need()) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) once.done();
    return e;
}

hipError_t conv_igemm_launch(ConvParams p, int cin_t, int bn, int ks, int stride, hipStream_t stream);
hipError_t conv_glds1_launch(ConvParams p, hipStream_t stream, int n_cu = 0, bool old_form = false, bool *list_taken = nullptr);   // n_cu >= 8: the persistent form
hipError_t conv_pglds_launch(ConvParams p, int n_cu, hipStream_t stream, bool *list_taken = nullptr);
hipError_t conv_prw_launch(ConvParams p, int th, int n_cu, hipStream_t stream, bool *list_taken = nullptr);   // Cout % 256 == 0, modes NHWC / PS / POOL; th = 16 | 8
hipError_t conv_pglds_i8_launch(ConvI8Params p, int n_cu, hipStream_t stream);
hipError_t conv_prw_i8_launch(ConvI8Params p, int th, int n_cu, hipStream_t stream);   // Cin % 128 == 0, Cout % 256 == 0, int8 out
hipError_t conv1x1_i8_launch(ConvI8Params p, hipStream_t stream);
hipError_t conv32p_launch(Conv32Params p, int n_cu, hipStream_t stream, int nw = 0);
hipError_t conv32s_launch(Conv32Params p, int n_cu, hipStream_t stream, bool nosplit = false);   // the single-pass (CoutPad == 32) layers
hipError_t le_rb_rows_launch(RowsRbParams p, int n_cu, hipStream_t stream);   // fused ResBlock_with_SFT, row-streaming (le_rows.hip)
hipError_t le_rb_rows_i8_launch(RowsRbI8Params p, int n_cu, hipStream_t stream);   // ... every layer W8A8 on int8 MFMA (le_rows_i8.hip)
hipError_t le_tail_rows_i8_launch(RowsTailI8Params p, int n_cu, hipStream_t stream);
hipError_t le_head_rows_i8_launch(RowsHeadI8Params p, int n_cu, hipStream_t stream);
hipError_t le_tail_rows_launch(RowsTailParams p, int n_cu, hipStream_t stream);   // up_conv3 .. conv_last in one launch (le_rows.hip)
hipError_t le_head_rows_launch(RowsHeadParams p, int n_cu, hipStream_t stream);   // conv_first .. down_conv1 in one launch (le_rows.hip)
hipError_t conv_t16_launch(ConvParams p, hipStream_t stream, int n_cu);
hipError_t conv_q8_launch(ConvQ8Params p, hipStream_t stream, int n_cu);
hipError_t conv_q8_multi_launch(ConvQ8MultiParams p, int n_cu, hipStream_t stream);
hipError_t conv3x3s2_preg_launch(ConvParams p, int n_cu, hipStream_t stream);

hipError_t pre_unpack_launch(const uint8_t *bgr, f16 *out, int H, int W, hipStream_t s);
// The six resize-table pointers of a reserved size (ATen's _upsample_bicubic2d_aa taps: lane 0's workspace entries "aa.*")
struct AaTables {
    const float *wx;
    const int *xmn, *xns;
    const float *wy;
    const int *ymn, *yns;
};
hipError_t cond_resize_launch(const f16 *in, f16 *out, int H, int W, int Ho, int Wo, const AaTables &t, hipStream_t s);
hipError_t pre_fused_launch(const uint8_t *bgr, f16 *out, f16 *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s);
hipError_t post_u8_launch(const void *in, int is_f32, int H, int W, uint8_t *bgr, hipStream_t s);
hipError_t post_rgb48_launch(const void *in, int is_f32, int H, int W, uint16_t *rgb, int pq, float peak, hipStream_t s,
                             const float *pq_bnd = nullptr);

// activation fake-quantiser of a W8A8 layer evaluated in fp32 (classifier convs, Linear heads): on = 0 passes x through
struct FakeQ { int on; float inv, zoff, scale, zero; };
hipError_t cls_block_launch(const void *in, int in_f16, int Ci, int Hi, int Wi, const float *nmean, const float *nrstd,
                            const float *ngamma, const float *nbeta, const float *Wt, const float *bias, int Co, float *out,
                            int Ho, int Wo, float *part, hipStream_t s, const FakeQ *qin = nullptr, const FakeQ *qstat = nullptr,
                            int *nblk = nullptr);
hipError_t cls_stats_launch(const float *part, int C, int nblk, int n, float eps, float *mean, float *rstd, hipStream_t s);
struct AgcmFoldArgs {
    const float *mean5;
    const float *w20, *b20;
    const float *ws[3], *bs[3], *wt[3], *bt[3];
    const float *w1, *b1, *w2, *b2, *w3, *b3;
};
hipError_t agcm_fold_launch(const AgcmFoldArgs &a, f16 *frags, float *biasbuf, hipStream_t s);
hipError_t agcm_mlp_launch(const f16 *in, f16 *out, size_t npix, const f16 *frags, const float *biasbuf, hipStream_t s);

hipError_t conv_c3_launch(const f16 *in, int H, int W, const f16 *wfrag, const float *scale, const float *shift, int cout,
                          int act, f16 *out, f16 *out_pool, int n_cu, hipStream_t s, float pool_q_inv = 0.f, float pool_q_zero = 0.f,
                          const f16 *w2frag = nullptr, float *part2 = nullptr,    // HG.conv1: + conv10's second half per pixel (f32 [H][W][4])
                          const int *tile_list = nullptr, bool *list_taken = nullptr);   // ... over the listed 8 x 32 tiles only (hg_need.hip)
// LE.conv_first as a W8A8 layer: int8 A fragments [2][64 lanes][16 B] (K = (ky | kx4, c4)), scale[32], shift[16 border classes][32]
hipError_t conv_c3_q8_launch(const f16 *in, int H, int W, const int8_t *wq, const float *scale, const float *shift, float q_inv,
                             float q_zoff, int act, f16 *out, int n_cu, hipStream_t s);
// pool_q_inv > 0: out_pool holds int8 codes clamp(rint(v * pool_q_inv + pool_q_zero), -128, 127), COUT bytes per pixel
// last layer of a fused chain as a W8A8 layer: int8 weight fragments [2][64 lanes][16 B], ss = scale[32] | shift[32]
struct QLastArgs {
    const int8_t *wq;
    const float *ss;
    float q_inv, q_zoff;
};
hipError_t le_cond_trunk_launch(const f16 *img, int H, int W, const f16 *wfrag, const float *bias, f16 *cond, f16 *cond1,
                                int n_cu, hipStream_t s, const QLastArgs *q6 = nullptr);
hipError_t cond_tail_launch(const f16 *x, int x_stride, size_t npx, const f16 *wfrag, const float *bias, f16 *out, int n_cu,
                            hipStream_t s, const QLastArgs *q2 = nullptr);
// ---- fully quantised (W8A8) per-pixel chains (le_chain_q8.hip); layouts documented there
struct TrunkQ8Args {
    const int8_t *wfrag;           // [20][64 lanes][16 B]
    const float *consts;           // [1664]
    float q1_inv, q1_zoff, q4_inv;
    float zoff[5];
};
hipError_t le_cond_trunk_q8_launch(const f16 *img, int H, int W, const TrunkQ8Args &a, f16 *cond, f16 *cond1, int n_cu, hipStream_t s);
hipError_t cond_tail_q8_launch(const int8_t *x, size_t npx, const int8_t *wfrag, const float *consts, float zoff2, f16 *out, int n_cu,
                               hipStream_t s);
hipError_t agcm_mlp_q8_launch(const f16 *in, f16 *out, size_t npix, const int8_t *wfrag, const float *consts, float q1_inv, float q1_zoff,
                              float zoff2, float zoff3, hipStream_t s);
hipError_t planar3_to_q8_launch(const f16 *in, size_t npix, float inv, float zoff, int8_t *out, hipStream_t s);
struct AgcmFoldQ8Args {
    FakeQ q20, qlin[6];            // model.20; cond_scale_{first,HR,last}, cond_shift_{first,HR,last}
    const float *P, *Q;            // [3][64] each: x_scale * w_scale[m]; w_scale[m] * (128 x_scale + x_zero) * sum(w) + bias[m]
    float inv2, inv3;              // 1 / x_scale of HRconv and conv_last
    float *consts;                 // out: 320 per-frame constants of agcm_mlp_q8
};
hipError_t agcm_fold_q8_launch(const AgcmFoldArgs &a, const AgcmFoldQ8Args &q, float *biasbuf, hipStream_t s);
// flags: null, or one byte per 16x16 cell of the padded frame ([ceil(Hp/16)][ceil(Wp/16)]), set to 1 where the cell holds a masked
// pixel inside H x W (never cleared here: hg_need consumes them)
hipError_t hg_prep_launch(const f16 *base, int H, int W, int Hp, int Wp, f16 *img_pad, uint8_t *mask, float r, float thresh,
                          hipStream_t s, uint8_t *flags = nullptr);
// ---- hg_need.hip: the HG layers' need lists from hg_prep's flags.  Everything lies in one buffer (`base` + byte offsets).
constexpr int HG_NEED_MAX_LAYERS = 24, HG_NEED_MAX_TENSORS = 32, HG_NEED_LEVELS = 6;
// The need maps' unit per level (0 = full resolution .. 5 = 1/32), as log2 of its side in pixels of that level, per setting of
// variant hg_sparse.  Level 0 is hg_prep's flags (16x16).  1: one 16x16 cell everywhere; 2: 4, 2, 1, 1, 1 pixels at levels 1 .. 5,
// i.e. 8, 8, 8, 16, 32 full-resolution pixels.  No unit is larger than a kernel tile (16).
constexpr int hg_need_unit_log2[3][HG_NEED_LEVELS] = {{4, 4, 4, 4, 4, 4}, {4, 4, 4, 4, 4, 4}, {4, 2, 1, 0, 0, 0}};
struct HgNeedLayer {
    int level, mode, ks;       // input level; 0 writes at its level, 1 pool-fused (one level down), 2 pixel shuffle (one level up)
    int in, skip, out;         // tensor ids (skip < 0: none)
    int in_first, skip_first;  // this layer is the last reader in launch order (the first hg_need sees): it stores the map, others OR
    int out_chained;           // out is the input of the next layer in launch order (the last layer: out is the flags' map) ...
    int in_chained;            // ... in is the output of the layer before: the map may be handed on in the kernel's LDS
    int th, tw;                // the kernel tiles the list is written for: 16 or 8 rows of 16 pixels (tw = 0 or 16), or of 32 (conv_c3: 8 x 32)
    int list_off;              // int [0] count, [1 ..] tile indices ty * ceil(W_level / tw) + tx, ascending
};
struct HgNeedParams {
    unsigned char *base;
    int Hp, Wp, n_layers;
    int lu[HG_NEED_LEVELS];                 // the unit table in use
    int flags_off;                          // hg_prep's flags, one byte per 16x16 full-resolution cell
    int flags_map;                          // the tensor whose need map the flags are (Up_conv5's sums)
    int kbits_off, tbits_off, scratch_words;    // two scratch maps for layers too large for the kernel's LDS
    int map_off[HG_NEED_MAX_TENSORS];       // need map of tensor t: bit rows, 64 units per 64-bit word, ceil(units / 64) words per row
    HgNeedLayer L[HG_NEED_MAX_LAYERS];      // launch order
};
hipError_t hg_need_launch(const HgNeedParams &p, hipStream_t s);
struct HgFinalFusedArgs {
    const f16 *img;
    const uint8_t *mask;
    const float *part;
    const f16 *wfrag;
    const float *scale, *shift, *b10, *wl, *bl;
    void *out;
    int out_f32, H, W, Hp, Wp;
};
hipError_t hg_final_fused_launch(const HgFinalFusedArgs &a, int n_cu, hipStream_t s);
// the same tail when conv_c3_launch(..., w2frag, part2) has left conv10's second half per pixel: a per-pixel kernel (a.wfrag, scale, shift unused)
hipError_t hg_final_light_launch(const HgFinalFusedArgs &a, const float *part2, hipStream_t s);
hipError_t letterbox_launch(const LetterboxParams &p, hipStream_t s);
hipError_t post_scale_launch(const PostScaleParams &p, int is_f32, int pq, hipStream_t s);
// the same with anti-ringing of strength antiring / 256, 1 .. 256 (post_scale_ar.hip; the rule: include/hdrtv_mi355x.h)
hipError_t post_scale_ar_launch(const PostScaleParams &p, int antiring, int is_f32, int pq, hipStream_t s);
// the same with the codes sharpened before the passes: cas = the CAS code 1032 .. 4096, antiring 0 .. 256 (post_scale_cas.hip)
hipError_t post_scale_cas_launch(const PostScaleParams &p, int antiring, int cas, int is_f32, int pq, hipStream_t s);
// quantise + FSR upscale (post_fsr.hip): EASU alone (rcas = 0) or EASU + RCAS with sharp = float32(2^-sharpness), 0.25 .. 1;
// hipErrorInvalidValue, nothing enqueued, unless 1 <= H <= dH <= 2H and 1 <= W <= dW <= 2W; pq != 0 needs p.pq_bnd
hipError_t post_fsr_launch(const PostFsrParams &p, int rcas, float sharp, int is_f32, int pq, hipStream_t s);
// the film grain of include/hdrtv_mi355x.h, 0 < intensity <= 0.1 and 0 <= seed < 1 (film_grain.h has the pixel rule); each returns
// hipErrorInvalidValue with nothing enqueued otherwise, and under its twin's conditions.  film_grain.hip: codes -> grained codes
// (dst == src allowed), and tensor -> quant_rgb -> grained codes in one launch
hipError_t film_grain_launch(const uint16_t *src, uint16_t *dst, int H, int W, float intensity, float seed, hipStream_t s);
hipError_t post_rgb48_grain_launch(const void *in, int is_f32, int H, int W, uint16_t *rgb, int pq, float peak, const float *pq_bnd,
                                   float intensity, float seed, hipStream_t s);
// the tone map of include/hdrtv_mi355x.h (post_tonemap.hip): codes -> tone-mapped codes (dst == src allowed), and tensor -> quant_rgb
// -> tone-mapped codes in one launch.  gain: the caller's 65536 floats; lin: resample_tables.h pq_eotf_table; pq_bnd: the PQ code
// boundaries, needed whatever pq is.  hipErrorInvalidValue, nothing enqueued, for a null pointer or H, W < 1
hipError_t rgb48_tonemap_launch(const uint16_t *src, uint16_t *dst, int H, int W, const float *gain, const float *lin, const float *pq_bnd,
                                hipStream_t s);
hipError_t post_rgb48_tonemap_launch(const void *in, int is_f32, int H, int W, uint16_t *rgb, int pq, float peak, const float *gain,
                                     const float *lin, const float *pq_bnd, hipStream_t s);
// post_scale_grain.hip: the Lanczos tile with the staged (antiring 0 .. 256; cas 0 or 1032 .. 4096: sharpened) codes grained over H x W
hipError_t post_scale_grain_launch(const PostScaleParams &p, int antiring, int cas, float intensity, float seed, int is_f32, int pq,
                                   hipStream_t s);
// post_fsr_grain.hip: the FSR tile with the final codes grained over dH x dW
hipError_t post_fsr_grain_launch(const PostFsrParams &p, int rcas, float sharp, float intensity, float seed, int is_f32, int pq, hipStream_t s);
// quantise + Mitchell shrink (post_down.hip) with anti-ringing 0 .. 256, and with ssim != 0 the SSimDownscaler correction behind it;
// hipErrorInvalidValue, nothing enqueued, unless 1 <= dH <= H <= 4 dH, 1 <= dW <= W <= 4 dW and 1 <= ntx, nty <= 17; pq != 0 needs p.pq_bnd
hipError_t post_down_launch(const PostDownParams &p, int antiring, int ssim, int is_f32, int pq, hipStream_t s);
// quantise + spline36 enlargement (post_ssimsr.hip), and with ssim != 0 the SSimSuperRes passes behind it; hipErrorInvalidValue,
// nothing enqueued, unless 1 <= H < dH <= 2 H and 1 <= W < dW <= 2 W; pq != 0 needs p.pq_bnd
hipError_t post_ssimsr_launch(const PostSsimsrParams &p, int ssim, int is_f32, int pq, hipStream_t s);
// fmt 0 P010 | 1 yuv420p10 | 2 yuv422p10, siting 0 left | 1 top-left (4:2:0 only); W even, H even for 4:2:0; pq != 0 needs p.pq_bnd
hipError_t post_ycbcr10_launch(const Ycbcr10Params &p, int is_f32, int pq, hipStream_t s);
hipError_t rgb48_to_ycbcr10_launch(const Ycbcr10Params &p, hipStream_t s);
// the same two with the ordered dither of include/hdrtv_mi355x.h (post_ycbcr_dither.hip)
hipError_t post_ycbcr10_dither_launch(const Ycbcr10Params &p, int is_f32, int pq, hipStream_t s);
hipError_t rgb48_to_ycbcr10_dither_launch(const Ycbcr10Params &p, hipStream_t s);
// the same two with Floyd-Steinberg error diffusion (post_ycbcr_fs.hip): a samples launch into `scratch` (ycbcr10_fs_scratch_bytes
// bytes, 4-byte aligned), then the diffusion launch; passes: bit 0 the samples launch, bit 1 the diffusion launch (3 = the conversion)
int64_t ycbcr10_fs_scratch_bytes(int fmt, int H, int W);       // negative for a bad argument
hipError_t post_ycbcr10_fs_launch(const Ycbcr10Params &p, int is_f32, int pq, void *scratch, int passes, hipStream_t s);
hipError_t rgb48_to_ycbcr10_fs_launch(const Ycbcr10Params &p, void *scratch, int passes, hipStream_t s);
// hipErrorInvalidValue, nothing enqueued, unless H, W >= 1, range in 1 .. DB_HALO, threshold in 1 .. 65535 and src != dst
hipError_t rgb48_deband_launch(const DebandParams &p, hipStream_t s);
// zero the record on `s`, then one kernel over the rectangle on at most max_wgs workgroups (the record does not depend on the grid);
// hipErrorInvalidValue, nothing enqueued, unless the rectangle lies in the frame and p.stats is 8-byte aligned; pq != 0 needs p.pq_bnd
hipError_t light_stats_launch(const LightStatsParams &p, int is_f32, int pq, int max_wgs, hipStream_t s);
hipError_t rgb48_light_stats_launch(const LightStatsParams &p, int max_wgs, hipStream_t s);
hipError_t metrics_launch(const MetricsParams &p, hipStream_t s);
int metrics_blocks(int H, int W);
// the same kernel on two u16 [H][W][3] RGB48 frames through its CodeLoad policy (p.pitch, p.norm and the gains; R4 / R6 of
// include/hdrtv_mi355x.h); hipErrorInvalidValue, nothing enqueued, unless H, W >= 1 and pitch >= 3 W
hipError_t metrics_u16_launch(const MetricsParams &p, hipStream_t s);
// the full-reference chain (metrics_full.hip).  Each launcher returns hipErrorInvalidValue with nothing enqueued for a null pointer
// or a size its kernel does not take; border_counts_launch and channel_hist_launch zero their record on `s` first
hipError_t border_counts_launch(const BorderCountsParams &p, hipStream_t s);
bool area_reduce_size_ok(int sh, int sw, int nh, int nw);     // 1 <= nh <= sh <= FR_MAX_SHRINK nh, likewise the widths
hipError_t area_reduce_launch(const AreaReduceParams &p, hipStream_t s);
hipError_t channel_hist_launch(const ChannelHistParams &p, hipStream_t s);
// host side of R5: hist u32 [2][3][65536] of n samples each -> gain[3], bias[3], gain_abs[3], bias_abs[3] as float32
void grade_match_host(const uint32_t *hist, double n, float peak_nits, float *out12);

// precision="fp32" (fp32_ops.hip)
hipError_t conv_f32_launch(const F32ConvParams &p, int ks, int stride, int n_cu, hipStream_t s);
bool conv_f32_on_mfma(const F32ConvParams &p, int ks, int n_cu);      // whether conv_f32_launch runs a stride-1 layer on the fp32 matrix pipe
hipError_t ew_f32_launch(int op, const float *a, const float *b, const float *c, float *y, size_t n, hipStream_t s);
hipError_t avgpool3s2_leaky_f32_launch(const float *x, float *y, int C, int H, int W, float slope, hipStream_t s);
hipError_t instnorm_f32_launch(float *x, const float *gamma, const float *beta, int C, int n, float eps, hipStream_t s);
hipError_t plane_mean_f32_launch(const float *x, float *y, int C, int n, hipStream_t s);
hipError_t gfm_heads_f32_launch(const F32GfmParams &p, hipStream_t s);
hipError_t maxpool2_f32_launch(const float *x, float *y, int C, int H, int W, hipStream_t s);
hipError_t window_f32_launch(const float *x, float *y, int C, int H, int W, int Ho, int Wo, int mode, hipStream_t s);
hipError_t hg_mask_f32_launch(const float *base, float *mask, size_t npix, float r, hipStream_t s);
hipError_t hg_blend_f32_launch(const float *t, const float *img, const float *mask, float *out, int H, int W, int Hp, int Wp,
                               hipStream_t s);
hipError_t pre_f32_launch(const uint8_t *bgr, float *rgb, float *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s);
// the condition-map half of pre_f32_launch on its own (planar fp32 RGB -> cond): the Y'CbCr routes unpack with their own kernels
hipError_t cond_resize_f32_launch(const float *rgb, float *cond, int H, int W, int Ho, int Wo, const AaTables &t, int mode, hipStream_t s);
