// api_graph.hip -- launch sequencing of one hdrtv_infer: AGCM, LE and HG layer by layer (struct Seq: api.h).
#include "api.h"

namespace hdrtv_host {

// ----------------------------------------------------------------------- Seq: one launch per call, counted, checked, profiled
void Seq::conv(const std::string &key, const f16 *src0, int c0, const f16 *src1, int c1, int Hi, int Wi, int act, int mode, f16 *dst, int dstC, int Hd, int Wd, const f16 *res1, const f16 *res2, f16 *dst_full, f16 *dst_planar, const f16 *res_planar, const float *dotw, float *dst_dot, int s0_stride)
{
    if (!ok()) return;
    auto it = c->conv.find(key);
    if (it == c->conv.end()) { rc = fail(c, HDRTV_ESTATE, "no packed conv %s", key.c_str()); return; }
    const ConvLayer &L = it->second;
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.src0 = src0; p.src1 = src1; p.c0 = c0; p.c1 = c1;
    p.s0_stride = s0_stride ? s0_stride : c0; p.s1_stride = c1;
    p.Hi = Hi; p.Wi = Wi;
    const int pad = L.ks / 2;
    p.Ho = (Hi + 2 * pad - L.ks) / L.stride + 1;
    p.Wo = (Wi + 2 * pad - L.ks) / L.stride + 1;
    p.wpk = wtp<f16>(c, L.wpk); p.scale = wtp<float>(c, L.scale); p.shift = wtp<float>(c, L.shift);
    p.CoutPad = L.coutPad; p.Cout = L.cout; p.act = act; p.mode = mode;
    p.dst = dst; p.dst_full = dst_full; p.dstC = dstC; p.Hd = Hd; p.Wd = Wd;
    p.res1 = res1; p.res2 = res2; p.dst_planar = dst_planar; p.res_planar = res_planar;
    p.dotw = dotw; p.dst_dot = dst_dot;
    if (c0 + c1 != L.cin) { rc = fail(c, HDRTV_ESTATE, "conv %s: channel mismatch", key.c_str()); return; }
    p.zeros = wtp<f16>(c, c->zeros_off);
    p.tail_w = tail_w; p.tail_b = tail_b; p.tail_s = tail_s; p.tail_out = tail_out;
    tail_w = nullptr; tail_b = nullptr; tail_s = nullptr; tail_out = nullptr;
    p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
    // a need list set for this launch (run_hg): consumed here; only a kernel with the list's tile geometry takes it (conv_prw: 16 or 8
    // rows, conv_pglds and conv_glds1: 16)
    const int *const need = need_list;
    const int need_rows = need_th, need_cells = need_total;
    need_list = nullptr; need_th = 0; need_total = 0;
    const int nt_slow = c->var.at("pglds_nt_slow");
    // default: the Up convs (Cout = 4 Cin: 4 .. 16 Cout-tiles per pixel tile) walk Cout-tile slowest -- an XCD then shares one
    // weight slab instead of re-fetching up to 16 (-17 % L2 misses, profiles/r02_pmc_traffic_tile_order.json); the other
    // layers walk it fastest so that the blocks of an XCD share halo tiles (+45 .. +75 % misses the other way round)
    p.nt_slow = nt_slow == 3 ? (mode == ST_PS) : (nt_slow == 2 ? (L.coutPad >= 512) : nt_slow);
    // the kernel, chosen once: the tag and the launch below both follow `route`
    enum { T16, S2G, PRW, PGLDS, GLDS1, IGEMM } route = IGEMM;
    int prw_th = 0;
    const bool g64 = L.stride == 1 && L.cin_t == 64 && L.bn == 128 && !res1 && !res2 && !dst_full && mode != ST_PLANAR3;
    const bool no_t16 = c->var.at("no_t16") != 0;                         // developer A/B: the generic implicit-GEMM kernel
    if (!no_t16 && L.ks == 3 && L.stride == 2 && L.cin == 32 && L.coutPad == 32 && !src1 && mode == ST_NHWC && !res1 && !res2)
        route = T16;
    else if (L.ks == 3 && L.stride == 2 && L.cin_t == 64 && L.bn == L.coutPad && (L.coutPad == 64 || L.coutPad == 192))
        route = S2G;
    else if (g64 && L.ks == 3 && L.cout == L.coutPad) {                   // HG 3x3 convs: persistent LDS-DMA kernel
        // Cout a multiple of 256: the private-weight schedule (conv3x3_prw.hip); Up_conv5 (ST_PS_DOT3) only at 256, always 16 rows
        prw_th = prw_tile_rows(c, mode, L.coutPad, p.Ho, p.Wo);
        route = prw_th ? PRW : PGLDS;
    } else if (g64 && L.ks == 1 && mode == ST_NHWC && (c0 + c1) >= 128 && L.coutPad <= 512 && (act == ACT_RELU || act == ACT_NONE))
        route = GLDS1;                                                     // HG 1x1 fuse convs
    // a fused 1x1 tail (run_le sets it and then skips the tail's own launch) exists in conv3x3s2_preg's epilogue only
    if (p.tail_w && route != S2G) { rc = fail(c, HDRTV_ESTATE, "conv %s: a fused CondNet tail was requested but the layer does not run on conv3x3s2_preg", key.c_str()); return; }
    const char *epi = mode == ST_POOL ? "pool" : (mode == ST_PS ? "ps" : (mode == ST_PS_DOT3 ? "ps_dot3" : "nhwc"));
    char tag[64];
    hipError_t e;
    bool list_taken = false;        // the kernel walked the need list (a run too long for its LDS slots runs every tile)
    switch (route) {
    case T16: snprintf(tag, sizeof tag, "conv_t16<32,3,2>"); e = conv_t16_launch(p, s, c->n_cu); break;
    case S2G:
        snprintf(tag, sizeof tag, p.tail_w ? "conv3x3s2_preg<%d>+tail" : "conv3x3s2_preg<%d>", L.coutPad);
        e = conv3x3s2_preg_launch(p, c->n_cu, s);
        break;
    case PRW:
        if (need && need_rows == prw_th) p.tile_list = need;
        snprintf(tag, sizeof tag, "%s<%s>", prw_th == 8 ? "conv_prw8" : "conv_prw", epi);
        e = conv_prw_launch(p, prw_th, c->n_cu, s, &list_taken);
        break;
    case PGLDS:
        if (need && need_rows == 16) p.tile_list = need;
        snprintf(tag, sizeof tag, "conv_pglds<%s>", epi);
        e = conv_pglds_launch(p, c->n_cu, s, &list_taken);
        break;
    case GLDS1:
        if (need && need_rows == 16) p.tile_list = need;
        snprintf(tag, sizeof tag, "conv_glds1");
        e = conv_glds1_launch(p, s, c->n_cu, c->var.at("glds1_old") != 0, &list_taken);
        break;
    default:
        snprintf(tag, sizeof tag, "conv_igemm<%d,%d,%d,%d>", L.cin_t, L.bn, L.ks, L.stride);
        e = conv_igemm_launch(p, L.cin_t, L.bn, L.ks, L.stride, s);
    }
    double macs = (double)p.Ho * p.Wo * L.cin * L.ks * L.ks * L.cout;
    double bytes = 2.0 * Hi * Wi * L.cin + 2.0 * L.ks * L.ks * L.cin * L.coutPad;
    if (p.tail_w) {                 // a fused 1x1 tail: + its MACs, 16 channels out instead of the 64 it consumes
        macs += (double)p.Ho * p.Wo * (p.tail_s ? 64 * 16 : 64 * 64 + 64 * 16);
        bytes -= 2.0 * p.Ho * p.Wo * (64 - 16);
    }
    const double outel = mode == ST_POOL ? (double)Hd * Wd * L.cout + (dst_full ? (double)p.Ho * p.Wo * L.cout : 0.0)
                                          : (mode == ST_PLANAR3 ? 3.0 * Hd * Wd
                                                                : (mode == ST_PS_DOT3 ? 8.0 * Hd * Wd : (double)p.Ho * p.Wo * L.cout));
    bytes += 2.0 * outel * (1 + (res1 ? 1 : 0) + (res2 ? 1 : 0) + (res_planar ? 1 : 0));
    // the profile scales conv_prw's MACs and bytes by the tiles it walked; the other kernels keep the dense layer's (hdrtv_profile_tiles
    // has their counts)
    chk(e, key.c_str(), tag, macs, bytes, list_taken ? p.tile_list : nullptr, need_cells, route == PRW);
}


void Seq::conv8(const std::string &key, const int8_t *src0, int c0, const int8_t *src1, int c1, int Hi, int Wi, int mode, void *dst, int dstC, int Hd, int Wd, const float *dotw, float *dst_dot)
{
    if (!ok()) return;
    auto it = c->conv8.find(key);
    if (it == c->conv8.end()) { rc = fail(c, HDRTV_ESTATE, "no packed int8 conv %s", key.c_str()); return; }
    const ConvI8Layer &L = it->second;
    if (c0 + c1 != L.cin) { rc = fail(c, HDRTV_ESTATE, "conv %s: channel mismatch", key.c_str()); return; }
    ConvI8Params p;
    memset(&p, 0, sizeof p);
    p.src0 = src0; p.src1 = src1; p.c0 = c0; p.c1 = c1; p.Hi = Hi; p.Wi = Wi; p.Ho = Hi; p.Wo = Wi;
    p.wpk = wtp<int8_t>(c, L.wpk); p.scale = wtp<float>(c, L.scale); p.shift = wtp<float>(c, L.shift);
    p.Cout = L.cout; p.mode = mode; p.out_f16 = L.out_f16; p.dst = dst; p.dstC = dstC; p.Hd = Hd; p.Wd = Wd;
    p.padline = wtp<int8_t>(c, L.padline);
    p.delta = L.has_delta ? wtp<float>(c, L.delta) : nullptr;
    p.delta_acc = L.has_delta ? wtp<int>(c, L.delta_acc) : nullptr;
    p.lo_clamp = L.lo_clamp;
    p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
    p.dotw = dotw; p.dst_dot = dst_dot;
    char tag[64];
    if (L.ks == 3) snprintf(tag, sizeof tag, "conv_pglds_i8<%s%s>", mode == ST_POOL ? "pool" : (mode == ST_PS ? "ps" : (mode == ST_PS_DOT3 ? "ps_dot3" : "nhwc")), c0 == 64 ? ",c64" : "");
    else snprintf(tag, sizeof tag, "conv1x1_i8%s", L.out_f16 ? "<f16>" : "");
    const double macs = (double)Hi * Wi * L.cin * L.ks * L.ks * L.cout_real;
    const double outel = mode == ST_POOL ? (double)Hd * Wd * L.cout_real : (double)Hi * Wi * L.cout_real;
    const double bytes = (double)Hi * Wi * L.cin + (double)L.ks * L.ks * L.cin * L.cout +
                         (mode == ST_PS_DOT3 ? 16.0 * Hd * Wd : outel * (L.out_f16 ? 2.0 : 1.0));
    // the private-weight schedule (conv3x3_prw_i8.hip) and its tile shape, picked as for the fp16 layers (Seq::conv)
    const int prw_mode = c->var.at("prw");
    int prw_th = prw_mode != 0 && L.ks == 3 && c0 != 64 && (L.cout % 256) == 0 && mode != ST_PS_DOT3 && !L.out_f16
                     ? prw_rows(prw_mode, Hi, Wi, L.cout, c->n_cu) : 0;
    // variant "prw_i8": 0 = never, 1 = only where the 8-row tiles win (the low-resolution layers), 2 = wherever "prw" selects it
    const int i8_mode = c->var.at("prw_i8");
    if (i8_mode == 0 || (i8_mode == 1 && prw_th != 8)) prw_th = 0;
    const bool prw = prw_th != 0;
    if (prw) snprintf(tag, sizeof tag, "conv_prw%s_i8<%s>", prw_th == 8 ? "8" : "", mode == ST_POOL ? "pool" : (mode == ST_PS ? "ps" : "nhwc"));
    chk(L.ks == 3 ? (prw ? conv_prw_i8_launch(p, prw_th, c->n_cu, s) : conv_pglds_i8_launch(p, c->n_cu, s)) : conv1x1_i8_launch(p, s),
        key.c_str(), tag, macs, bytes);
}


void Seq::convq8(const std::string &key, const void *src, bool src_i8, int src_stride, int Hi, int Wi, int act, void *dst, int dstC, const ActQf *oq)
{
    if (!ok()) return;
    auto it = c->q8.find(key);
    if (it == c->q8.end()) { rc = fail(c, HDRTV_ESTATE, "no packed W8A8 conv %s", key.c_str()); return; }
    const QLayer &L = it->second;
    ConvQ8Params p;
    memset(&p, 0, sizeof p);
    p.src = src; p.src_i8 = src_i8 ? 1 : 0; p.Cin = L.cin; p.src_stride = src_stride; p.Hi = Hi; p.Wi = Wi;
    p.ks = L.ks; p.stride = L.stride;
    const int pad = L.ks / 2;
    p.Ho = (Hi + 2 * pad - L.ks) / L.stride + 1; p.Wo = (Wi + 2 * pad - L.ks) / L.stride + 1;
    p.wpk8 = wtp<int8_t>(c, L.wpk8); p.scale = wtp<float>(c, L.scale); p.shift = wtp<float>(c, L.shift);
    p.CoutPad = L.coutPad; p.Cout = L.cout; p.act = act; p.q_inv = L.q.inv(); p.q_zoff = L.q.zoff();
    p.dst = dst; p.dst_i8 = oq ? 1 : 0; p.dstC = dstC;
    if (oq) { p.oq_inv = oq->inv(); p.oq_zoff = oq->zoff(); }
    char tag[64];
    snprintf(tag, sizeof tag, "conv_q8<%d,%d,%d>", L.cin, L.ks, L.stride);
    const double macs = (double)p.Ho * p.Wo * L.cin * L.ks * L.ks * L.cout;
    const double bytes = (double)Hi * Wi * L.cin * (src_i8 ? 1.0 : 2.0) + (double)L.ks * L.ks * L.cin * L.coutPad +
                         (double)p.Ho * p.Wo * L.cout * (oq ? 1.0 : 2.0);
    chk(conv_q8_launch(p, s, c->n_cu), key.c_str(), tag, macs, bytes);
}


void Seq::c3(const std::string &key, const f16 *in, int H, int W, int act, f16 *out, f16 *out_pool, float pool_q_inv, float pool_q_zero, const f16 *w2frag, float *part2, const int *need, int need_tiles)
{
    if (!ok()) return;
    const C3Layer &L = c->c3.at(key);
    // need: HG.conv1's need list (8 x 32 tiles); the profile keeps the dense layer's MACs and bytes (hdrtv_profile_tiles has the count)
    bool list_taken = false;
    const hipError_t e = conv_c3_launch(in, H, W, wtp<f16>(c, L.wfrag), wtp<float>(c, L.scale), wtp<float>(c, L.shift), L.cout, act, out,
                                        out_pool, c->n_cu, s, pool_q_inv, pool_q_zero, w2frag, part2, need, &list_taken);
    chk(e, key.c_str(),
        part2 ? "conv_c3<64,dot3>" : (L.cout == 64 ? "conv_c3<64>" : "conv_c3<32>"), (double)H * W * (27 * L.cout + (part2 ? 192 : 0)),
        (double)H * W * (6.0 + (out ? 2.0 * L.cout : 0.0) + (out_pool ? (pool_q_inv > 0.f ? 0.25 : 0.5) * L.cout : 0.0) + (part2 ? 16.0 : 0.0)),
        list_taken ? need : nullptr, need_tiles, false);
}


void Seq::conv32(const std::string &key, const f16 *src, const f16 *cond, const std::string &sft_key, int H, int W, int act, int mode, f16 *dst, int dstC, int Hd, int Wd, const f16 *res1, const f16 *res2, f16 *dst_planar, const f16 *res_planar, const f16 *c3_img, const std::string &c3_key)
{
    if (!ok()) return;
    auto it = c->conv.find(key);
    auto iq = c->q32.find(key);
    if (it == c->conv.end() && iq == c->q32.end()) { rc = fail(c, HDRTV_ESTATE, "no packed conv %s", key.c_str()); return; }
    const bool i8 = iq != c->q32.end();
    ConvLayer L;
    Conv32Params p;
    memset(&p, 0, sizeof p);
    if (i8) {             // W8A8 layer: int8 MFMA on the quantised tile
        const QLayer &Q = iq->second;
        L.cout = Q.cout; L.coutPad = Q.coutPad;
        p.wpk8 = wtp<int8_t>(c, Q.wpk8); p.scale = wtp<float>(c, Q.scale); p.shift = wtp<float>(c, Q.shift);
        p.q_inv = Q.q.inv(); p.q_zoff = Q.q.zoff();
    } else {
        L = it->second;
        p.wpk = wtp<f16>(c, L.wpk); p.scale = wtp<float>(c, L.scale); p.shift = wtp<float>(c, L.shift);
    }
    p.src = src; p.cond = cond; p.H = H; p.W = W;
    bool sq = false;
    if (cond) {
        const SftLayer &S = c->sft.at(sft_key);
        p.sft_wfrag = wtp<f16>(c, S.wfrag); p.sft_bias = wtp<float>(c, S.bias);
        if (S.q) {        // W8A8 SFT convs: int8 MFMA on the quantised condition pixel
            sq = true;
            p.sq_wfrag = wtp<int8_t>(c, S.qfrag); p.sq_const = wtp<float>(c, S.qconst);
            for (int b = 0; b < 2; ++b) { p.sq_inv[b] = S.inv[b]; p.sq_zoff[b] = S.zoff[b]; p.sq_hzoff[b] = S.hzoff[b]; }
        }
    }
    p.CoutPad = L.coutPad; p.Cout = L.cout; p.act = act; p.mode = mode;
    p.dst = dst; p.dstC = dstC; p.Hd = Hd; p.Wd = Wd; p.res1 = res1; p.res2 = res2;
    p.dst_planar = dst_planar; p.res_planar = res_planar; p.zeros = wtp<f16>(c, c->zeros_off);
    p.dump = reinterpret_cast<f16 *>(stamp_buf());
    const double npx = (double)H * W;
    const double macs = npx * 32 * 9 * L.cout + (cond ? npx * 2 * (16 * 16 + 16 * 32) : 0.0) + (c3_img ? npx * 27 * 32 : 0.0);
    const double outb = mode == ST_PLANAR3 ? 6.0 * npx : 2.0 * npx * L.cout;
    const double bytes = npx * ((c3_img ? 6 : 64) + (cond ? 32 : 0)) + outb * (1 + (res1 ? 1 : 0) + (res2 ? 1 : 0) + (res_planar ? 1 : 0)) +
                         (i8 ? 1.0 : 2.0) * 9 * 32 * L.coutPad;
    p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
    if (c3_img) {         // conv_first fused in front of SFT_layer1 + HR_conv1: src is the planar image
        const C3Layer &L3 = c->c3.at(c3_key);
        p.c3_img = c3_img; p.c3_wfrag = wtp<f16>(c, L3.wfrag);      // bias inside the fragments (pack_c3), no BatchNorm
    }
    // single-pass layers run the one-barrier schedule (conv32s.hip); variant "conv32_old" is the developer A/B switch
    const bool old_sched = c->var.at("conv32_old") != 0;
    const bool one_barrier = L.coutPad == 32 && !old_sched;
    char tag[48];
    snprintf(tag, sizeof tag, "conv32%c<%d,%s%s%s>", one_barrier ? 's' : 'p', L.coutPad / 32, c3_img ? "c3+" : "", cond ? (sq ? "sft-i8" : "sft") : "plain", i8 ? ",i8" : "");
    if (c3_img && !one_barrier) { rc = fail(c, HDRTV_ESTATE, "conv_first fusion needs the one-barrier schedule"); return; }
    chk(one_barrier ? conv32s_launch(p, c->n_cu, s, c->var.at("conv32_nosplit") != 0) : conv32p_launch(p, c->n_cu, s, c->var.at("conv32_nw")), key.c_str(), tag, macs, bytes);
}


void Seq::resblock(const std::string &base, const f16 *x, const f16 *cond, int H, int W, f16 *tb, f16 *y, const f16 *extra)
{
    // no second residual, enough rows per segment to amortise the 4-row warm-up: ONE row-streaming launch, the intermediate
    // never leaves LDS
    const bool rows = ok() && !extra && rows_on(H, W, false);
    // every layer of the block W8A8 (the full-QAT recipe): the row-streaming kernel on int8 MFMA (le_rows_i8.hip), the rings hold
    // the layers' int8 codes; bit-identical to the two conv32s<sft-i8, i8> launches at the bottom (variant le_rows_i8 = 0: the
    // fake-quant form below, or those launches)
    if (rows && c->var.at("le_rows_i8")) {
        auto q1 = c->q32.find(base + ".conv1"), q2 = c->q32.find(base + ".conv2");
        const SftLayer &S1 = c->sft.at(base + ".sft1"), &S2 = c->sft.at(base + ".sft2");
        if (q1 != c->q32.end() && q2 != c->q32.end() && S1.q && S2.q && q1->second.coutPad == 32 && q2->second.coutPad == 32) {
            RowsRbI8Params p;
            memset(&p, 0, sizeof p);
            p.x = x; p.cond = cond; p.c1 = rows_i8(q1->second); p.c2 = rows_i8(q2->second); p.s1 = rows_i8(S1); p.s2 = rows_i8(S2);
            p.slope1 = act_slope(ACT_RELU);
            p.dst = y; p.trash = const_cast<char *>(wtp<char>(c, c->dump_off)); p.H = H; p.W = W;
            const double npx = (double)H * W;
            chk(le_rb_rows_i8_launch(p, c->n_cu, s), base.c_str(), "le_rb_rows<i8>",
                npx * (2.0 * 32 * 9 * 32 + 4.0 * (16 * 16 + 16 * 32)), npx * (64 + 32 + 64) + 2.0 * 9 * 32 * 32);
            return;
        }
    }
    // fp16 block (le_rows.hip), W8A8 layers as fake-quant (variant le_rows_fq); bit-identical to the two launches below
    if (rows) {
        RowsRbParams p;
        memset(&p, 0, sizeof p);
        bool q1, q2, qs1, qs2;
        const ConvLayer *L1 = rows_conv(base + ".conv1", p.fq_c1, q1), *L2 = rows_conv(base + ".conv2", p.fq_c2, q2);
        const SftLayer &S1 = c->sft.at(base + ".sft1"), &S2 = c->sft.at(base + ".sft2");
        if (L1 && L2 && rows_sft(S1, p.fq_s1, qs1) && rows_sft(S2, p.fq_s2, qs2)) {
            p.fq = (q1 ? 1 : 0) | (q2 ? 2 : 0) | (qs1 ? 4 : 0) | (qs2 ? 8 : 0);
            p.x = x; p.cond = cond; p.H = H; p.W = W; p.dst = y;
            p.w1 = wtp<f16>(c, L1->wpk); p.w2 = wtp<f16>(c, L2->wpk); p.b1 = wtp<float>(c, L1->shift); p.b2 = wtp<float>(c, L2->shift);
            p.sft1_wfrag = wtp<f16>(c, S1.wfrag); p.sft1_bias = wtp<float>(c, S1.bias);
            p.sft2_wfrag = wtp<f16>(c, S2.wfrag); p.sft2_bias = wtp<float>(c, S2.bias);
            p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
            p.dump = stamp_buf();
            const double npx = (double)H * W;
            chk(le_rb_rows_launch(p, c->n_cu, s), base.c_str(), p.fq ? "le_rb_rows<fq>" : "le_rb_rows",
                npx * (2.0 * 32 * 9 * 32 + 4.0 * (16 * 16 + 16 * 32)), npx * (64 + 32 + 64) + 2.0 * 2 * 9 * 32 * 32);
            return;
        }
    }
    conv32(base + ".conv1", x, cond, base + ".sft1", H, W, ACT_RELU, ST_NHWC, tb, 32, H, W);
    conv32(base + ".conv2", tb, cond, base + ".sft2", H, W, ACT_NONE, ST_NHWC, y, 32, H, W, x, extra);
}


int f32_plan(hdrtv_ctx *c, int H, int W)
{
    Seq q{c, nullptr, nullptr};
    return run_f32(c, q, true, H, W, nullptr, nullptr, nullptr, nullptr);
}

int run_agcm(hdrtv_ctx *c, Seq &q, const f16 *rgb, const f16 *cond, f16 *agcm_out)
{
    const Shapes s = shapes_for(c->H, c->W);
    const int cls_ci[5] = {3, 16, 32, 64, 128}, cls_co[5] = {16, 32, 64, 128, 128};
    char a[64], b[64];
    for (int i = 0; i < 5; ++i) {
        snprintf(a, sizeof a, "agcm.u%d", i + 1);
        float *out = q.wsp<float>(a);
        const void *in = cond;
        const float *nm = nullptr, *nr = nullptr, *ng = nullptr, *nb = nullptr;
        if (i > 0) {
            snprintf(b, sizeof b, "agcm.u%d", i);
            in = q.wsp<float>(b);
            snprintf(b, sizeof b, "agcm.mean%d", i); nm = q.wsp<float>(b);
            snprintf(b, sizeof b, "agcm.rstd%d", i); nr = q.wsp<float>(b);
            snprintf(b, sizeof b, "cls%d.g", i - 1); ng = wtp<float>(c, c->f32v.at(b));
            snprintf(b, sizeof b, "cls%d.be", i - 1); nb = wtp<float>(c, c->f32v.at(b));
        }
        snprintf(b, sizeof b, "cls%d.w", i);
        const float *w = wtp<float>(c, c->f32v.at(b));
        snprintf(b, sizeof b, "cls%d.b", i);
        const float *bias = wtp<float>(c, c->f32v.at(b));
        int nblk = 0;
        q.chk(cls_block_launch(in, i == 0, cls_ci[i], s.ch[i], s.cw[i], nm, nr, ng, nb, w, bias, cls_co[i], out, s.ch[i + 1],
                               s.cw[i + 1], q.wsp<float>("agcm.part"), q.s, c->cls_q[i].on ? &c->cls_q[i] : nullptr,
                               (i == 4 && c->cls_q[5].on) ? &c->cls_q[5] : nullptr, &nblk),
              "cls_block", c->cls_q[i].on ? "cls_block<fq>" : "cls_block", (double)s.ch[i] * s.cw[i] * cls_ci[i] * cls_co[i]);
        snprintf(a, sizeof a, "agcm.mean%d", i + 1);
        snprintf(b, sizeof b, "agcm.rstd%d", i + 1);
        q.chk(cls_stats_launch(q.wsp<float>("agcm.part"), cls_co[i], nblk, s.ch[i + 1] * s.cw[i + 1], 1e-5f, q.wsp<float>(a),
                               q.wsp<float>(b), q.s),
              "cls_stats", "cls_stats");
    }
    AgcmFoldArgs fa;
    fa.mean5 = q.wsp<float>("agcm.mean5");
    fa.w20 = wtp<float>(c, c->f32v.at("cls20.w")); fa.b20 = wtp<float>(c, c->f32v.at("cls20.b"));
    for (int st = 0; st < 3; ++st) {
        snprintf(a, sizeof a, "gfm.s%d.w", st); fa.ws[st] = wtp<float>(c, c->f32v.at(a));
        snprintf(a, sizeof a, "gfm.s%d.b", st); fa.bs[st] = wtp<float>(c, c->f32v.at(a));
        snprintf(a, sizeof a, "gfm.t%d.w", st); fa.wt[st] = wtp<float>(c, c->f32v.at(a));
        snprintf(a, sizeof a, "gfm.t%d.b", st); fa.bt[st] = wtp<float>(c, c->f32v.at(a));
    }
    fa.w1 = wtp<float>(c, c->f32v.at("agcm.w1")); fa.b1 = wtp<float>(c, c->f32v.at("agcm.b1"));
    fa.w2 = wtp<float>(c, c->f32v.at("agcm.w2")); fa.b2 = wtp<float>(c, c->f32v.at("agcm.b2"));
    fa.w3 = wtp<float>(c, c->f32v.at("agcm.w3")); fa.b3 = wtp<float>(c, c->f32v.at("agcm.b3"));
    if (c->agcm_q8) {         // W8A8 GFM convs: per-frame dequantisation constants, then the int8 chain
        AgcmFoldQ8Args qa;
        qa.q20 = c->cls_q[5];
        for (int i = 0; i < 6; ++i) qa.qlin[i] = c->lin_q[i];
        qa.P = wtp<float>(c, c->ag_P); qa.Q = wtp<float>(c, c->ag_Q);
        qa.inv2 = c->ag_q[1].inv(); qa.inv3 = c->ag_q[2].inv();
        qa.consts = q.wsp<float>("agcm.qconst");
        q.chk(agcm_fold_q8_launch(fa, qa, q.wsp<float>("agcm.bias"), q.s), "agcm_fold", "agcm_fold<q8>", 128.0 * 6 + 6.0 * (64 + 64 + 3) * 2);
        q.chk(agcm_mlp_q8_launch(rgb, agcm_out, (size_t)c->H * c->W, wtp<int8_t>(c, c->ag_frag), qa.consts, c->ag_q[0].inv(), c->ag_q[0].zoff(),
                                 c->ag_q[1].zoff(), c->ag_q[2].zoff(), q.s),
              "agcm_mlp", "agcm_mlp<q8>", (double)c->H * c->W * (3 * 64 + 64 * 64 + 64 * 3), 12.0 * c->H * c->W);
        return q.rc;
    }
    q.chk(agcm_fold_launch(fa, q.wsp<f16>("agcm.frags"), q.wsp<float>("agcm.bias"), q.s), "agcm_fold", "agcm_fold",
          128.0 * 6 + 6.0 * (64 + 64 + 3) * 2);
    q.chk(agcm_mlp_launch(rgb, agcm_out, (size_t)c->H * c->W, q.wsp<f16>("agcm.frags"), q.wsp<float>("agcm.bias"), q.s),
          "agcm_mlp", "agcm_mlp", (double)c->H * c->W * (3 * 64 + 64 * 64 + 64 * 3), 12.0 * c->H * c->W);
    return q.rc;
}

// HDRUNet3T1._forward_safe_aligned (HDRUNet3T1_arch.py:152-206) with x = [agcm_out, agcm_out]
int run_le(hdrtv_ctx *c, Seq &q, const f16 *img, f16 *out_planar)
{
    const Shapes s = shapes_for(c->H, c->W);
    const int H = s.H, W = s.W;
    f16 *cond = q.wsp<f16>("le.cond");
    f16 *cond1 = q.wsp<f16>("le.cond1"), *cond2 = q.wsp<f16>("le.cond2"), *cond3 = q.wsp<f16>("le.cond3"),
        *cond4 = q.wsp<f16>("le.cond4");
    f16 *h2a = q.wsp<f16>("le.h2a");
    // condition trunk
    // cond_first (3 layers) + CondNet1 (3 layers) in one launch: img -> cond (64 ch) and cond1 (16 ch)
    auto qlast = [&](const QLastLayer &Q, QLastArgs &a) -> const QLastArgs * {
        if (!Q.on) return nullptr;
        a.wq = wtp<int8_t>(c, Q.wq); a.ss = wtp<float>(c, Q.ss); a.q_inv = Q.q.inv(); a.q_zoff = Q.q.zoff();
        return &a;
    };
    QLastArgs qa6, qa2;
    if (q.ok() && c->trunk_q8) {
        TrunkQ8Args ta;
        ta.wfrag = wtp<int8_t>(c, c->tq_frag); ta.consts = wtp<float>(c, c->tq_const);
        ta.q1_inv = c->tq_q[0].inv(); ta.q1_zoff = c->tq_q[0].zoff(); ta.q4_inv = c->tq_q[3].inv();
        for (int i = 0; i < 5; ++i) ta.zoff[i] = c->tq_q[i + 1].zoff();
        q.chk(le_cond_trunk_q8_launch(img, H, W, ta, cond, cond1, c->n_cu, q.s), "LE.cond_trunk", "le_cond_trunk_q8",
              (double)H * W * (27 * 64 + 4 * 64 * 64 + 64 * 16), (double)H * W * (6 + 128 + 32));
    } else if (q.ok())
        q.chk(le_cond_trunk_launch(img, H, W, wtp<f16>(c, c->trunk_wfrag), wtp<float>(c, c->trunk_bias), cond, cond1, c->n_cu, q.s,
                                   qlast(c->q_trunk6, qa6)),
              "LE.cond_trunk", c->q_trunk6.on ? "le_cond_trunk<q6>" : "le_cond_trunk", (double)H * W * (27 * 64 + 4 * 64 * 64 + 64 * 16), (double)H * W * (6 + 128 + 32));
    auto isq8 = [&](const char *L) { return c->q8.find(L) != c->q8.end(); };
    auto qof = [&](const char *L) -> const ActQf * { auto it = c->q8.find(L); return it == c->q8.end() ? nullptr : &it->second.q; };
    f16 *h2b = q.wsp<f16>("le.h2b");
    // CondNet{2,3,4}.0 (3x3 / stride 2 from the 64-channel condition map).  All-fp16 recipes read `cond` once (one launch,
    // 192 channels); a W8A8 layer among them quantises `cond` with its own x_scale / x_zero and runs alone, writing the int8
    // codes of the layer that reads it when that one is W8A8 too.
    const f16 *a2 = nullptr, *a3 = nullptr, *a4 = nullptr;
    const int8_t *a2q = nullptr, *a3q = nullptr, *a4q = nullptr;
    int astride = 64;
    bool cond2_fused = false;
    if (c->conv.find("LE.CondNet234.0") != c->conv.end()) {
        f16 *x192 = q.wsp<f16>("le.x192");
        // CondNet2.2 + .4 ride in that launch's epilogue (variant cond2_fused; a W8A8 CondNet2.4 keeps its own kernel): the first 64 of
        // the 192 channels then never reach HBM
        cond2_fused = c->var.at("cond2_fused") != 0 && !c->tail_q8 && !c->q_tail2.on;
        if (cond2_fused) { q.tail_w = wtp<f16>(c, c->tail_wfrag); q.tail_b = wtp<float>(c, c->tail_bias); q.tail_out = cond2; }
        q.conv("LE.CondNet234.0", cond, 64, nullptr, 0, H, W, ACT_LRELU01, ST_NHWC, x192, 192, s.H1, s.W1);
        a2 = x192; a3 = x192 + 64; a4 = x192 + 128; astride = 192;
    } else {
        f16 *ca[3] = {q.wsp<f16>("le.c2a"), q.wsp<f16>("le.c3a"), q.wsp<f16>("le.c4a")};
        int8_t *ca8[3] = {q.wsp<int8_t>("le8.c2a"), q.wsp<int8_t>("le8.c3a"), q.wsp<int8_t>("le8.c4a")};
        const char *l0[3] = {"LE.CondNet2.0", "LE.CondNet3.0", "LE.CondNet4.0"}, *l2[3] = {nullptr, "LE.CondNet3.2", "LE.CondNet4.2"};
        const f16 **af[3] = {&a2, &a3, &a4};
        const int8_t **aq[3] = {&a2q, &a3q, &a4q};
        // the W8A8 ones together: `cond` is read once and quantised per layer in registers (conv_q8_multi)
        ConvQ8MultiParams mp;
        memset(&mp, 0, sizeof mp);
        mp.src = cond; mp.src_stride = 64; mp.Hi = H; mp.Wi = W; mp.Ho = s.H1; mp.Wo = s.W1;
        double m_macs = 0.0, m_bytes = 2.0 * 64 * H * W;
        for (int i = 0; i < 3; ++i) {
            if (!isq8(l0[i])) continue;
            const QLayer &L = c->q8.at(l0[i]);
            const ActQf *oq = l2[i] ? qof(l2[i]) : (c->tail_q8 ? &c->tl_q[0] : nullptr);    // CondNet2.0 feeds the fused tail
            ConvQ8Group &G = mp.g[mp.ngroups++];
            G.wpk8 = wtp<int8_t>(c, L.wpk8); G.scale = wtp<float>(c, L.scale); G.shift = wtp<float>(c, L.shift);
            G.q_inv = L.q.inv(); G.q_zoff = L.q.zoff(); G.act = ACT_LRELU01;
            G.dst = oq ? (void *)ca8[i] : (void *)ca[i]; G.dst_i8 = oq ? 1 : 0;
            if (oq) { G.oq_inv = oq->inv(); G.oq_zoff = oq->zoff(); *aq[i] = ca8[i]; } else { *af[i] = ca[i]; }
            m_macs += (double)s.H1 * s.W1 * 64 * 9 * 64;
            m_bytes += (double)s.H1 * s.W1 * 64 * (oq ? 1.0 : 2.0) + 9.0 * 64 * 64;
        }
        if (mp.ngroups && q.ok()) {
            char tag[48];
            snprintf(tag, sizeof tag, "conv_q8_multi<%d>", mp.ngroups);
            q.chk(conv_q8_multi_launch(mp, c->n_cu, q.s), "LE.CondNet234.0", tag, m_macs, m_bytes);
        }
        for (int i = 0; i < 3; ++i) {
            if (isq8(l0[i])) {
                continue;
            } else {
                q.conv(l0[i], cond, 64, nullptr, 0, H, W, ACT_LRELU01, ST_NHWC, ca[i], 64, s.H1, s.W1);
                *af[i] = ca[i];
            }
        }
    }
    // CondNet2.2 + .4 (1x1 64->64, LeakyReLU, 1x1 64->16) in one pass over CondNet2.0's 64 channels
    if (q.ok() && c->tail_q8) {
        if (!a2q) return q.rc = fail(c, HDRTV_ESTATE, "internal: W8A8 CondNet2 tail without int8 input");
        q.chk(cond_tail_q8_launch(a2q, (size_t)s.H1 * s.W1, wtp<int8_t>(c, c->tl_frag), wtp<float>(c, c->tl_const), c->tl_q[1].zoff(), cond2,
                                  c->n_cu, q.s),
              "LE.CondNet2.2+4", "cond_tail_q8", (double)s.H1 * s.W1 * (64 * 64 + 64 * 16), (double)s.H1 * s.W1 * (64 + 32));
    } else if (q.ok() && !cond2_fused)
        q.chk(cond_tail_launch(a2, astride, (size_t)s.H1 * s.W1, wtp<f16>(c, c->tail_wfrag), wtp<float>(c, c->tail_bias), cond2, c->n_cu, q.s,
                               qlast(c->q_tail2, qa2)),
              "LE.CondNet2.2+4", c->q_tail2.on ? "cond_tail<q2>" : "cond_tail", (double)s.H1 * s.W1 * (64 * 64 + 64 * 16), (double)s.H1 * s.W1 * (128 + 32));
    // CondNet3 / CondNet4: .2 (3x3 / stride 2, 64 -> 64, LeakyReLU) then .4 (1x1 resp. 3x3 / stride 2, 64 -> 16)
    {
        const f16 *af[2] = {a3, a4};
        const int8_t *aq[2] = {a3q, a4q};
        f16 *h2[2] = {h2a, h2b}, *cout[2] = {cond3, cond4};
        const char *l2[2] = {"LE.CondNet3.2", "LE.CondNet4.2"}, *l4[2] = {"LE.CondNet3.4", "LE.CondNet4.4"};
        bool tail4 = false;
        for (int i = 0; i < 2; ++i) {
            const void *h = h2[i];
            bool h_i8 = false;
            if (isq8(l2[i])) {
                const ActQf *oq = qof(l4[i]);
                int8_t *h8 = oq ? q.wsp<int8_t>(i ? "le8.h2b" : "le8.h2a") : nullptr;
                q.convq8(l2[i], aq[i] ? (const void *)aq[i] : (const void *)af[i], aq[i] != nullptr, aq[i] ? 64 : astride, s.H1, s.W1,
                         ACT_LRELU01, oq ? (void *)h8 : (void *)h2[i], 64, oq);
                if (oq) { h = h8; h_i8 = true; }
            } else {
                // CondNet3.4 (1x1, no activation) rides in CondNet3.2's epilogue (variant cond3_fused): its 64-channel input never reaches HBM
                auto t4 = c->conv.find(l4[i]);
                if (i == 0 && c->var.at("cond3_fused") && !isq8(l4[i]) && t4 != c->conv.end() && t4->second.ks == 1 && t4->second.cin == 64 &&
                    t4->second.cout == 16 && t4->second.coutPad == 32 && t4->second.cin_t == 64) {
                    q.tail_w = wtp<f16>(c, t4->second.wpk); q.tail_s = wtp<float>(c, t4->second.scale); q.tail_b = wtp<float>(c, t4->second.shift);
                    q.tail_out = cout[i];
                    tail4 = true;
                }
                q.conv(l2[i], af[i], 64, nullptr, 0, s.H1, s.W1, ACT_LRELU01, ST_NHWC, h2[i], 64, s.H2, s.W2, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, astride);
            }
            if (tail4) { tail4 = false; continue; }
            if (isq8(l4[i])) q.convq8(l4[i], h, h_i8, 64, s.H2, s.W2, ACT_NONE, cout[i], 16, nullptr);
            else q.conv(l4[i], h2[i], 64, nullptr, 0, s.H2, s.W2, ACT_NONE, ST_NHWC, cout[i], 16, i ? s.H3 : s.H2, i ? s.W3 : s.W2);
        }
    }
    // main branch: every SFT is fused into the 3x3 conv that follows it
    f16 *f0a = q.wsp<f16>("le.f0a"), *f0b = q.wsp<f16>("le.f0b"), *fea0 = q.wsp<f16>("le.fea0"), *up3 = q.wsp<f16>("le.up3");
    bool head_fused = false;
    // the full-resolution head and tail each as one row-streaming launch: even shapes, enough rows per segment
    const bool rows = q.rows_on(H, W, true);
    // conv_first .. down_conv1 in one row-streaming launch (le_rows.hip) when every layer is fp16 or a W8A8 layer the kernel runs
    // as fake-quant (variant le_rows_fq)
    // every layer of the head W8A8 (the full-QAT recipe): the row kernel on int8 MFMA (le_rows_i8.hip), bit-identical to conv_c3_q8 +
    // conv32s<sft-i8, i8> + conv_q8<32,3,2>
    if (q.ok() && rows && c->var.at("le_rows_i8") && !c->var.at("no_c3q8")) {
        auto qc = c->q8.find("LE.conv_first#c3");
        auto qh = c->q32.find("LE.HR_conv1"), qd = c->q32.find("LE.down_conv1#rows8");
        const SftLayer &S1 = c->sft.at("LE.SFT_layer1");
        if (qc != c->q8.end() && qh != c->q32.end() && qd != c->q32.end() && S1.q && qh->second.coutPad == 32 && qd->second.coutPad == 32) {
            RowsHeadI8Params p;
            memset(&p, 0, sizeof p);
            p.img = img; p.cond = cond1; p.fea0 = fea0; p.fea1 = q.wsp<f16>("le.fea1a"); p.H = H; p.W = W;
            p.cf = q.rows_i8(qc->second); p.hr = q.rows_i8(qh->second); p.dn = q.rows_i8(qd->second); p.s = q.rows_i8(S1);
            p.slope_relu = act_slope(ACT_RELU);
            p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
            const double npx = (double)H * W;
            q.chk(le_head_rows_i8_launch(p, c->n_cu, q.s), "LE.head", "le_head_rows<i8>",
                  npx * (27.0 * 32 + 2.0 * (16 * 16 + 16 * 32) + 32.0 * 9 * 32 + 32.0 * 9 * 32 / 4), npx * (6 + 32 + 64 + 16) + 2.0 * 9 * 32 * 32);
            head_fused = true;
        }
    }
    if (!head_fused && q.ok() && rows && !c->var.at("no_c3fuse") && !c->var.at("conv32_old")) {
        RowsHeadParams p;
        memset(&p, 0, sizeof p);
        bool qh, qd, qs, qi = isq8("LE.conv_first");
        const ConvLayer *Lh = q.rows_conv("LE.HR_conv1", p.fq_y, qh), *Ld = q.rows_conv("LE.down_conv1", p.fq_f, qd);
        const SftLayer &S1 = c->sft.at("LE.SFT_layer1");
        auto i3 = c->c3.find(qi ? "le.conv_first#fq" : "le.conv_first");
        if (Lh && Ld && q.rows_sft(S1, p.fq_s, qs) && i3 != c->c3.end() && (!qi || c->var.at("le_rows_fq"))) {
            if (qi) p.fq_img = Seq::fqp(c->q8.at("LE.conv_first").q);
            p.fq = (qi ? 1 : 0) | (qh ? 2 : 0) | (qd ? 4 : 0) | (qs ? 8 : 0);
            p.img = img; p.cond = cond1; p.H = H; p.W = W; p.fea0 = fea0; p.fea1 = q.wsp<f16>("le.fea1a");
            p.c3_wfrag = wtp<f16>(c, i3->second.wfrag);
            p.sft_wfrag = wtp<f16>(c, S1.wfrag); p.sft_bias = wtp<float>(c, S1.bias);
            p.w_hr = wtp<f16>(c, Lh->wpk); p.b_hr = wtp<float>(c, Lh->shift); p.w_down = wtp<f16>(c, Ld->wpk); p.b_down = wtp<float>(c, Ld->shift);
            p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
            p.dump = q.stamp_buf();
            const double npx = (double)H * W;
            q.chk(le_head_rows_launch(p, c->n_cu, q.s), "LE.head", p.fq ? "le_head_rows<fq>" : "le_head_rows",
                  npx * (27.0 * 32 + 2.0 * (16 * 16 + 16 * 32) + 32.0 * 9 * 32 + 32.0 * 9 * 32 / 4), npx * (6 + 32 + 64 + 16) + 2.0 * 2 * 9 * 32 * 32);
            head_fused = true;
        }
    }
    if (!head_fused) {
        if (isq8("LE.conv_first")) {
            if (c->var.at("no_c3q8")) {                  // developer A/B switch: the generic two-launch form     // the 3 planes as NHWC int8 codes (3 of 32 bytes real), then the generic int8 conv
                int8_t *img32 = q.wsp<int8_t>("le8.img32");
                const QLayer &Lq = c->q8.at("LE.conv_first");
                if (q.ok()) q.chk(planar3_to_q8_launch(img, (size_t)H * W, Lq.q.inv(), Lq.q.zoff(), img32, q.s), "le.conv_first.pack", "planar3_to_q8", 0.0, 38.0 * H * W);
                q.convq8("LE.conv_first", img32, true, 32, H, W, ACT_RELU, f0a, 32, nullptr);
            } else if (q.ok()) {      // quantised while the patch is staged, K = (ky | kx4, c4): two int8 MFMAs per 32 pixels (conv_c3_q8)
                const QLayer &Lq = c->q8.at("LE.conv_first#c3");
                q.chk(conv_c3_q8_launch(img, H, W, wtp<int8_t>(c, Lq.wpk8), wtp<float>(c, Lq.scale), wtp<float>(c, Lq.shift), Lq.q.inv(),
                                        Lq.q.zoff(), ACT_RELU, f0a, c->n_cu, q.s),
                      "LE.conv_first", "conv_c3_q8", (double)H * W * 27 * 32, (double)H * W * (6.0 + 64.0));
            }
            q.conv32("LE.HR_conv1", f0a, cond1, "LE.SFT_layer1", H, W, ACT_RELU, ST_NHWC, fea0, 32, H, W);
        } else {
            // fp16 conv_first is computed inside HR_conv1's kernel from the three planes (conv32s.hip, C3): its 32-channel output
            // (0.53 GB at 4K, written and read back) never exists.  Variants no_c3fuse / conv32_old: the two-launch form
            // (developer A/B switches); a W8A8 HR_conv1 behind an fp16 conv_first has no fused kernel.
            const bool fuse = !c->var.at("no_c3fuse") && !c->var.at("conv32_old") && c->q32.find("LE.HR_conv1") == c->q32.end();
            if (fuse) {
                q.conv32("LE.HR_conv1", f0a, cond1, "LE.SFT_layer1", H, W, ACT_RELU, ST_NHWC, fea0, 32, H, W, nullptr, nullptr, nullptr, nullptr,
                         img, "le.conv_first");
            } else {
                q.c3("le.conv_first", img, H, W, ACT_RELU, f0a, nullptr);
                q.conv32("LE.HR_conv1", f0a, cond1, "LE.SFT_layer1", H, W, ACT_RELU, ST_NHWC, fea0, 32, H, W);
            }
        }
    }
    f16 *fea1a = q.wsp<f16>("le.fea1a"), *fea1 = q.wsp<f16>("le.fea1"), *l1b = q.wsp<f16>("le.l1b");
    auto down = [&](const char *key, const f16 *src, int Hi, int Wi, f16 *dst, int Ho, int Wo) {
        if (isq8(key)) q.convq8(key, src, false, 32, Hi, Wi, ACT_RELU, dst, 32, nullptr);
        else q.conv(key, src, 32, nullptr, 0, Hi, Wi, ACT_RELU, ST_NHWC, dst, 32, Ho, Wo);
    };
    if (!head_fused) down("LE.down_conv1", fea0, H, W, fea1a, s.H1, s.W1);
    q.resblock("LE.recon_trunk1.0", fea1a, cond2, s.H1, s.W1, l1b, fea1);
    f16 *fea2a = q.wsp<f16>("le.fea2a"), *fea2 = q.wsp<f16>("le.fea2"), *l2b = q.wsp<f16>("le.l2b");
    down("LE.down_conv2", fea1, s.H1, s.W1, fea2a, s.H2, s.W2);
    q.resblock("LE.recon_trunk2.0", fea2a, cond3, s.H2, s.W2, l2b, fea2);
    f16 *fea3 = q.wsp<f16>("le.fea3"), *l3b = q.wsp<f16>("le.l3b"), *t3x = q.wsp<f16>("le.t3x"), *t3y = q.wsp<f16>("le.t3y");
    down("LE.down_conv3", fea2, s.H2, s.W2, fea3, s.H3, s.W3);
    q.resblock("LE.recon_trunk3.0", fea3, cond4, s.H3, s.W3, l3b, t3x);
    q.resblock("LE.recon_trunk3.1", t3x, cond4, s.H3, s.W3, l3b, t3y);
    q.resblock("LE.recon_trunk3.2", t3y, cond4, s.H3, s.W3, l3b, t3x);
    q.resblock("LE.recon_trunk3.3", t3x, cond4, s.H3, s.W3, l3b, t3y, fea3);   // "+ fea3" (line 180) fused as 2nd residual
    // up path: relu(shuffle(conv)) + skip, cropped to the skip's size (_align_to)
    f16 *up1 = q.wsp<f16>("le.up1"), *t4 = q.wsp<f16>("le.t4");
    q.conv32("LE.up_conv1.0", t3y, nullptr, "", s.H3, s.W3, ACT_RELU, ST_PS, up1, 32, s.H2, s.W2, fea2);
    q.resblock("LE.recon_trunk4.0", up1, cond3, s.H2, s.W2, l2b, t4);
    f16 *up2 = q.wsp<f16>("le.up2"), *t5 = q.wsp<f16>("le.t5");
    q.conv32("LE.up_conv2.0", t4, nullptr, "", s.H2, s.W2, ACT_RELU, ST_PS, up2, 32, s.H1, s.W1, fea1);
    q.resblock("LE.recon_trunk5.0", up2, cond2, s.H1, s.W1, l1b, t5);
    // the full-resolution tail: one row-streaming launch (le_rows.hip) when every layer is fp16 or a W8A8 layer the kernel runs as
    // fake-quant, else per layer
    if (q.ok() && rows && c->var.at("le_rows_i8")) {
        // every layer of the tail W8A8 (the full-QAT recipe): the row kernel on int8 MFMA (le_rows_i8.hip), bit-identical to the three
        // per-layer int8 launches at the bottom
        auto qu = c->q32.find("LE.up_conv3.0"), qh = c->q32.find("LE.HR_conv2"), ql = c->q32.find("LE.conv_last");
        const SftLayer &S2 = c->sft.at("LE.SFT_layer2");
        if (qu != c->q32.end() && qh != c->q32.end() && ql != c->q32.end() && S2.q && qu->second.coutPad == 128 &&
            qh->second.coutPad == 32 && ql->second.coutPad == 32) {
            RowsTailI8Params p;
            memset(&p, 0, sizeof p);
            p.u = t5; p.fea0 = fea0; p.cond = cond1; p.res_planar = img; p.dst_planar = out_planar; p.H = H; p.W = W;
            p.up = q.rows_i8(qu->second); p.hr = q.rows_i8(qh->second); p.last = q.rows_i8(ql->second); p.s = q.rows_i8(S2);
            p.slope_relu = act_slope(ACT_RELU);
            p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
            const double npx = (double)H * W;
            q.chk(le_tail_rows_i8_launch(p, c->n_cu, q.s), "LE.tail", "le_tail_rows<i8>",
                  npx * (32.0 * 9 * 128 / 4 + 2.0 * (16 * 16 + 16 * 32) + 32.0 * 9 * 32 + 32.0 * 9 * 3), npx * (16 + 64 + 32 + 6 + 6) + 9.0 * 32 * (128 + 32 + 32));
            return q.rc;
        }
    }
    if (q.ok() && rows) {
        RowsTailParams p;
        memset(&p, 0, sizeof p);
        bool qu, qh, ql, qs;
        const ConvLayer *Lu = q.rows_conv("LE.up_conv3.0", p.fq_u, qu), *Lh = q.rows_conv("LE.HR_conv2", p.fq_y, qh),
                        *Ll = q.rows_conv("LE.conv_last", p.fq_z, ql);
        const SftLayer &S2 = c->sft.at("LE.SFT_layer2");
        if (Lu && Lh && Ll && q.rows_sft(S2, p.fq_s, qs)) {
            p.fq = (qu ? 1 : 0) | (qh ? 2 : 0) | (ql ? 4 : 0) | (qs ? 8 : 0);
            p.u = t5; p.fea0 = fea0; p.cond = cond1; p.res_planar = img; p.dst_planar = out_planar; p.H = H; p.W = W;
            p.w_up = wtp<f16>(c, Lu->wpk); p.b_up = wtp<float>(c, Lu->shift);
            p.sft_wfrag = wtp<f16>(c, S2.wfrag); p.sft_bias = wtp<float>(c, S2.bias);
            p.w_hr = wtp<f16>(c, Lh->wpk); p.b_hr = wtp<float>(c, Lh->shift); p.w_last = wtp<f16>(c, Ll->wpk); p.b_last = wtp<float>(c, Ll->shift);
            p.trash = const_cast<char *>(wtp<char>(c, c->dump_off));
            p.dump = q.stamp_buf();
            const double npx = (double)H * W;
            q.chk(le_tail_rows_launch(p, c->n_cu, q.s), "LE.tail", p.fq ? "le_tail_rows<fq>" : "le_tail_rows",
                  npx * (32.0 * 9 * 128 / 4 + 2.0 * (16 * 16 + 16 * 32) + 32.0 * 9 * 32 + 32.0 * 9 * 3), npx * (16 + 64 + 32 + 6 + 6) + 2.0 * 9 * 32 * (128 + 32 + 32));
            return q.rc;
        }
    }
    q.conv32("LE.up_conv3.0", t5, nullptr, "", s.H1, s.W1, ACT_RELU, ST_PS, up3, 32, H, W, fea0);
    q.conv32("LE.HR_conv2", up3, cond1, "LE.SFT_layer2", H, W, ACT_RELU, ST_NHWC, f0b, 32, H, W);
    q.conv32("LE.conv_last", f0b, nullptr, "", H, W, ACT_NONE, ST_PLANAR3, nullptr, 0, H, W, nullptr, nullptr, out_planar, img);
    return q.rc;
}

// hg_need's program for a padded frame, from the layer table: the tensors' need maps, one list per layer.  Returns the bytes of
// the buffer ("hg.need") all of it lies in; the layout does not depend on the variants (every map is sized for the finest unit
// table), only HgNeedLayer::th and the unit table (hg_sparse = 1: 16x16 cells, else the sub-tile units) do.
// Layout: flags | two blocks no longer used (the byte-per-cell maps of the first form; they keep the lists where they were) |
// the layers' lists | the tensors' bit-row maps | two scratch maps | conv1's list | the map of conv1's input.
// conv1 (conv_c3: pool-fused 3x3 at level 0, 8 x 32 tiles, img -> hg_layers[0].in) is not a row of the table; it is p.L[0], in front
// of the table's rows, and what it adds to the buffer lies behind everything else.
size_t hg_need_plan(hdrtv_ctx *c, int Hp, int Wp, HgNeedParams &p)
{
    memset(&p, 0, sizeof p);
    p.Hp = Hp; p.Wp = Wp;
    constexpr int n_layers = (int)(sizeof hg_layers / sizeof hg_layers[0]);
    static_assert(n_layers + 1 <= HG_NEED_MAX_LAYERS && n_layers + 3 <= HG_NEED_MAX_TENSORS, "hg_need's tables are too small");
    constexpr int max_level = [] { int m = 0; for (const HgLayer &L : hg_layers) m = L.level > m ? L.level : m; return m; }();
    static_assert(max_level < HG_NEED_LEVELS, "hg_need's unit tables have too few levels");
    memcpy(p.lu, hg_need_unit_log2[c->var.at("hg_sparse") == 1 ? 1 : 2], sizeof p.lu);
    auto ncell = [&](int level) { return (((Hp >> level) + 15) / 16) * (((Wp >> level) + 15) / 16); };
    // 64-bit words of a level's bit-row map, and of a map with one row per 8-row tile (the list pass), under any unit table
    auto nwords = [&](int level) {
        size_t m = 0;
        for (const auto &tab : hg_need_unit_log2) {
            const int u = 1 << tab[level], rows = std::max(((Hp >> level) + u - 1) / u, ((Hp >> level) + 7) / 8);
            m = std::max(m, (size_t)rows * ((((Wp >> level) + u - 1) / u + 63) / 64));
        }
        return m;
    };
    const char *names[HG_NEED_MAX_TENSORS];
    int level[HG_NEED_MAX_TENSORS], nt = 0;
    auto tensor = [&](const char *name, int lev) {
        if (!name) name = "part";                    // Up_conv5's sums: their need map is hg_prep's flags
        for (int i = 0; i < nt; ++i)
            if (!strcmp(names[i], name)) return i;
        names[nt] = name; level[nt] = lev;
        return nt++;
    };
    for (int i = 0; i < n_layers; ++i) {
        const HgLayer &L = hg_layers[i];
        HgNeedLayer &N = p.L[i + 1];
        N.level = L.level; N.ks = L.ks; N.tw = 16;
        N.mode = L.mode == ST_POOL ? 1 : (L.ps ? 2 : 0);
        N.in = tensor(L.in, L.level);
        N.skip = L.skip ? tensor(L.skip, L.level) : -1;
        N.out = tensor(L.out, L.out_level());
        N.th = L.ks == 3 && Seq::prw_tile_rows(c, L.mode, L.cout, Hp >> L.level, Wp >> L.level) == 8 ? 8 : 16;    // conv()'s own choice
    }
    const int nt_table = nt;                         // conv1's input comes last: its map lies behind the table's
    {
        HgNeedLayer &N = p.L[0];
        N.level = 0; N.ks = 3; N.mode = 1;
        N.out = tensor(hg_layers[0].in, 1);
        N.in = tensor("img", 0);
        N.skip = -1;
        N.th = 8; N.tw = 32;                         // conv_c3's tiles (le_hg_misc.hip)
    }
    p.n_layers = n_layers + 1;
    // hg_need walks the table backwards: the first reader it meets stores a tensor's map, so no map needs clearing
    bool seen[HG_NEED_MAX_TENSORS] = {};
    for (int i = p.n_layers - 1; i >= 0; --i) {
        HgNeedLayer &N = p.L[i];
        N.in_first = !seen[N.in];
        seen[N.in] = true;
        if (N.skip >= 0) { N.skip_first = !seen[N.skip]; seen[N.skip] = true; }
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return (int)o; };
    p.flags_off = take((size_t)ncell(0));
    take((size_t)ncell(0));
    for (int t = 0; t < nt_table; ++t)
        if (strcmp(names[t], "part")) take((size_t)ncell(level[t]));
    for (int i = 1; i <= n_layers; ++i) p.L[i].list_off = take(4 * (2 * (size_t)ncell(p.L[i].level) + 4));
    size_t scratch = 0;
    for (int t = 0; t < nt; ++t) scratch = std::max(scratch, nwords(level[t]));
    for (int t = 0; t < nt_table; ++t) {
        p.map_off[t] = take(8 * nwords(level[t]));
        if (!strcmp(names[t], "part")) p.flags_map = t;
    }
    for (int i = 0; i < p.n_layers; ++i) {
        p.L[i].out_chained = i + 1 < p.n_layers ? p.L[i + 1].in == p.L[i].out : p.L[i].out == p.flags_map;
        p.L[i].in_chained = i > 0 && p.L[i - 1].out == p.L[i].in;
    }
    p.scratch_words = (int)scratch;
    p.kbits_off = take(8 * scratch);
    p.tbits_off = take(8 * scratch);
    // conv1: 8 x 32 tiles, two per 16x16 cell
    p.L[0].list_off = take(4 * (2 * (size_t)ncell(0) + 4));
    p.map_off[nt_table] = take(8 * nwords(0));
    return off;
}

// HG_Composite.forward tail + Hallucination_Generator.forward.  complete_taps: hdrtv_get_tap's on-demand completion -- conv1 ..
// Up_conv5 over every tile from the hg.img of the lane's last frame, no hg_prep, no blend.
int run_hg(hdrtv_ctx *c, Seq &q, const f16 *base, void *out, int out_f32, bool complete_taps)
{
    const Shapes s = shapes_for(c->H, c->W);
    const int Hp = s.Hp, Wp = s.Wp;
    f16 *img = q.wsp<f16>("hg.img");
    uint8_t *mask = q.wsp<uint8_t>("hg.mask");
    // Need lists (variant hg_sparse; fp16 HG with the per-pixel tail): every layer of the head, conv1 included, computes only the
    // tiles a masked output pixel depends on (conv_c3<64,dot3>, conv_pglds, conv_prw, conv_glds1 each walk their list),
    // the blend takes img everywhere else.  Built on the device behind hg_prep (hg_need.hip).
    const bool sparse = !complete_taps && c->var.at("hg_sparse") != 0 && !c->hg_i8 && !c->var.at("final_recompute");
    HgNeedParams np;
    if (sparse) {
        hg_need_plan(c, Hp, Wp, np);
        np.base = q.wsp<unsigned char>("hg.need");
    }
    if (q.ws == c->lane_ws[0] && !complete_taps) {
        // lane 0's hg.* tensors are partial from here on; a frame captured into a graph may be replayed any number of times later
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        c->taps_partial = sparse;
        c->taps_replayable = sparse && hipStreamIsCapturing(q.s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
        c->taps_stream = q.s;
    }
    if (!complete_taps)
        q.chk(hg_prep_launch(base, s.H, s.W, Hp, Wp, img, mask, c->mask_r, 0.1f, q.s, sparse ? np.base + np.flags_off : nullptr), "hg_prep",
              "hg_prep", 0.0, 13.0 * Hp * Wp);
    if (sparse) q.chk(hg_need_launch(np, q.s), "hg_need", "hg_need", 0.0, 0.0);
    float *part = q.wsp<float>("hg.part");
    // conv1: only the pooled map is kept; its kernel also leaves conv10's second half (the 64 -> 3 sums over conv1's channels) per
    // pixel, so the tail is a per-pixel kernel.  Variant final_recompute (developer A/B switch): the tail recomputes conv1
    // instead (hg_final_fused) -- same arithmetic, same results.
    const bool light = !c->var.at("final_recompute");
    float *part2 = light ? q.wsp<float>("hg.part2") : nullptr;
    const f16 *w2frag = light ? wtp<f16>(c, c->hgf_wfrag) + 6 * 64 * 8 : nullptr;      // fragments 6..9 of the tail's set
    // the table's tensors, each looked up once: hg.<t>, or (W8A8 checkpoint: conv2 .. conv9 on int8 MFMA) the int8 codes hg8.<t>
    constexpr int n_layers = (int)(sizeof hg_layers / sizeof hg_layers[0]);
    const char *tn[3 * n_layers];
    void *tp[3 * n_layers];
    int nt = 0;
    auto tensor = [&](const char *name) -> void * {
        if (!name) return nullptr;
        for (int i = 0; i < nt; ++i)
            if (!strcmp(tn[i], name)) return tp[i];
        char key[32];
        snprintf(key, sizeof key, "%s%s", c->hg_i8 ? "hg8." : "hg.", name);
        tn[nt] = name;
        tp[nt] = q.wsp<void>(key);
        return tp[nt++];
    };
    // conv1 keeps only its pooled map, conv2's input.  W8A8: the fp16 -> int8 boundary costs no pass of its own, conv1 stores the
    // codes conv2 wants (hg_q0_inv = 0 for an fp16 HG: no quantiser)
    // (its need list: the per-pixel tail reads part2 at masked pixels only, conv2 reads the pooled map where its own list says)
    const bool c1_list = sparse && light;
    q.c3("hg.conv1", img, Hp, Wp, ACT_RELU, nullptr, (f16 *)tensor(hg_layers[0].in), c->hg_q0_inv, c->hg_q0_zero, w2frag, part2,
         c1_list ? reinterpret_cast<const int *>(np.base + np.L[0].list_off) : nullptr, c1_list ? ((Hp + 7) / 8) * ((Wp + 31) / 32) : 0);
    char key[32];
    for (const HgLayer &L : hg_layers) {
        snprintf(key, sizeof key, "hg.%s", L.name);
        if (sparse) {
            const HgNeedLayer &N = np.L[&L - hg_layers + 1];
            q.need_list = reinterpret_cast<const int *>(np.base + N.list_off);
            q.need_th = N.th;
            q.need_total = (((Hp >> L.level) + N.th - 1) / N.th) * (((Wp >> L.level) + 15) / 16);
        }
        const int c1 = L.skip_cin, c0 = L.cin - c1, Hi = Hp >> L.level, Wi = Wp >> L.level;
        const int Ho = Hp >> L.out_level(), Wo = Wp >> L.out_level();
        const bool dot3 = L.mode == ST_PS_DOT3;
        const float *dotw = dot3 ? wtp<float>(c, c->hg_w10a) : nullptr;
        float *dst_dot = dot3 ? part : nullptr;
        if (c->hg_i8)
            q.conv8(key, (const int8_t *)tensor(L.in), c0, (const int8_t *)tensor(L.skip), c1, Hi, Wi, L.mode, tensor(L.out), L.out_c(), Ho, Wo, dotw, dst_dot);
        else
            q.conv(key, (const f16 *)tensor(L.in), c0, (const f16 *)tensor(L.skip), c1, Hi, Wi, L.act, L.mode, (f16 *)tensor(L.out), L.out_c(), Ho, Wo,
                   nullptr, nullptr, nullptr, nullptr, nullptr, dotw, dst_dot);
    }
    if (!q.ok() || complete_taps) return q.rc;
    const C3Layer &L1 = c->c3.at("hg.conv1");
    HgFinalFusedArgs fa;
    fa.img = img; fa.mask = mask; fa.part = part; fa.wfrag = wtp<f16>(c, c->hgf_wfrag);
    fa.scale = wtp<float>(c, L1.scale); fa.shift = wtp<float>(c, L1.shift);
    fa.b10 = wtp<float>(c, c->f32v.at("hg.b10"));
    fa.wl = wtp<float>(c, c->f32v.at("hg.wl")); fa.bl = wtp<float>(c, c->f32v.at("hg.bl"));
    fa.out = out; fa.out_f32 = out_f32; fa.H = s.H; fa.W = s.W; fa.Hp = Hp; fa.Wp = Wp;
    if (light)
        q.chk(hg_final_light_launch(fa, part2, q.s), "hg_final", "hg_final_light", (double)s.H * s.W * 6 * 3,
              (double)s.H * s.W * (6 + 1 + 32 + 3 * (out_f32 ? 4 : 2)));
#ifdef HDRTV_AB
    else
        q.chk(hg_final_fused_launch(fa, c->n_cu, q.s), "hg_final", "hg_final_fused", (double)Hp * Wp * (128 * 3 + 6 * 3),
              (double)s.H * s.W * (6 + 1 + 16 + 3 * (out_f32 ? 4 : 2)));
#endif
    return q.rc;
}

}  // namespace hdrtv_host
