"""Float64 reference of ONE launch of the HG head's W8A8 path, with an a-priori bound and a model.  TEST INFRASTRUCTURE ONLY.

CPU only.  Built on tests/hg_layer_ref.py (H: the stage table, its fp16 launches hg_prep, conv1 and hg_final, `split_pair`, HBounded /
HRounded) and tests/le_i8_layer_ref.py (Q: `Codes`, `_epilogue_span`, `border_classes`, `class_sums`, the marked-element
bookkeeping, `cap_ok`, CAP_SHARE / CAP_MIN); both are imported, not copied.  The head is BASELINE.json configs[4].

STAGES: one per launch `run_hg` (csrc/api_graph.hip) issues for a W8A8 checkpoint with hg_sparse = 0, 21 in all, H's names and profile keys:
  prep      [hg_prep | hg_prep]                        le.out -> img, mask           H's stage, exact
  conv1     [hg.conv1 | conv_c3<64,dot3>]              img -> p1 (codes), part2      H's conv1 + the quantising store (le_hg_misc.hip:235-247)
  conv2     [conv_pglds_i8<nhwc,c64>]                  p1 -> conv2
  conv3_1 .. conv_code2   [conv_pglds_i8 / conv_prw_i8 / conv_prw8_i8 <pool | nhwc>]
  Up_conv1 .. Up_conv4    [.. <ps>]
  conv6 .. conv9          [conv1x1_i8]                 cat(up, encoder skip) -> codes; conv9: 64 real output channels of a 128-wide tile
  Up_conv5  [conv_pglds_i8<ps_dot3,c64>]               conv9 -> part (fp32)
  final     [hg_final | hg_final_light]                (img, mask, part, part2) -> out   H's stage
Every hg8.* tensor and hg.part has its own workspace slot, so every launch is held alone on the device's own input codes: the input of
an int8 layer is EXACT, and with it the integer sum.  conv1x1_i8<f16> cannot be reached: every 1x1 layer of the table (conv6 .. conv9)
has an int8 reader (Up_conv2.0 .. Up_conv5.0), so Seq::conv8 never packs a 1x1 layer with out_f16.

A W8A8 layer is evaluated three ways.
  v      the network as it is written (W8A8Conv2d.forward, Hallucination_arch.py), float64: dequantise the input codes (q + 128) x_scale
         + x_zero, zero-pad AFTER dequantisation, convolve with weight_int8 * w_scale, add the bias, BatchNorm with running statistics,
         ReLU where the layer has one, maxpool2 / PixelShuffle, and for a code output the reader's quantiser clip(rint((y - x_zero') /
         x_scale'), 0, 255).  None of the kernel's fold: no code-0 halo, no delta, no pool before the quantiser, no lo_clamp.
  model  the kernel's arithmetic at its rounding points: the exact integer sum with out-of-image taps as int8 code 0; scale[n],
         shift[n], delta[cls][n], delta_acc[cls][n] = nearbyint(..), lo_clamp and read_actq's "integer within 1e-3" rule restated from
         api_pack.hip pack_conv_i8 (:94-180, :82-93) in float64 and rounded to fp32 where it rounds; cls = (row bits << 2) | column
         bits, bit 0 = first tap outside, bit 1 = last tap outside (conv3x3_pglds_i8.hip:252, conv3x3_prw_i8.hip:232); for code outputs
         sh + 128 rounded, + delta[cls] rounded (border pixels), (float)acc * sc + sj as ONE fma (the span of the contracted and the
         uncontracted form decides what is MARKED), fmaxf(., lo_clamp + 128), the 2x2 max before rounding for `pool`, round to nearest
         even with saturation to [0, 255] (v_cvt_pk_u8_f32), ^ 0x80.  The PixelShuffle channel permutation of the packer (np -> 4 (np %
         cps) + np / cps) with the kernels' addressing Y = 2 oy + (sub >> 1), X = 2 ox + (sub & 1) IS torch's PixelShuffle in natural
         channel order, which is how it is written here.  ps_dot3: delta_acc added to the integer sum, fmaxf(acc * sc + sh, 0), the f16
         rounding, the three dot products with conv10's first 64 inputs as f16 hi + lo 2^-10 pairs in fp32 accumulation (H.HRounded.dot,
         H.split_pair).  conv1: v_cvt_pk_u8_f32((float)v_f16 * hg_q0_inv + (hg_q0_zero + 128)) on the pooled f16 value.
  d      derived, never measured.  With sc32 = sc (1 + e1), sh32 = sh (1 + e2), s128 = (sh32 + 128)(1 + e3), delta32 = delta (1 + e5),
         sj = (s128 + delta32)(1 + e6), the product (1 + e7) where the form is uncontracted, the sum (1 + e4), |e| <= U32, and (float)acc
         rounded (1 + e0) only where |acc| >= 2^24:
             |device - (acc sc + sh + 128 + delta)| <= U32 ((3 or 4) |acc sc| + |sh| + |sj| + (|sh| + 128) + [border] (|delta| + |sj|))
         -- that is U32 (3 or 4) |acc sc| + 2 U32 |sh| plus one U32 |.| for each further rounded add, each at the magnitude it
         rounds.  acc sc + sh + delta[cls] is the network's value on the same codes in real arithmetic (the fold is an identity), which
         `layer` ASSERTS on every frame as `fold`: |model's unrounded argument - v's coordinate| <= d at EVERY element, before the
         activation (ReLU / lo_clamp, pool and the rounding are the same monotone maps on both sides) -- so v's own code can differ from
         the model's only where a tie lies within d.  Where read_actq snaps a zero point to an integer (|kf - k| <= 1e-3) the distance
         of the two, x_scale |kf - k| sum|W| |gain| / x_scale' + |kf' - k'|, is part of d; it is 0 for the three checkpoints tested.
         ps_dot3: the same without the + 128 / delta terms, plus half an accumulator unit x_scale w_scale[n] gs / 2 at border pixels of
         a float zero point (the stated cost of delta_acc; the comment in conv3x3_pglds_i8.hip:258-260 says "x_scale * w_scale / 2",
         which omits no factor for Up_conv5: it has no BatchNorm and a real-valued output, gs = 1), then H's terms: half an f16 ulp taken
         sharply with the allowance for a rounding that falls the other way (HBounded.quant), the weight-split term and gamma_66 of the
         fp32 dot products (HBounded.dot).  conv1, prep, final: H's own bounds.

CONDITIONS (tests/test_gpu_hg_i8_layers.py), per launch, output tensor, size and form:
  hard       f16 / fp32 output: |device - v| <= d everywhere.  Code output: device code = model code everywhere, within 1 only at MARKED
             elements (the epilogue span -- the contracted and the uncontracted fp32 form, after clamp and pool -- rounds to two codes);
             marked elements per tensor at most max(2, 1e-3 n) (Q.cap_ok); `fold` = 0 violations.  hg8.p1 is the one quantiser behind
             f16 arithmetic of its own launch (cap = False in Q's terms): the device's f16 value lies in [f16(v - d), f16(v + d)] of
             conv1's own fp32 bound, the pooled ends are quantised by the EVALUATED fma, and the device's code must lie between the two
             codes; the share of elements where they differ is held by wide_ok against the share (f16 distance of the ends) / step.
  precision  mean|device - v| <= 2 mean|model - v|, code tensors in code units against v's float64 coordinate.
  inputs     f16 / fp32: H.input_condition; code tensor: >= 25 % of the model's codes strictly between the clamp (lo_clamp, else 0) and
             255; final: the device's mask 10 .. 90 % ones.
  coverage   `plan` claims every hg.* / hg_* launch, checks every kernel tag, fails on an unclaimed launch and on hg_need.

NOT held this way after this file: le_rows<fq>, agcm_fold<q8> / agcm_mlp<q8> (tests/test_gpu_int8_hr.py).
"""
from __future__ import annotations

import numpy as np
import torch

import hg_layer_ref as H
import le_i8_layer_ref as Q
from hg_layer_ref import FRAMES, REFUSED, U32, Check, as_t, f16, input_condition, metrics, split  # noqa: F401  (re-exported)
from le_i8_layer_ref import CAP_MIN, CAP_SHARE, Codes, _epilogue_span, border_classes, cap_ok, f32  # noqa: F401

# hg_layers' `consumer` column (csrc/api.h:371-389): the layer whose quantiser codes the output; Up_conv5's reader is fp16
CONSUMER = {"conv2": "conv3_1.0", "conv3_1": "conv3_2.0", "conv3_2": "conv4_1.0", "conv4_1": "conv4_2.0", "conv4_2": "conv5_1.0",
            "conv5_1": "conv5_2.0", "conv5_2": "conv_code1.0", "conv_code1": "conv_code2.0", "conv_code2": "Up_conv1.0", "Up_conv1": "conv6",
            "conv6": "Up_conv2.0", "Up_conv2": "conv7", "conv7": "Up_conv3.0", "Up_conv3": "conv8", "conv8": "Up_conv4.0", "Up_conv4": "conv9",
            "conv9": "Up_conv5.0", "Up_conv5": None}
CODE_TENSORS = ("p1",) + tuple(r[10] for r in H.HG_LAYERS if r[0] != "Up_conv5")
TAPS = {t: ("hg8." + t if t in CODE_TENSORS else n) for t, n in H.TAPS.items()}
STAGES, BY_NAME = H.STAGES, H.BY_NAME
CALIBRATIONS = {"integer": "seeded-w8a8:1234", "minmax": "seeded-w8a8-minmax:1234"}

MUT8 = ("cls_swap", "cls_first", "cls0", "pad_u8_0", "pad128_nodelta", "delta_no_gain", "no_lo_clamp", "pool_after_round", "trunc", "wrap",
        "cat_swap", "ps_swap", "conv9_pad_real", "no_f16", "no_lo", "no_delta_acc", "c1_fp32", "other_zero")


class ActQ:
    """read_actq (api_pack.hip:82-93): value = scale (q - kf), q the u8 code; kf snaps to an integer k in 0..255 within 1e-3."""

    def __init__(self, sd, layer):
        self.xs = float(np.asarray(sd[layer + ".x_scale"], np.float32).reshape(-1)[0])
        self.xz = float(np.asarray(sd[layer + ".x_zero"], np.float32).reshape(-1)[0])
        self.kf_true = -self.xz / self.xs
        k = float(np.rint(self.kf_true))
        self.integer = abs(self.kf_true - k) <= 1e-3 and 0 <= k <= 255
        self.kf = k if self.integer else self.kf_true


class L8:
    """One row of hg_layers with its W8A8 tensors (weight_int8 kept as int8: the head has 35 M of them)."""

    def __init__(self, row, sd):
        self.name, co, ci, self.skip_cin, self.k, self.ps, self.mode, self.relu, self.src, self.skip, self.dst, bn = row
        wn = self.name + ".0" if self.k == 3 else self.name
        self.wname, self.cin = wn, ci
        self.w8i = torch.from_numpy(np.ascontiguousarray(np.asarray(sd[wn + ".weight_int8"], np.int8)))
        self.ws = as_t(np.asarray(sd[wn + ".w_scale"], np.float32).reshape(-1))
        self.b = as_t(np.asarray(sd[wn + ".bias"], np.float32))
        self.q = ActQ(sd, wn)
        self.o = ActQ(sd, CONSUMER[self.name]) if CONSUMER[self.name] else None
        self.bn = tuple(as_t(np.asarray(sd[f"{bn}.{k}"], np.float32)) for k in ("weight", "bias", "running_mean", "running_var")) if bn else None

    @property
    def w8(self):
        return self.w8i.double()

    def gain(self):
        """BatchNorm's gain g / sqrt(var + 1e-5) in float64 (pack_conv_i8 :141), 1 without BatchNorm."""
        return self.bn[0] / torch.sqrt(self.bn[3] + 1e-5) if self.bn else torch.ones_like(self.ws)


class Pack8:
    """fp: H.pack's dict for the fp16 launches (conv1, conv10's halves, conv_last); L: the 18 W8A8 rows; q0: conv2.0's quantiser."""

    def __init__(self, sd, mask_r=0.75):
        class _NoW(dict):          # H.pack also packs the 18 rows' fp16 weights, which a W8A8 checkpoint does not have and nothing here reads
            def __missing__(self, k):
                if k.endswith(".weight"):
                    return np.zeros(1, np.float32)
                raise KeyError(k)
        self.sd = sd
        self.fp = {k: v for k, v in H.pack(_NoW(sd), True, mask_r).items() if k not in CONSUMER}
        self.L = {r[0]: L8(r, sd) for r in H.HG_LAYERS}
        self.q0 = ActQ(sd, "conv2.0")

    def with_mask_r(self, r):
        self.fp["mask_r"] = float(r)
        return self


def pack(sd, mask_r=0.75):
    return Pack8(sd, mask_r)


# ------------------------------------------------------------------------------------------------- the packer, restated
def tables(L, mut=None, other=None):
    """pack_conv_i8's constants -> dict(sc, sh, delta [16, Co], dacc [16, Co], lo, need) as fp32 values in float64, and the unrounded
    sc / sh / delta (`x_`) for the bound."""
    q, o = L.q, L.o
    kf = other if mut == "other_zero" else q.kf
    w8 = L.w8
    a = q.xs * L.ws
    wsum = w8.sum(dim=(1, 2, 3))
    gs = L.gain()
    sc, sh = a * gs, a * (128.0 - kf) * wsum + L.b
    if L.bn:
        sh = (sh - L.bn[2]) * gs + L.bn[1]
    if o:
        sc, sh, gs = sc / o.xs, sh / o.xs + o.kf - 128.0, gs / o.xs
    need = L.k == 3 and kf != 128.0
    delta = torch.zeros((16, a.numel()), dtype=torch.float64)
    dacc, dacc_x = delta.clone(), delta.clone()
    if need:
        L_ = type("T", (), {"w8": w8, "k": 3})
        miss = wsum[None] - Q.class_sums(L_)                               # [16, Co]: weight sums over the taps OUTSIDE the image
        gd = (torch.ones_like(gs) / (o.xs if o else 1.0)) if mut == "delta_no_gain" else gs
        delta = -a[None] * (128.0 - kf) * miss * gd[None]
        dacc_x = -(128.0 - kf) * miss
        dacc = torch.round(dacc_x)                                         # nearbyint: ties to even
    lo = float(min(255.0, max(0.0, np.rint(o.kf))) - 128.0) if (L.relu and o) else -128.0
    return {"sc": f32(sc), "sh": f32(sh), "delta": f32(delta), "dacc": dacc, "lo": lo, "need": need, "x_sc": sc, "x_sh": sh, "x_delta": delta,
            "dacc_res": (dacc - dacc_x).abs()}


def classes(L, h, w, mut=None):
    cls = border_classes(h, w, L.k, 1, mut == "cls_swap")
    if mut == "cls_first":                          # a both-bits class (one-row / one-column map) taken as its first bit only
        rb, cb = cls >> 2, cls & 3
        cls = (torch.where(rb == 3, torch.ones_like(rb), rb) << 2) | torch.where(cb == 3, torch.ones_like(cb), cb)
    if mut in ("cls0", "pad128_nodelta"):           # padding as int8 code 0 (u8 128) WITHOUT its correction = class 0's constants everywhere
        cls = torch.zeros_like(cls)
    return cls


def _rne_u8(x, trunc=False, wrap=False):
    q = torch.floor(x) if trunc else torch.round(x)
    return (torch.remainder(q, 256.0) if wrap else torch.clamp(q, 0, 255)) - 128.0


def _post(L, x, lo128, mut=None):
    """The code epilogue behind the fp32 argument x (u8 coordinate): clamp, shuffle, pool BEFORE rounding, round, saturate, ^ 0x80."""
    if mut == "pool_after_round":                   # the clamp and the rounding first, the pool on the codes: must not differ
        y = _rne_u8(torch.clamp(x, min=lo128))
        y = H._ps2(y) if L.ps else y
        return H._pool(y) if L.mode == "pool" else y
    y = x if mut == "no_lo_clamp" else torch.clamp(x, min=lo128)
    if L.ps:
        y = H._ps2(y, mut == "ps_swap")
    if L.mode == "pool":
        y = H._pool(y)
    return _rne_u8(y, mut == "trunc", mut == "wrap")


def _cat(L, ins, swap=False):
    if len(ins) == 1:
        return ins[0]
    return torch.cat((ins[1], ins[0]) if swap else (ins[0], ins[1]))


def network(L, c):
    """v before the activation, real units: W8A8Conv2d.forward + BatchNorm2d(eval) in float64 on the input codes c (int8)."""
    x = (c + 128.0) * L.q.xs + L.q.xz
    y = H._conv(x, L.w8 * L.ws[:, None, None, None], 1) + L.b[:, None, None]
    if L.bn:
        g, be, mu, var = (t[:, None, None] for t in L.bn)
        y = (y - mu) * g / torch.sqrt(var + 1e-5) + be
    return y


def layer(L, P, ins, mut=None, other=None, model_only=False):
    """One int8 launch on its input codes -> {out: result dict}, marks.  Result: v / d / model (R.metrics' operands), v_prec, codes,
    fold (elements at which the folded form leaves the network form's bound), between (code tensors: share of the model's codes
    strictly between the clamp and 255)."""
    c = _cat(L, ins, mut == "cat_swap")
    T = tables(L, mut, other)
    acc = Q._pad_conv(c, L.w8, 1, -128.0 if (mut == "pad_u8_0" and L.k == 3) else 0.0)
    h, w = c.shape[-2:]
    cls = classes(L, h, w, mut)
    sc = T["sc"][:, None, None]
    dot3 = L.mode == "ps_dot3"
    if dot3:
        if T["need"] and mut != "no_delta_acc":
            acc = acc + T["dacc"][cls].permute(2, 0, 1)
        sj = T["sh"][:, None, None].expand_as(acc)
    else:
        sj = f32(f32(T["sh"] + 128.0)[None] + T["delta"])[cls].permute(2, 0, 1)          # [Co, h, w]: (sh + 128) rounded, + delta rounded
    a32 = f32(acc)                                                                        # (float)acc: exact below 2^24
    u = f32(a32 * sc + sj)                                                                # ONE fma
    if dot3:
        m = H.HRounded(mut if mut in ("ps_swap", "no_lo") else None)
        x = torch.clamp(m.ps(u), min=0.0)
        model = m.dot(x if mut == "no_f16" else f16(x), P.fp["w10a"], True)
    else:
        model = _post(L, u, T["lo"] + 128.0, mut)
        if mut == "conv9_pad_real" and L.name == "conv9":      # the 128-wide tile's padded half stored too and read as a 64-channel tensor
            full = torch.cat((model, torch.zeros_like(model)))                             # scale = shift = 0 there: u8 128 = int8 0
            model = full.permute(1, 2, 0).reshape(-1)[:model.numel()].reshape(h, w, -1).permute(2, 0, 1).contiguous()
    if model_only:
        return {L.dst: {"model": model}}, []
    # ---- v and d
    y = network(L, c)
    border = (cls != 0).double()[None] if T["need"] else torch.zeros((1, h, w), dtype=torch.float64)
    big = (acc.abs() >= 2.0 ** 24).double()
    asc = (a32 * T["x_sc"][:, None, None]).abs()
    xsh = T["x_sh"].abs()[:, None, None]
    o = L.o
    snap = 0.0
    if L.q.kf != L.q.kf_true or (o and o.kf != o.kf_true):
        gsx = (L.gain() / (o.xs if o else 1.0)).abs()[:, None, None]
        snap = abs(L.q.kf - L.q.kf_true) * L.q.xs * H._conv(torch.ones_like(c), (L.w8 * L.ws[:, None, None, None]).abs(), 1) * gsx + (abs(o.kf - o.kf_true) if o else 0.0)
    if dot3:
        t = y
        d = 1.01 * U32 * ((3.0 + big) * asc + 2.0 * xsh) + border * (T["dacc_res"][cls].permute(2, 0, 1) > 0).double() * 0.5 * T["x_sc"].abs()[:, None, None] + snap
    else:
        t = (y - o.xz) / o.xs                                                             # v's u8 coordinate before the activation
        xdl = T["x_delta"][cls].permute(2, 0, 1).abs()
        sjm = xsh + 128.0 + xdl
        d = 1.01 * U32 * ((3.0 + big) * asc + xsh + sjm + (xsh + 128.0) + border * (xdl + sjm)) + snap
    fold = int(((u - t).abs() > d).sum())
    lo, hi = _epilogue_span(a32, sc, sj)
    if dot3:
        b = H.HBounded()
        x = b.act(b.ps((y, d)), 0.0)
        v, dv = b.dot(b.quant(x), P.fp["w10a"], True)
        vp = H.HBounded(sharp=False)
        v_prec = vp.dot(vp.quant(x), P.fp["w10a"], True)[0]
        return {L.dst: {"v": v, "d": dv, "model": model, "v_prec": v_prec, "codes": False, "fold": fold}}, []
    lo128 = T["lo"] + 128.0
    clo, chi = _post(L, lo, lo128), _post(L, hi, lo128)
    marked = clo != chi
    # v's own code: ReLU in the coordinate is max(t, kf'), then shuffle / pool / the reader's quantiser
    tv = torch.clamp(t, min=o.kf_true) if L.relu else t
    tv = H._ps2(tv) if L.ps else tv
    tv = H._pool(tv) if L.mode == "pool" else tv
    netq = torch.clamp(torch.round(tv), 0, 255) - 128.0
    floor_code = lo128 - 128.0 if L.relu else -128.0
    between = float(((model > floor_code) & (model < 127.0)).double().mean())
    res = {"v": model, "d": marked.double(), "model": model, "v_prec": torch.clamp(tv, 0, 255) - 128.0, "codes": True, "fold": fold, "netq": netq,
           "between": between, "ref": Codes(netq, clo, chi, tv, None, torch.clamp(tv, 0, 255) - 128.0)}
    return {L.dst: res}, [(L.name + "->" + (CONSUMER[L.name] or ""), int(marked.sum()), marked.numel(), True, 0.0)]


# ------------------------------------------------------------------------------------------------- conv1: the fp16 -> int8 boundary
def _q0(P, x, sgn=0.0):
    """v_cvt_pk_u8_f32((float)x * hg_q0_inv + (hg_q0_zero + 128)) ^ 0x80 (le_hg_misc.hip:237-246; api_pack.hip:849-850)."""
    inv = float(np.float32(1.0) / np.float32(P.q0.xs))
    z128 = float(np.float32(np.float32(P.q0.kf - 128.0) + np.float32(128.0)))
    tk = x * inv + z128
    return torch.clamp(torch.round(f32(tk + sgn * 2.0 ** -50 * ((x * inv).abs() + abs(z128)))), 0, 255) - 128.0


def conv1(P, taps, mut=None, model_only=False):
    m = H.HRounded()
    ym = m.act(m.convbn(taps["img"], P.fp["conv1"]), 0.0)
    mp1 = _q0(P, H._pool(ym if mut == "c1_fp32" else f16(ym)))
    mpart2 = m.dot(m.quant(ym), P.fp["w10b"], False)
    if model_only:
        return {"p1": {"model": mp1}, "part2": {"model": mpart2}}, []
    res = H.evaluate(Check(["conv1"], by_name=H.BY_NAME, taps=H.TAPS), P.fp, taps)
    part2 = dict(res["part2"], codes=False, fold=0)
    b = H.HBounded()
    v, d0 = b.act(b.convbn(b.inp(taps["img"]), P.fp["conv1"]), 0.0)                      # conv1's own fp32 bound, before the f16 store
    plo, phi, pv = H._pool(f16(v - d0)), H._pool(f16(v + d0)), H._pool(v)
    lo, hi = _q0(P, plo, -1.0), _q0(P, phi, 1.0)
    tv = torch.clamp((pv - P.q0.xz) / P.q0.xs, 0, 255) - 128.0
    between = float(((mp1 > -128.0) & (mp1 < 127.0)).double().mean())
    p1 = {"v": 0.5 * (lo + hi), "d": 0.5 * (hi - lo), "model": mp1, "v_prec": tv, "codes": True, "fold": 0, "between": between,
          "netq": torch.round(tv), "ref": Codes(torch.round(tv), lo, hi, pv, None, tv)}
    expect = float(torch.clamp((phi - plo) / P.q0.xs, max=1.0).mean())
    return {"p1": p1, "part2": part2}, [("conv1->conv2.0", int((hi != lo).sum()), lo.numel(), False, expect)]


# ------------------------------------------------------------------------------------------------- checks
def evaluate(check, P, taps, mut=None, other=None, model_only=False):
    """One check (one launch) on `taps` -> ({out: result}, marks)."""
    name = check.stages[0].name
    assert len(check.stages) == 1
    if name == "conv1":
        return conv1(P, taps, mut, model_only)
    if name in P.L:
        L = P.L[name]
        return layer(L, P, [taps[L.src]] + ([taps[L.skip]] if L.skip else []), mut, other, model_only)
    if model_only:
        got = check.run(H.HRounded(), P.fp, taps)
        return {t: {"model": got[t]} for t in check.outs}, []
    res = H.evaluate(check, P.fp, taps)
    return {t: dict(r, codes=False, fold=0) for t, r in res.items()}, []


def input_ok(t, r):
    """The input condition of one output -> (ok, share).  Code tensor: 25 % of the model's codes strictly between the clamp and 255."""
    if r["codes"]:
        return r["between"] >= 0.25, r["between"]
    if t in H.EXACT:
        return True, 1.0
    ok, share, _ = input_condition(r)
    return ok, share


def _allowed(name):
    if name == "prep":
        return {"hg_prep"}
    if name == "conv1":
        return {"conv_c3<64,dot3>"}
    if name == "final":
        return {"hg_final_light"}
    row = next(r for r in H.HG_LAYERS if r[0] == name)
    _, cout, cin, skip_cin, ks, _ps, mode, *_ = row
    if ks == 1:
        return {"conv1x1_i8"}
    if cin == 64:
        return {f"conv_pglds_i8<{mode},c64>"}
    assert cout % 256 == 0
    return {f"conv_pglds_i8<{mode}>", f"conv_prw_i8<{mode}>", f"conv_prw8_i8<{mode}>"}


PRW_LAYERS = tuple(r[0] for r in H.HG_LAYERS if r[4] == 3 and r[2] != 64)          # the 3x3 rows Seq::conv8 may route to conv_prw_i8
# every kernel tag Seq::c3 and Seq::conv8 (csrc/api_graph.hip:103-139, :167-179) can emit for this head's table, with hg_prep and the tail
KERNEL_TAGS = tuple(sorted(set().union(*(_allowed(s.name) for s in STAGES))))


def plan(profile):
    """(layer, kernel) records of one profiled frame -> [Check], one per launch.  An HG launch no check claims, a missing launch, a
    need-list launch or a kernel tag the layer cannot have fails."""
    recs = [(l, k) for l, k, *_ in profile if l.startswith(("hg.", "hg_", "HG."))]
    ran = [l for l, _ in recs]
    assert "hg_need" not in ran, "the frame ran with need lists"
    by_key = {s.key: s for s in STAGES}
    assert sorted(ran) == sorted(by_key), ("HG launches without a check / checks without a launch", sorted(set(ran) ^ set(by_key)))
    for l, k in recs:
        assert k in _allowed(by_key[l].name), (l, k, sorted(_allowed(by_key[l].name)))
    return [Check([by_key[l].name], by_name=BY_NAME, taps=TAPS) for l in ran]


def dense_profile(prw=""):
    """The records of one frame, for planning without a device; prw: "", "prw" or "prw8" for the rows that can take that kernel."""
    out = []
    for s in STAGES:
        tags = sorted(_allowed(s.name))
        pick = [k for k in tags if prw and k.startswith(f"conv_{prw}_i8<")] or [k for k in tags if "prw" not in k]
        out.append((s.key, pick[0]))
    return out


def model_env(P, le_out, mut=None, other=None):
    """Every stage's MODEL in order on one LE output -> {logical tensor: value as the device hands it out}."""
    e = {"le.out": le_out}
    for s in STAGES:
        c = Check([s.name], by_name=BY_NAME, taps=TAPS)
        res, _ = evaluate(c, P, e, mut, other, model_only=True)
        for t, r in res.items():
            e[t] = r["model"] if t in CODE_TENSORS else (r["model"].float().double() if t in H.F32_OUTS else f16(r["model"]))
    return e
