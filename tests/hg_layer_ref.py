"""Float64 reference of ONE launch of the HG head's fp16 path, with an a-priori error bound.  TEST INFRASTRUCTURE ONLY.

Built on tests/le_layer_ref.py (read its docstring first): the same two evaluators -- `Bounded`, every value a pair (v, d) with d DERIVED
from the arithmetic (eps = 2^-11 at an f16 store, gamma_K = K 2^-24 over a reduction of K fp32 terms), and `Rounded`, the same graph
with the roundings applied where the kernels apply them -- extended by the primitives the head needs (csrc/ =
hdr-realtime-video-pipeline_amd/csrc/):

  convbn    conv + the epilogue `acc * scale + shift` in fp32 (conv3x3_prw.hip:284-287, conv3x3_pglds.hip:257-260, conv1x1_glds.hip:154-157
            and :336-339, le_hg_misc.hip:160-163).  scale / shift are api_pack.hip's fold, reproduced in float32 operation by operation
            (pack_conv :55-59, pack_c3 :473-475):  s = g / sqrtf(var + 1e-5f),  shift = (b - mu) * s + be;  without BatchNorm scale = 1,
            shift = bias.  Weights are rounded to f16 as pack_conv :63 / pack_c3 :485 round them.
                d_y = |s| |W| d_x + gamma_(K+2) |s| |W| (|x| + d_x) + 2 * 2^-24 |shift|,   K <= Cin k k the number of products of
            that output element that are not exactly 0 (adding an exact 0 rounds nothing: padding, and the zeros a ReLU leaves)
            (the accumulator starts at 0 and the shift enters in the epilogue only: the K products, the multiply by s and the add
            act on the sum; the shift sees the add's rounding and one unit in the last place of its own, should the host compiler
            contract the fold).
  pool      2x2 max of the STORED f16 values (conv3x3_prw.hip:386 and :396, le_hg_misc.hip:230-232): on v and on d -- the maximum of
            four values each within d_i of v_i lies within max d_i of max v_i.
  cat       channel concatenation, the input first and the skip behind it (HgLayer::cin, api.h:324; Seq::conv's src0 / src1).
  pad32     reflect padding at the bottom / right to a multiple of 32 (hg_prep, le_hg_misc.hip:391-397): a copy, d = 0 -- bit-exact.
  mask      hg_prep's highlight mask (le_hg_misc.hip:398-401):  m = (max(r, g, b) - mask_r) / (1 - mask_r) in fp32,  mask = m > 0.1f.
            The float64 value decides it except where it lies within the fp32 arithmetic's reach of the threshold,
            4 * 2^-24 (|max| + r) / (1 - r) + 2 * 2^-24 |m| (the subtraction, 1 - r, the division and its operands); there d = 1
            (either answer).  The inputs are f16 values, 2^-11-spaced near the threshold, so for a given mask_r the number of such
            pixels is known without a frame: `mask_uncertain_values(r)` walks every f16 value in [0, 2] -- it is 0 for every
            mask_r of FRAMES (tests/test_hg_layer_ref_host.py asserts that), so the device's mask must be the reference's at every pixel.
  dot       the fused 64 -> 3 sums of conv10's two halves, fp32 outputs:
              hg.part   Up_conv5's epilogue (conv3x3_prw.hip:132-141 table, :338-349 and :364 sums; conv3x3_pglds.hip:130-141, :345
                        is the same chain): each fp32 weight as the f16 pair hi = f16(w), lo = f16((w - hi) 1024); per 32-channel half
                        ah = sum hi x, al = sum lo x on the matrix pipe (fp32), R = ah + al / 1024, then R0 + R1.
              hg.part2  conv1's epilogue (le_hg_misc.hip:172): ONE f16 weight -- w2frag is (f16)w10 (api_pack.hip:870), no hi / lo
                        pair: conv10's second half is rounded like every other weight, and v is taken with that rounded weight.
                d = |w| d_x + |w - w_rep| (|x| + d_x) + gamma_66 |w_rep| (|x| + d_x)
            w_rep = hi + lo / 1024 computed exactly (|w - w_rep| <= 2^-22 |w|: the "weight-split term"); gamma_66: 64 products + the
            two adds.  The rounding model accumulates these sums in float32, channel by channel -- the only rounding of an fp32 output
            besides the f16 store of x in front of it; the precision condition is taken against that.  x itself never reaches
            memory: see `quant`, and tests/test_hg_layer_ref_host.py for what that costs the bound (a DROPPED lo half stays inside it
            on a frame's dense input; a lo half with the wrong scale does not).
  final     hg_final_light (le_hg_misc.hip:566-576): conv10 = f16((part2 + part) + b10) (:566, two fp32 adds), conv_last over
            cat(conv10, img) in fp32 (:572-574: bias + 6 products, gamma_12, fp32 weights as put_f32 stores them) rounded to f16
            (:575), out = 1 * v + img in fp32 at masked pixels (:576, one rounding) and img itself elsewhere (d = 0), cropped to H x W.
  quant     an f16 rounding inside a launch whose result feeds fp32 arithmetic of the same launch (the operands of `dot`, conv10 and
            conv_last in `final`): HBounded.quant takes it sharply, and `evaluate` keeps the unrounded value beside it as v_prec.

The f16 stores that are modelled: every tensor a layer writes -- `(f16)fmaxf(acc * sc + sh, act_lb)` (the lines above); the pooled
layers store first and pool the f16 values; the Up blocks shuffle, clamp and store (the shuffle is an index map: conv3x3_prw.hip:317);
conv1's activations are f16 (le_hg_misc.hip:160-163) both for the pooled map and as the B operand of its dot products (:166);
Up_conv5's are f16 as the B operand of theirs (conv3x3_prw.hip:342-343).

Weights: `weights.seeded_hg_state(1234)`.  conv10's first half and conv_last stay fp32 (put_f32, api_pack.hip:852-861).

STAGES, one entry per launch of `run_hg` (csrc/api_graph.hip:720-811) in its dense form, profile key in brackets.  Every HG tensor has
its own workspace slot, so every launch is checked alone on the device's own input taps:

  prep      [hg_prep]        le.out -> img, mask                         img and mask exact (see `mask`)
  conv1     [hg.conv1]       img -> p1, part2                            the full-resolution conv1 never exists
  conv2 .. conv_code2, Up_conv1 .. Up_conv4, conv6 .. conv9              HG_LAYERS below = hg_layers (csrc/api.h:334-354)
  Up_conv5  [hg.Up_conv5]    conv9 -> part                               fp32, bound with the weight-split term
  final     [hg_final]       (img, mask, part, part2) -> out
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from le_layer_ref import (EPS, U32, Bounded, Check, Rounded, Stage, _conv, _half_ulp, _ps2, as_t, f16,  # noqa: F401  (re-exported)
                          input_condition, metrics, split)

THRESH = float(np.float32(0.1))         # hg_prep's `thresh` argument (api_graph.hip:743)

# (name, cout, cin, skip_cin, ks, ps, mode, relu, in, skip, out, bn) -- csrc/api.h:334-354, launch order
HG_LAYERS = (
    ("conv2", 128, 64, 0, 3, 0, "nhwc", True, "p1", None, "conv2", "conv2.1"),
    ("conv3_1", 256, 128, 0, 3, 0, "pool", True, "conv2", None, "p3", "conv3_1.1"),
    ("conv3_2", 256, 256, 0, 3, 0, "nhwc", True, "p3", None, "conv3_2", "conv3_2.1"),
    ("conv4_1", 512, 256, 0, 3, 0, "pool", True, "conv3_2", None, "p4", "conv4_1.1"),
    ("conv4_2", 512, 512, 0, 3, 0, "nhwc", True, "p4", None, "conv4_2", "conv4_2.1"),
    ("conv5_1", 512, 512, 0, 3, 0, "pool", True, "conv4_2", None, "p5", "conv5_1.1"),
    ("conv5_2", 512, 512, 0, 3, 0, "nhwc", True, "p5", None, "conv5_2", "conv5_2.1"),
    ("conv_code1", 512, 512, 0, 3, 0, "pool", True, "conv5_2", None, "pc", "conv_code1.1"),
    ("conv_code2", 512, 512, 0, 3, 0, "nhwc", True, "pc", None, "conv_code2", "conv_code2.1"),
    ("Up_conv1", 2048, 512, 0, 3, 512, "ps", True, "conv_code2", None, "up1", ""),
    ("conv6", 512, 1024, 512, 1, 0, "nhwc", False, "up1", "conv5_2", "conv6", ""),
    ("Up_conv2", 2048, 512, 0, 3, 512, "ps", True, "conv6", None, "up2", ""),
    ("conv7", 256, 1024, 512, 1, 0, "nhwc", False, "up2", "conv4_2", "conv7", ""),
    ("Up_conv3", 1024, 256, 0, 3, 256, "ps", True, "conv7", None, "up3", ""),
    ("conv8", 128, 512, 256, 1, 0, "nhwc", False, "up3", "conv3_2", "conv8", ""),
    ("Up_conv4", 512, 128, 0, 3, 128, "ps", True, "conv8", None, "up4", ""),
    ("conv9", 64, 256, 128, 1, 0, "nhwc", False, "up4", "conv2", "conv9", ""),
    ("Up_conv5", 256, 64, 0, 3, 64, "ps_dot3", True, "conv9", None, "part", ""),
)


def _pool(x, shift=False):
    if shift:                                           # mutation: the window one pixel down / right (last row / column repeated)
        x = torch.cat((x[:, 1:], x[:, -1:]), 1)
        x = torch.cat((x[:, :, 1:], x[:, :, -1:]), 2)
    return F.max_pool2d(x[None], 2)[0]


def _pad32(x, zero=False):
    ph, pw = (-x.shape[-2]) % 32, (-x.shape[-1]) % 32
    if not (ph or pw):
        return x
    return F.pad(x[None], (0, pw, 0, ph), mode="constant" if zero else "reflect")[0]


def split_pair(w):
    """An fp32 weight as the kernels' f16 pair: (hi, lo) with lo scaled by 1024 (conv3x3_prw.hip:139-140), float64 holding exact values.
    (w - hi) and its product with 1024 are exact in fp32: hi is w's own leading 11 bits."""
    hi = f16(w)
    lo = f16((w - hi) * 1024.0)
    return hi, lo


def mask_value(mx, r):
    """float64 m of hg_prep for the f16 maxima `mx`, with the reach of the fp32 evaluation around it."""
    r = float(np.float32(r))
    m = (mx - r) / (1.0 - r)
    reach = 4 * U32 * (mx.abs() + r) / (1.0 - r) + 2 * U32 * m.abs()
    return m, reach


def mask_uncertain_values(r):
    """How many f16 values in [0, 2] a pixel's maximum could take at which fp32 arithmetic may put m on the other side of the threshold."""
    allv = torch.from_numpy(np.arange(0, 0x4001, dtype=np.uint16).view(np.float16).astype(np.float64))      # 0 .. 2.0
    m, reach = mask_value(allv, r)
    return int(((m - THRESH).abs() <= reach).sum())


class HBounded(Bounded):
    def __init__(self, sharp=True):
        self.sharp = sharp

    def quant(self, x):
        """An f16 rounding INSIDE a launch, in front of arithmetic that continues in fp32 (the operands of the fused dot products,
        conv10 and conv_last in the tail).  sharp: the value is taken rounded, v <- f16(v) -- rounding is monotone, so the device's
        f16(v + delta), |delta| <= d, lies in [f16(v - d), f16(v + d)]: d <- the larger distance of the two from f16(v), which is 0
        wherever no rounding boundary lies within d of v.  Carried as a worst case (not sharp: `store`) the 64 operand roundings of
        a dot product, 2^-12 relative each, would hide everything finer -- the 2^-22 weight-split term first of all."""
        if not self.sharp:
            return self.store(x)
        v, d = x
        q = f16(v)
        return (q, torch.maximum(f16(v + d) - q, q - f16(v - d)))

    def convbn(self, x, L):
        v, d = x
        w, sc, sh = L["w"], L["sc"], L["sh"]
        s = sc[:, None, None]
        y = _conv(v, w, 1) * s + sh[:, None, None]
        mag = _conv(v.abs() + d, w.abs(), 1)
        g = (_conv((v.abs() + d > 0).double(), (w != 0).double(), 1) + 2) * U32           # K: the products that are not exactly 0
        dy = s.abs() * (_conv(d, w.abs(), 1) if bool(d.any()) else 0.0) + g * s.abs() * mag + 2 * U32 * sh.abs()[:, None, None]
        return (y, dy)

    def pool(self, x):
        return (_pool(x[0]), _pool(x[1]))

    def cat(self, a, b):
        return (torch.cat((a[0], b[0])), torch.cat((a[1], b[1])))

    def pad32(self, x):
        return (_pad32(x[0]), _pad32(x[1]))

    def mask(self, img, r):
        m, reach = mask_value(img[0].max(0, keepdim=True)[0], r)
        return ((m > THRESH).double(), ((m - THRESH).abs() <= reach).double())

    def dot(self, x, w, pair):
        v, d = x
        if pair:
            hi, lo = split_pair(w)
            rep = hi + lo / 1024.0
        else:
            rep = w
        mag = v.abs() + d
        e = lambda a, b: torch.einsum("oc,chw->ohw", a, b)      # noqa: E731
        return (e(w, v), e(w.abs(), d) + e((w - rep).abs(), mag) + 66 * U32 * e(rep.abs(), mag))

    def add3(self, a, b, c):
        v = a[0] + b[0] + c[:, None, None]
        d = a[1] + b[1]
        return (v, d + 2 * U32 * (a[0].abs() + b[0].abs() + c.abs()[:, None, None] + d))

    def c10(self, x):
        return self.quant(x)

    def lin6(self, c10, img, wl, bl):
        x = torch.cat((c10[0], img[0]))
        dx = torch.cat((c10[1], img[1]))
        e = lambda a, b: torch.einsum("oc,chw->ohw", a, b)      # noqa: E731
        return (e(wl, x) + bl[:, None, None], e(wl.abs(), dx) + 12 * U32 * (e(wl.abs(), x.abs() + dx) + bl.abs()[:, None, None]))

    def blend(self, t, img, mask, hw):
        on = mask[0] > 0
        v = torch.where(on, t[0] + img[0], img[0])
        d = torch.where(on, t[1] + U32 * ((t[0] + img[0]).abs() + t[1]), torch.zeros_like(v))
        return (v[:, :hw[0], :hw[1]], d[:, :hw[0], :hw[1]])


class HRounded(Rounded):
    """The rounding model of the head; `mut` switches ONE deliberate mistake on (tests/test_hg_layer_ref_host.py)."""
    MUTATIONS = ("zero_tap", "no_shift", "pool_shift", "cat_swap", "ps_swap", "zero_pad", "no_lo", "lo_unscaled", "c10_f32", "blend_all", "acc16")

    def quant(self, x):
        return self._r(x)

    def convbn(self, x, L):
        w, sc, sh = L["w"], L["sc"], L["sh"]
        k = w.shape[-1]
        if self.mut == "zero_tap" and k == 3:
            w = w.clone()
            w[:, :, 0, 2] = 0.0
        if self.mut == "no_shift":
            sh = torch.zeros_like(sh)
        if self.mut == "acc16" and k == 3:
            # the accumulator rounded to f16 after every `chunk` terms (K order: tap, then channels)
            acc = torch.zeros(1, dtype=torch.float64)
            for ky in range(3):
                for kx in range(3):
                    for c0 in range(0, w.shape[1], self.chunk):
                        w1 = torch.zeros_like(w)
                        w1[:, c0:c0 + self.chunk, ky, kx] = w[:, c0:c0 + self.chunk, ky, kx]
                        acc = f16(acc + _conv(x, w1, 1))
        else:
            acc = _conv(x, w, 1)
        return acc * sc[:, None, None] + sh[:, None, None]

    def pool(self, x):
        return _pool(x, self.mut == "pool_shift")

    def cat(self, a, b):
        return torch.cat((b, a) if self.mut == "cat_swap" else (a, b))

    def pad32(self, x):
        return _pad32(x, self.mut == "zero_pad")

    def mask(self, img, r):
        mx = img.max(0, keepdim=True)[0].float()                # hg_prep's own fp32 expressions
        r32 = torch.tensor(r, dtype=torch.float32)
        m = ((mx - r32) / (1.0 - r32)).clamp(0.0, 1.0)
        return (m > torch.tensor(0.1, dtype=torch.float32)).double()

    def dot(self, x, w, pair):
        if self.exact:
            return torch.einsum("oc,chw->ohw", w, x)
        xf = x.float()

        def chain(wv, c0, c1):                                   # fp32 accumulation, one channel after the other
            acc = torch.zeros((wv.shape[0],) + tuple(x.shape[1:]), dtype=torch.float32)
            wf = wv.float()
            for c in range(c0, c1):
                acc = acc + wf[:, c, None, None] * xf[c]
            return acc
        if not pair:
            return chain(w, 0, w.shape[1]).double()
        hi, lo = split_pair(w)
        n = w.shape[1] // 2
        out = None
        for c0 in (0, n):
            r = chain(hi, c0, c0 + n)
            if self.mut != "no_lo":
                r = r + chain(lo, c0, c0 + n) * (1.0 if self.mut == "lo_unscaled" else 1.0 / 1024.0)
            out = r if out is None else out + r
        return out.double()

    def _f32(self, v):
        return v if self.exact else v.float().double()

    def add3(self, a, b, c):
        return self._f32(self._f32(a + b) + c[:, None, None])

    def c10(self, x):
        return x if self.mut == "c10_f32" else self._r(x)

    def lin6(self, c10, img, wl, bl):
        return self._f32(torch.einsum("oc,chw->ohw", wl, torch.cat((c10, img))) + bl[:, None, None])

    def blend(self, t, img, mask, hw):
        on = mask > 0 if self.mut != "blend_all" else torch.ones_like(mask, dtype=torch.bool)
        return torch.where(on, self._f32(t + img), img)[:, :hw[0], :hw[1]]


# ------------------------------------------------------------------------------------------------- weights
def _fold(hg, conv, bn, rounded):
    """(scale, shift) of one layer.  rounded: api_pack.hip's fold in float32, operation by operation (:55-59, :473-475)."""
    b = np.asarray(hg[conv + ".bias"], np.float32)
    if not bn:
        return as_t(np.ones_like(b)), as_t(b)
    g, be, mu, var = (np.asarray(hg[f"{bn}.{k}"], np.float32) for k in ("weight", "bias", "running_mean", "running_var"))
    if rounded:
        s = (g / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
        return as_t(s), as_t(((b - mu) * s + be).astype(np.float32))
    g, be, mu, var, b = (a.astype(np.float64) for a in (g, be, mu, var, b))
    s = g / np.sqrt(var + 1e-5)
    return as_t(s), as_t((b - mu) * s + be)


def pack(hg, rounded=True, mask_r=0.75):
    """The head's operands as float64.  rounded: conv weights f16 (pack_conv :63, pack_c3 :485, w2frag :870), fold in float32;
    conv10's first half, its bias and conv_last fp32 as they are.  rounded = False: the checkpoint itself (the oracle's network)."""
    def w(name):
        a = np.asarray(hg[name + ".weight"], np.float32)
        return as_t(a.astype(np.float16) if rounded else a)
    P = {"mask_r": float(mask_r)}
    sc, sh = _fold(hg, "conv1.0", "conv1.1", rounded)
    P["conv1"] = {"w": w("conv1.0"), "sc": sc, "sh": sh}
    for name, _, _, _, ks, *_rest in HG_LAYERS:
        conv = name + ".0" if ks == 3 else name
        sc, sh = _fold(hg, conv, _rest[-1], rounded)
        P[name] = {"w": w(conv), "sc": sc, "sh": sh}
    w10 = np.asarray(hg["conv10.weight"], np.float32).reshape(3, 128)
    P["w10a"] = as_t(w10[:, :64])
    P["w10b"] = as_t(w10[:, 64:].astype(np.float16) if rounded else w10[:, 64:])
    P["b10"] = as_t(np.asarray(hg["conv10.bias"], np.float32))
    P["wl"] = as_t(np.asarray(hg["conv_last.weight"], np.float32).reshape(3, 6))
    P["bl"] = as_t(np.asarray(hg["conv_last.bias"], np.float32))
    return P


# -------------------------------------------------------------------------------------------------- stages
def s_prep(o, P, e):
    e["img"] = o.pad32(e["le.out"])
    e["mask"] = o.mask(e["img"], P["mask_r"])


def s_conv1(o, P, e):
    y = o.act(o.convbn(e["img"], P["conv1"]), 0.0)
    e["p1"] = o.pool(o.store(y))                                    # le_hg_misc.hip:160-163, :230-232
    e["part2"] = o.dot(o.quant(y), P["w10b"], False)                # the same f16 values as the B operand, :166, :172


def _mk_layer(name, mode, relu, src, skip, dst):
    def fn(o, P, e):
        x = e[src] if skip is None else o.cat(e[src], e[skip])
        y = o.convbn(x, P[name])
        if mode in ("ps", "ps_dot3"):
            y = o.ps(y)
        y = o.act(y, 0.0) if relu else y
        if mode == "ps_dot3":
            y = o.dot(o.quant(y), P["w10a"], True)                  # conv3x3_prw.hip:342-345
        else:
            y = o.store(y)
            if mode == "pool":
                y = o.pool(y)
        e[dst] = y
    return fn


def s_final(o, P, e):
    c10 = o.c10(o.add3(e["part2"], e["part"], P["b10"]))            # le_hg_misc.hip:566
    t = o.quant(o.lin6(c10, e["img"], P["wl"], P["bl"]))            # :572-575
    hw = tuple(o.val(e["le.out"]).shape[-2:])
    e["out"] = o.blend(t, e["img"], e["mask"], hw)                  # :576, the crop :579-586


def _stages():
    S = [Stage("prep", "hg_prep", ["le.out"], ["img", "mask"], s_prep),
         Stage("conv1", "hg.conv1", ["img"], ["p1", "part2"], s_conv1)]
    for name, _, _, _, _, _, mode, relu, src, skip, dst, _ in HG_LAYERS:
        S.append(Stage(name, "hg." + name, [src] + ([skip] if skip else []), [dst], _mk_layer(name, mode, relu, src, skip, dst)))
    S.append(Stage("final", "hg_final", ["img", "mask", "part", "part2", "le.out"], ["out"], s_final))
    return S


STAGES = _stages()
BY_NAME = {s.name: s for s in STAGES}
# logical tensor -> workspace tap ("out" is hdrtv_infer's output tensor); hg.part / hg.part2 are [Hp][Wp][4] fp32, three used
TAPS = {"le.out": "le.out", "img": "hg.img", "mask": "hg.mask", "part": "hg.part", "part2": "hg.part2"}
TAPS.update({t: "hg." + t for s in STAGES for t in s.outs if t not in TAPS and t != "out"})
EXACT = ("img", "mask")             # outputs with d = 0 (mask: but at the uncertain values, of which FRAMES' mask_r have none)


def plan(profile):
    """(layer, kernel) records of one profiled frame -> [Check], one per launch; an HG launch that no check claims is an error, and so
    is a need-list launch (the frame must run dense: with hg_sparse != 0 hdrtv_get_tap re-runs the head before it returns a tensor)."""
    ran = [l for l, *_ in profile if l.startswith(("hg.", "hg_", "HG."))]
    assert "hg_need" not in ran, "the frame ran with need lists"
    by_key = {s.key: s for s in STAGES}
    assert sorted(ran) == sorted(by_key), ("HG launches without a check / checks without a launch", sorted(set(ran) ^ set(by_key)))
    return [Check([by_key[l].name], by_name=BY_NAME, taps=TAPS) for l in ran]


def dense_profile():
    return [(s.key, "") for s in STAGES]


def full_graph(P, le_out, o=None):
    """Every stage in order on one LE output: {logical tensor: value}.  Default o and pack(.., False): the oracle's head in float64."""
    o = o or HRounded(exact=True)
    e = {"le.out": o.inp(le_out)}
    for s in STAGES:
        s.fn(o, P, e)
    return {k: o.val(v) for k, v in e.items()}


def taps_from_graph(env):
    """A float64 environment as the device hands it out: f16 tensors rounded, the fp32 ones (part, part2, out) to float32."""
    return {k: (v.float().double() if k in ("part", "part2", "out") else f16(v)) for k, v in env.items()}


F32_OUTS = ("part", "part2", "out")  # outputs behind a `quant`: see evaluate


def evaluate(check, P, taps, model=None):
    """One check on `taps` -> {out: dict(v, d, model[, v_prec])}.  An output behind a `quant` has two references: v / d of the hard
    condition take the f16 operands rounded, as the launch defines them; v_prec is the float64 value with NO intermediate rounding,
    against which the precision condition  mean|device - v_prec| <= 2 mean|model - v_prec|  is taken (le_layer_ref.metrics) -- the
    device and the model both carry the operand roundings, and a rounding that falls the other way on the device is no loss of
    precision."""
    ref = check.run(HBounded(), P, taps)
    mod = check.run(model or HRounded(), P, taps)
    out = {t: {"v": ref[t][0], "d": ref[t][1], "model": mod[t]} for t in check.outs}
    if any(t in F32_OUTS for t in check.outs):
        plain = check.run(HBounded(sharp=False), P, taps)
        for t in check.outs:
            if t in F32_OUTS:
                out[t]["v_prec"] = plain[t][0]
    return out


# every kernel tag Seq::c3 and Seq::conv (csrc/api_graph.hip:58-80, :176) can emit for an fp16 head, with hg_prep and the tail
KERNEL_TAGS = ("hg_prep", "conv_c3<64,dot3>", "hg_final_light", "conv_glds1",
               "conv_pglds<nhwc>", "conv_pglds<pool>", "conv_pglds<ps>", "conv_pglds<ps_dot3>",
               "conv_prw<nhwc>", "conv_prw<pool>", "conv_prw<ps>", "conv_prw<ps_dot3>",
               "conv_prw8<nhwc>", "conv_prw8<pool>", "conv_prw8<ps>")

# The frames of tests/test_gpu_hg_layers.py: (H, W) -> ((seed, mask_r) of the `noise` frame, (seed, mask_r) of the `gradient` frame),
# weights.synthetic_frame.  mask_r: (median of the oracle's max(r, g, b) of the LE output - 0.1) / 0.9 to three decimals, so that about
# half of the pixels are masked (the test asks for 10 .. 90 % of the device's mask).
#   (96, 160)   maps 48x80, 24x40, 12x20, 6x10, 3x5: whole 16-row tiles at level 1, ragged below, level 5 smaller than a tile
#   (90, 150)   reflect-padded to 96x160: hg_prep's padding, hg_final_light's crop and its scalar path (W & 3 != 0)
#   (272, 480)  padded to 288x480: on 8 workgroups three and more tiles per workgroup down to level 3
#   (17, 68), (68, 17)   padded to 32x96 / 96x32: the smallest frames the head accepts whose level-5 map is one row / one column
#               (8x68 and 68x8 are refused: reflect padding needs Hp - H < H, api_workspace.hip:94-95)
FRAMES = {(96, 160): ((71, 0.501), (72, 0.401)), (90, 150): ((73, 0.503), (74, 0.415)), (272, 480): ((75, 0.502), (76, 0.372)),
          (17, 68): ((77, 0.499), (78, 0.417)), (68, 17): ((79, 0.497), (80, 0.403))}
REFUSED = ((8, 68), (68, 8))
