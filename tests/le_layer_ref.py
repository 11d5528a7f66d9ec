"""Float64 reference of ONE launch of the LE network's fp16 path, with an a-priori error bound.  TEST INFRASTRUCTURE ONLY.

CPU only (torch / numpy in float64, nothing of the device).  A launch is a short list of primitives -- conv, LeakyReLU, SFT,
PixelShuffle(2), the `_align_to` crop, residual add, "store as fp16" -- written ONCE against an `ops` object and evaluated by

    Bounded   every value as a pair (v, d): v in float64 with no intermediate rounding, d an elementwise bound on
              |device - v| DERIVED from the arithmetic, with  eps = 2^-11 (fp16 unit roundoff),  gamma_K = K 2^-24 (fp32
              accumulation over K terms: the layer's reduction length Cin k k, plus the bias):
                  y = W x + b           d_y = |W| d_x + gamma_K (|W| (|x| + d_x) + |b|)
                  x (1 + s)             |x| d_s + |1 + s| d_x + d_x d_s
                  activation, slope<=1  d unchanged; where the whole interval [v - d, v + d] is negative, d times the slope
                  an fp16 store         d <- d + eps (|v| + d) + 2^-25, taken at its sharper form  d + ulp(|v| + d) / 2:
                                        half a unit in the last place of the binade of |v| + d (<= eps (|v| + d)), 2^-25 below 2^-14
              Two sharpenings that stay rigorous: the error of the SFT shift head's hidden layer is carried as a linear term
              through the conv behind the SFT (|W_conv W_head| instead of |W_conv| |W_head|: Bounded.conv_lin), and a ReLU
              clears the bound where the whole interval is negative (Bounded.act).
    Rounded   the "rounding model": the same graph in float64 with the fp16 roundings applied where the kernels apply them.
              It is the yardstick of the precision condition  mean|device - v| <= 2 mean|model - v|  and, with a mutation
              switched on, the subject of tests/test_le_layer_ref_host.py.

The fp16 stores that are modelled, each next to the kernel line that performs it (csrc/ = hdr-realtime-video-pipeline_amd/csrc/):
  * every tensor written to HBM: `(f16)act_fast(acc * sc + sh, slope)` in the epilogues -- conv32s.hip:637, conv32p.hip:539,
    conv3x3s2_preg.hip:151, conv_tile_f16.hip:88, conv_igemm.hip:225, le_hg_misc.hip:160 (conv_c3), le_fused.hip:236 / :307
    (cond1, cond2), conv3x3s2_preg.hip:182 (CondNet3.4 in CondNet3.2's epilogue) and :222 (CondNet2.4 in CondNet234.0's);
  * the hidden layers of the 1x1 chains, kept in registers as packed f16: `lrelu_pack` (le_fused.hip:44-45, conv32s.hip:84-85,
    conv32p.hip:93-94, conv3x3s2_preg.hip:47-48) rounds the fp32 sum to f16 FIRST and then takes max(o, o * (f16)0.1f) in packed
    f16 -- so the negative side is rounded a second time and its slope is fp16(0.1) = 0.0999755859375, not 0.1 (`lrelu16`
    below; the deviation |fp16(0.1) - 0.1| |x| is part of the bound).  The generic epilogues take LeakyReLU in fp32 (`act`);
  * the SFT layer: hidden layer as above (conv32s.hip:401); (scale + 1) and shift rounded to f16 (conv32s.hip:313-314,
    `+ 1.f` in the fp32 accumulator init :282 -- api_pack.hip's pack_sft folds nothing: bias[32 + i] = b1s[i], :541); the
    modulated tile `y * s1p + s0p` in packed f16 written back to LDS (conv32s.hip:415, :430): one v_pk_fma_f16, one rounding;
  * relu(shuffle(conv)) rounded to f16 BEFORE the skip is added (conv32p.hip:539 then :574-575, conv32s.hip:637 then :651), every
    residual add in packed f16 with one rounding per add (conv32s.hip:649-651: x + conv2(..), then + the second residual);
  * conv_last: the conv result rounded to f16, the planar residual added in fp32, the sum rounded again (conv32s.hip:623-624).
The row-streaming kernels (le_rows.hip: one launch for the head, a ResBlock, the tail) keep the same intermediates as f16 in LDS
rings with "arithmetic, operand order and rounding points of the per-layer kernels" (le_rows.hip:30-32): a fused launch is the
longer primitive list of the launches it replaces.

Weights are the checkpoint's fp32 tensors rounded to f16 exactly as api_pack.hip rounds them (pack_conv :63, pack_sft :536-538,
pack_cond_trunk :609/:621/:631, pack_cond_tail :652/:654); biases stay fp32 -- with ONE fold: LE.conv_first's bias rides in the K
axis of its f16 fragments (pack_c3 / c3_welem, api_pack.hip:456, :478, :485) and is therefore rounded to f16 here too.
No kernel of this path flushes f16 subnormals: none sets a denormal mode in its code, and hipcc's default for gfx950 keeps them
(the kernel descriptors carry float_denorm_mode_16_64 = 3), so the absolute floor of every store stays at 2^-25.

STAGES, one entry per launch of the fp16 default path as `run_le` (csrc/api_graph.hip) issues it with every fusion switched off
(variants le_rows = 0, cond2_fused = 0, cond3_fused = 0, no_c3fuse = 1), profile key in brackets:

  trunk     [LE.cond_trunk]            agcm -> cond (cond_first.0/2/4)                             alone | one launch, two checks: the
  trunk1    [LE.cond_trunk]            cond -> cond1 (CondNet1.0/2/4)                              alone | 2nd half reads the stored bits
  x192      [LE.CondNet234.0]          cond -> x192 (CondNet2.0 | 3.0 | 4.0, 3x3 / 2)              alone; default form: composite with cond2
  cond2     [LE.CondNet2.2+4]          x192[0:64] -> cond2                                         alone; default form: inside x192's launch
  h2a       [LE.CondNet3.2]            x192[64:128] -> h2a                                         alone; default form: composite with cond3
  cond3     [LE.CondNet3.4]            h2a -> cond3                                                alone; default form: inside h2a's launch
  h2b       [LE.CondNet4.2]            x192[128:192] -> h2b                                        alone
  cond4     [LE.CondNet4.4]            h2b -> cond4                                                alone
  f0a       [le.conv_first]            agcm -> f0a                                                 alone; default form: inside fea0's launch
  fea0      [LE.HR_conv1]              (f0a, cond1) -> fea0 (SFT_layer1 + HR_conv1)                alone; default form: (agcm, cond1) -> fea0
  fea1a     [LE.down_conv1]            fea0 -> fea1a                                               alone; row form: one launch with f0a, fea0
  rt1a/rt1b [LE.recon_trunk1.0.conv1/2] fea1a -> l1b -> fea1                                       composite fea1a -> fea1 only: l1b is
                                                                                                   overwritten by recon_trunk5.0
  fea2a     [LE.down_conv2]            fea1 -> fea2a                                               alone
  rt2a/rt2b [LE.recon_trunk2.0.conv1/2] fea2a -> l2b -> fea2                                       composite only: l2b is overwritten by
                                                                                                   recon_trunk4.0
  fea3      [LE.down_conv3]            fea2 -> fea3                                                alone
  rt30a..rt32b [LE.recon_trunk3.0-3.2] fea3 -> .. -> t3x                                           NOT isolable: t3x / t3y alternate and
        l3b is shared, so of these six launches only the first input (fea3) and the last output (t3x) survive the frame.  They
        are checked as ONE composite fea3 -> t3x (the bound composes; after six SFT + conv pairs it is wide, so the input
        condition is not asked of this check) and otherwise only through the kernel they share with recon_trunk3.3
        (conv32s<1,sft>)
  rt33a     [LE.recon_trunk3.3.conv1]  t3x -> l3b                                                  alone
  rt33b     [LE.recon_trunk3.3.conv2]  (l3b, t3x, fea3) -> t3y  (second residual fea3)             alone
  up1       [LE.up_conv1.0]            (t3y, fea2) -> up1                                          alone
  rt4a/rt4b [LE.recon_trunk4.0.conv1/2] up1 -> l2b -> t4                                           each alone
  up2       [LE.up_conv2.0]            (t4, fea1) -> up2                                           alone
  rt5a/rt5b [LE.recon_trunk5.0.conv1/2] up2 -> l1b -> t5                                           each alone; row form: composite
  up3       [LE.up_conv3.0]            (t5, fea0) -> up3                                           alone; row form: inside the tail launch
  f0b       [LE.HR_conv2]              (up3, cond1) -> f0b (SFT_layer2 + HR_conv2)                 alone; row form: inside the tail launch
  out       [LE.conv_last]             (f0b, agcm) -> out  (planar residual agcm)                  alone; row form: (t5, fea0, cond1, agcm) -> out

`plan(profile)` turns the (layer, kernel) records of one profiled frame into the list of checks: it merges launches the build
fused (by the kernel tags) or whose intermediate does not survive, and fails on an LE launch that no check covers.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -11            # fp16 unit roundoff: half an ulp is at most EPS |x| ...
FLOOR = 2.0 ** -25          # ... and half the smallest subnormal below 2^-14 (_half_ulp)
U32 = 2.0 ** -24            # fp32 unit roundoff
S16 = float(np.float16(0.1))            # the slope lrelu_pack multiplies by


def f16(x):
    """float64 -> nearest f16 (numpy rounds float64 straight to half, ties to even) -> float64."""
    return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))


def _half_ulp(m):
    """Largest error of rounding a value of magnitude <= m to f16: half a unit in the last place of m's binade,
    2^(floor(log2 m) - 11) <= eps m, and 2^-25 in the subnormal range (|m| < 2^-14) -- never more than eps m + 2^-25."""
    e = torch.floor(torch.log2(torch.clamp(m, min=FLOOR / EPS)))
    return EPS * torch.pow(2.0, e)


def as_t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _conv(x, w, stride, pad_mode="zero"):
    k = w.shape[-1]
    p = k // 2
    x = x[None]
    if p:
        if pad_mode == "replicate_last_col":           # mutation: the column right of the image repeats the last one
            x = F.pad(x, (p, 0, p, p))
            x = torch.cat((x, x[..., -1:]), dim=-1)
        else:
            x = F.pad(x, (p, p, p, p))
    return F.conv2d(x, w, None, stride)[0]


def _ps2(x, swap=False):
    c, h, w = x.shape
    y = x.reshape(c // 4, 2, 2, h, w)
    if swap:                                            # mutation: sub-positions (0, 1) and (1, 0) exchanged
        y = y.transpose(1, 2)
    return y.permute(0, 3, 1, 4, 2).reshape(c // 4, 2 * h, 2 * w)


def _crop(x, hw, from_end=False):
    """HDRUNet3T1._align_to where the map is larger than its skip (2 ceil(n / 2) >= n: it is never smaller): centre crop,
    top = (xh - rh) // 2 = 0 for the one-pixel excess, i.e. the LAST row / column goes (conv32p.hip:404-405 `Y < p.Hd`)."""
    rh, rw = hw
    xh, xw = x.shape[-2:]
    assert xh - rh in (0, 1) and xw - rw in (0, 1), (x.shape, hw)
    if from_end:                                        # mutation: the first row / column goes instead
        return x[..., xh - rh:, xw - rw:]
    return x[..., :rh, :rw]


def _leaky(v, slope):
    return torch.where(v >= 0, v, v * slope)


class Bounded:
    """Values are (v, d), behind the SFT shift head (v, d, (A, e)): see conv_lin."""

    def inp(self, a):
        return (a, torch.zeros_like(a))

    def val(self, x):
        return x[0]

    def conv(self, x, w, b, stride=1, extra_terms=0):
        v, d = x[0], x[1]
        K = w.shape[1] * w.shape[2] * w.shape[3] + 1 + extra_terms
        g = K * U32
        y = _conv(v, w, stride) + b[:, None, None]
        dy = _conv(d + g * (v.abs() + self._total(x)), w.abs(), stride) + g * b.abs()[:, None, None]
        if len(x) == 3:             # the linear error term A e passes through W as (W A) e: |W A| <= |W| |A|
            A, eb = x[2]
            dy = dy + _conv(eb, torch.einsum("ockl,cj->ojkl", w, A).abs(), stride)
        return (y, dy)

    def conv_lin(self, x, w, b):
        """A 1x1 conv whose input error is NOT folded into d but kept as the linear term (A, e) = (W, d_x): the error of the SFT shift
        head's hidden layer reaches the 3x3 conv behind the SFT through W_conv W_head, and |W_conv W_head| e is a (several times)
        sharper bound than |W_conv| |W_head| e."""
        v, d = x
        g = (w.shape[1] + 1) * U32
        y = _conv(v, w, 1) + b[:, None, None]
        dy = _conv(g * (v.abs() + d), w.abs(), 1) + g * b.abs()[:, None, None]
        return (y, dy, (w[:, :, 0, 0], d))

    @staticmethod
    def _total(x):
        """d plus the linear term's worst case."""
        if len(x) == 2:
            return x[1]
        A, eb = x[2]
        return x[1] + torch.einsum("cj,jhw->chw", A.abs(), eb)

    def plus1(self, x):
        return (x[0] + 1.0, x[1])

    def act(self, x, slope):
        # the device's value lies in [v - d, v + d] and the activation is monotone with slope <= 1: d does not grow, and where the
        # whole interval is negative it shrinks by the slope (ReLU: to 0 -- both sides are exactly 0 there)
        v, d = x
        y = _leaky(v, slope)
        return (y, torch.maximum(_leaky(v + d, slope) - y, y - _leaky(v - d, slope)))

    def store(self, x):
        v, d = x[0], x[1]
        return (v, d + _half_ulp(v.abs() + self._total(x))) + tuple(x[2:])

    def lrelu16(self, x):
        v, d = self.act(self.store(x), 0.1)
        pv, pd = x
        # negative side: rnd16(o * fp16(0.1)) against 0.1 o with |o| <= |v| + d -- the slope's deviation and one more rounding,
        # wherever the device's value can be negative
        m = pv.abs() + pd + _half_ulp(pv.abs() + pd)
        extra = abs(S16 - 0.1) * m + _half_ulp(S16 * m)
        return (v, d + torch.where((pv - pd) < 0, extra, torch.zeros_like(extra)))

    def fma16(self, x, s1, s0):
        (xv, xd), (sv, sd), (tv, td) = x, s1, s0[:2]
        # one rounding: `y * s1p + s0p` is a v_pk_fma_f16 (hipcc contracts it under its default -ffp-contract; the ISA of conv32s.hip
        # and le_rows.hip holds one v_pk_fma_f16 per modulated f16 pair and no v_pk_mul_f16 besides lrelu_pack's)
        return self.store((xv * sv + tv, xv.abs() * sd + sv.abs() * xd + xd * sd + td) + tuple(s0[2:]))

    def add16(self, a, b):
        v, d = a[0] + b[0], a[1] + b[1]
        return self.store((v, d + U32 * (v.abs() + d)))

    def ps(self, x):
        return (_ps2(x[0]), _ps2(x[1]))

    def crop(self, x, hw):
        return (_crop(x[0], hw), _crop(x[1], hw))

    def chans(self, x, a, b):
        return (x[0][a:b], x[1][a:b])


class Rounded:
    """The rounding model; `mut` switches ONE deliberate mistake on (tests/test_le_layer_ref_host.py)."""
    MUTATIONS = ("zero_tap", "zero_weight", "replicate_last_col", "crop_from_end", "ps_swap", "slope02", "no_plus1", "res_twice", "acc16")

    def __init__(self, mut=None, exact=False, chunk=32):
        assert mut is None or mut in self.MUTATIONS, mut
        self.mut = mut
        self.chunk = chunk              # of "acc16"
        self.exact = exact              # no rounding at all: the plain float64 network (the stage table against the oracle)

    def _r(self, v):
        return v if self.exact else f16(v)

    def inp(self, a):
        return a

    def val(self, x):
        return x

    def conv(self, x, w, b, stride=1, extra_terms=0):
        k = w.shape[-1]
        if self.mut == "zero_tap" and k == 3:
            w = w.clone()
            w[:, :, 0, 2] = 0.0
        if self.mut == "zero_weight" and k == 3:
            w = w.clone()
            i = int(w.abs().argmax())
            w.view(-1)[i] = 0.0
        if self.mut == "acc16" and k == 3 and w.shape[1] == 32:
            # the accumulator rounded to f16 after every `chunk` terms (K order: tap, then channels)
            acc = torch.zeros(1, dtype=torch.float64)
            for ky in range(3):
                for kx in range(3):
                    for c0 in range(0, 32, self.chunk):
                        w1 = torch.zeros_like(w)
                        w1[:, c0:c0 + self.chunk, ky, kx] = w[:, c0:c0 + self.chunk, ky, kx]
                        acc = f16(acc + _conv(x, w1, stride))
            return acc + b[:, None, None]
        mode = "replicate_last_col" if (self.mut == "replicate_last_col" and k == 3) else "zero"
        return _conv(x, w, stride, mode) + b[:, None, None]

    def conv_lin(self, x, w, b):
        return self.conv(x, w, b)

    def plus1(self, x):
        return x if self.mut == "no_plus1" else x + 1.0

    def act(self, x, slope):
        if self.mut == "slope02" and slope == 0.1:
            slope = 0.2
        return _leaky(x, slope)

    def store(self, x):
        return self._r(x)

    def lrelu16(self, x):
        if self.exact:
            return _leaky(x, 0.1)
        o = f16(x)
        return torch.maximum(o, f16(o * (2 * S16 if self.mut == "slope02" else S16)))

    def fma16(self, x, s1, s0):
        return self._r(x * s1 + s0)

    def add16(self, a, b):
        if self.mut == "res_twice":
            return self._r(self._r(a + b) + b)
        return self._r(a + b)

    def ps(self, x):
        return _ps2(x, self.mut == "ps_swap")

    def crop(self, x, hw):
        return _crop(x, hw, self.mut == "crop_from_end")

    def chans(self, x, a, b):
        return x[a:b]



# ------------------------------------------------------------------------------------------------- weights
def pack(sd, rounded=True):
    """The LE tensors of a state dict as float64: weights rounded to f16 as api_pack.hip rounds them (pack_conv :63, pack_sft
    :536-538, pack_cond_trunk :609-631, pack_cond_tail :652-654), biases fp32; LE.conv_first's bias is an f16 K-slot of its
    fragments (pack_c3 :478, c3_welem :456).  rounded = False: the checkpoint as it is (the oracle's network)."""
    P = {}
    for k, v in sd.items():
        if not k.startswith("LE."):
            continue
        a = np.asarray(v, np.float32)
        if rounded and (k.endswith(".weight") or k == "LE.conv_first.bias"):
            a = a.astype(np.float16)
        P[k] = as_t(a)
    for part in ("weight", "bias"):
        P[f"LE.CondNet234.0.{part}"] = torch.cat([P[f"LE.CondNet{i}.0.{part}"] for i in (2, 3, 4)])     # pack_conv's '+' list, :15-32
    return P


# -------------------------------------------------------------------------------------------- graph pieces
def _c(o, P, name, x, stride=1, extra_terms=0):
    return o.conv(x, P[name + ".weight"], P[name + ".bias"], stride, extra_terms)


def _sft(o, P, name, x, cond):
    """SFTLayer.forward: x (scale + 1) + shift, scale / shift = conv1(leaky(conv0(cond)))."""
    hs = o.lrelu16(_c(o, P, name + ".SFT_scale_conv0", cond))                       # conv32s.hip:400-401
    ht = o.lrelu16(_c(o, P, name + ".SFT_shift_conv0", cond))
    s1 = o.store(o.plus1(_c(o, P, name + ".SFT_scale_conv1", hs, extra_terms=1)))   # + 1.f in the accumulator init :282, f16 :313
    s0 = o.store(o.conv_lin(ht, P[name + ".SFT_shift_conv1.weight"], P[name + ".SFT_shift_conv1.bias"]))     # :314
    return o.fma16(x, s1, s0)                                                       # :415, back to LDS :430


def _conv_act(o, P, name, x, slope, stride=1):
    y = _c(o, P, name, x, stride)
    return o.store(y if slope is None else o.act(y, slope))


def s_trunk(o, P, e):
    x = e["agcm"]
    for n in ("LE.cond_first.0", "LE.cond_first.2", "LE.cond_first.4"):
        x = o.lrelu16(_c(o, P, n, x))                                               # le_fused.hip:162-163, :186-187
    e["cond"] = x                                                                   # the packed f16 fragments are what is stored, :203-214


def s_trunk1(o, P, e):
    """The second half of the trunk launch.  Its operand is bit for bit the tensor the first half stores (le_fused.hip:193: `bf = nf`,
    :203-214 store those very fragments), so it is held to the float64 reference on the device's own `cond`."""
    x = e["cond"]
    for n in ("LE.CondNet1.0", "LE.CondNet1.2"):
        x = o.lrelu16(_c(o, P, n, x))
    e["cond1"] = o.store(_c(o, P, "LE.CondNet1.4", x))                              # le_fused.hip:236


def s_x192(o, P, e):
    y = _conv_act(o, P, "LE.CondNet234.0", e["cond"], 0.1, 2)                       # conv3x3s2_preg.hip:151
    e["x192a"], e["x192b"], e["x192c"] = o.chans(y, 0, 64), o.chans(y, 64, 128), o.chans(y, 128, 192)


def s_cond2(o, P, e):
    h = o.lrelu16(_c(o, P, "LE.CondNet2.2", e["x192a"]))                            # le_fused.hip:293 / conv3x3s2_preg.hip:211
    e["cond2"] = o.store(_c(o, P, "LE.CondNet2.4", h))                              # le_fused.hip:307 / conv3x3s2_preg.hip:222


def _mk_conv(dst, name, src, slope, stride=1):
    def fn(o, P, e):
        e[dst] = _conv_act(o, P, name, e[src], slope, stride)
    return fn


def s_fea0(o, P, e):
    e["fea0"] = _conv_act(o, P, "LE.HR_conv1", _sft(o, P, "LE.SFT_layer1", e["f0a"], e["cond1"]), 0.0)


def _mk_rb(base, x, cond, mid, out, extra=None):
    def fa(o, P, e):
        e[mid] = _conv_act(o, P, base + ".conv1", _sft(o, P, base + ".sft1", e[x], e[cond]), 0.0)

    def fb(o, P, e):
        y = _conv_act(o, P, base + ".conv2", _sft(o, P, base + ".sft2", e[mid], e[cond]), None)    # conv32s.hip:637
        y = o.add16(y, e[x])                                                                        # :651, first add
        if extra:
            y = o.add16(y, e[extra])                                                                # :651, second add ("+ fea3")
        e[out] = y
    return fa, fb


def _mk_up(name, src, skip, dst):
    def fn(o, P, e):
        u = o.store(o.act(o.ps(_c(o, P, name, e[src])), 0.0))                       # conv32p.hip:539 (per sub-position pass)
        skipv = e[skip]
        u = o.crop(u, tuple(o.val(skipv).shape[-2:]))                               # :404-405
        e[dst] = o.add16(u, skipv)                                                  # :574-575
    return fn


def s_f0b(o, P, e):
    e["f0b"] = _conv_act(o, P, "LE.HR_conv2", _sft(o, P, "LE.SFT_layer2", e["up3"], e["cond1"]), 0.0)


def s_out(o, P, e):
    e["out"] = o.add16(o.store(_c(o, P, "LE.conv_last", e["f0b"])), e["agcm"])      # conv32s.hip:623-624


class Stage:
    def __init__(self, name, key, ins, outs, fn):
        self.name, self.key, self.ins, self.outs, self.fn = name, key, tuple(ins), tuple(outs), fn


def _stages():
    S = [
        Stage("trunk", "LE.cond_trunk", ["agcm"], ["cond"], s_trunk),
        Stage("trunk1", "LE.cond_trunk", ["cond"], ["cond1"], s_trunk1),
        Stage("x192", "LE.CondNet234.0", ["cond"], ["x192a", "x192b", "x192c"], s_x192),
        Stage("cond2", "LE.CondNet2.2+4", ["x192a"], ["cond2"], s_cond2),
        Stage("h2a", "LE.CondNet3.2", ["x192b"], ["h2a"], _mk_conv("h2a", "LE.CondNet3.2", "x192b", 0.1, 2)),
        Stage("cond3", "LE.CondNet3.4", ["h2a"], ["cond3"], _mk_conv("cond3", "LE.CondNet3.4", "h2a", None)),
        Stage("h2b", "LE.CondNet4.2", ["x192c"], ["h2b"], _mk_conv("h2b", "LE.CondNet4.2", "x192c", 0.1, 2)),
        Stage("cond4", "LE.CondNet4.4", ["h2b"], ["cond4"], _mk_conv("cond4", "LE.CondNet4.4", "h2b", None, 2)),
        Stage("f0a", "le.conv_first", ["agcm"], ["f0a"], _mk_conv("f0a", "LE.conv_first", "agcm", 0.0)),
        Stage("fea0", "LE.HR_conv1", ["f0a", "cond1"], ["fea0"], s_fea0),
        Stage("fea1a", "LE.down_conv1", ["fea0"], ["fea1a"], _mk_conv("fea1a", "LE.down_conv1", "fea0", 0.0, 2)),
    ]

    def rb(tag, base, x, cond, mid, out, extra=None):
        fa, fb = _mk_rb(base, x, cond, mid, out, extra)
        S.append(Stage(tag + "a", base + ".conv1", [x, cond], [mid], fa))
        S.append(Stage(tag + "b", base + ".conv2", [mid, x, cond] + ([extra] if extra else []), [out], fb))

    rb("rt1", "LE.recon_trunk1.0", "fea1a", "cond2", "rt1.mid", "fea1")
    S.append(Stage("fea2a", "LE.down_conv2", ["fea1"], ["fea2a"], _mk_conv("fea2a", "LE.down_conv2", "fea1", 0.0, 2)))
    rb("rt2", "LE.recon_trunk2.0", "fea2a", "cond3", "rt2.mid", "fea2")
    S.append(Stage("fea3", "LE.down_conv3", ["fea2"], ["fea3"], _mk_conv("fea3", "LE.down_conv3", "fea2", 0.0, 2)))
    rb("rt30", "LE.recon_trunk3.0", "fea3", "cond4", "rt30.mid", "rt30.out")
    rb("rt31", "LE.recon_trunk3.1", "rt30.out", "cond4", "rt31.mid", "rt31.out")
    rb("rt32", "LE.recon_trunk3.2", "rt31.out", "cond4", "rt32.mid", "t3x")
    rb("rt33", "LE.recon_trunk3.3", "t3x", "cond4", "l3b", "t3y", "fea3")
    S.append(Stage("up1", "LE.up_conv1.0", ["t3y", "fea2"], ["up1"], _mk_up("LE.up_conv1.0", "t3y", "fea2", "up1")))
    rb("rt4", "LE.recon_trunk4.0", "up1", "cond3", "l2b", "t4")
    S.append(Stage("up2", "LE.up_conv2.0", ["t4", "fea1"], ["up2"], _mk_up("LE.up_conv2.0", "t4", "fea1", "up2")))
    rb("rt5", "LE.recon_trunk5.0", "up2", "cond2", "l1b", "t5")
    S.append(Stage("up3", "LE.up_conv3.0", ["t5", "fea0"], ["up3"], _mk_up("LE.up_conv3.0", "t5", "fea0", "up3")))
    S.append(Stage("f0b", "LE.HR_conv2", ["up3", "cond1"], ["f0b"], s_f0b))
    S.append(Stage("out", "LE.conv_last", ["f0b", "agcm"], ["out"], s_out))
    return S


STAGES = _stages()
BY_NAME = {s.name: s for s in STAGES}

# logical tensor -> (workspace tap, channel range or None).  "agcm" and "out" are hdrtv_infer's own output tensors, not taps.
# A logical tensor that is absent here does not survive the frame (its buffer holds a later launch's data when the frame ends).
TAPS = {
    "cond": ("le.cond", None), "cond1": ("le.cond1", None), "x192a": ("le.x192", (0, 64)), "x192b": ("le.x192", (64, 128)),
    "x192c": ("le.x192", (128, 192)), "cond2": ("le.cond2", None), "h2a": ("le.h2a", None), "cond3": ("le.cond3", None),
    "h2b": ("le.h2b", None), "cond4": ("le.cond4", None), "f0a": ("le.f0a", None), "fea0": ("le.fea0", None),
    "fea1a": ("le.fea1a", None), "fea1": ("le.fea1", None), "fea2a": ("le.fea2a", None), "fea2": ("le.fea2", None),
    "fea3": ("le.fea3", None), "t3x": ("le.t3x", None), "l3b": ("le.l3b", None), "t3y": ("le.t3y", None), "up1": ("le.up1", None),
    "l2b": ("le.l2b", None), "t4": ("le.t4", None), "up2": ("le.up2", None), "l1b": ("le.l1b", None), "t5": ("le.t5", None),
    "up3": ("le.up3", None), "f0b": ("le.f0b", None),
}


class Check:
    """One comparison: the launches `stages` evaluated as one primitive list on the taps `ins`, compared at `outs`."""

    def __init__(self, stages, drop=(), by_name=None, taps=None):
        by_name, taps = by_name or BY_NAME, taps or TAPS        # another network's stage table (tests/hg_layer_ref.py)
        self.stages = [by_name[s] for s in stages]
        made = [t for s in self.stages for t in s.outs]
        self.ins = tuple(dict.fromkeys(t for s in self.stages for t in s.ins if t not in made))
        self.outs = tuple(t for t in made if (t in taps or t == "out") and t not in drop)
        self.name = "+".join(stages) if len(stages) <= 3 else f"{stages[0]}..{stages[-1]}"
        self.composite = len(stages) > 1
        # recon_trunk3.0 - 3.2 as one six-launch composite: an extra beyond the launches that can be isolated.  Its bound has gone
        # through six SFT + conv pairs and is wide; the hard and the precision assertions apply, the input condition is not asked of it
        self.extra = len(stages) > 3

    def run(self, o, P, taps):
        e = {t: o.inp(taps[t]) for t in self.ins}
        for s in self.stages:
            s.fn(o, P, e)
        return {t: e[t] for t in self.outs}


def plan(profile):
    """(layer, kernel) records of one profiled frame -> [Check].  Launches the build fused (kernel tags) or whose intermediate is
    overwritten later in the frame become one composite check; an LE launch no check claims is an error."""
    recs = [(l, k) for l, k, *_ in profile if l.startswith(("LE.", "le."))]
    tag = {}
    for l, k in recs:
        tag.setdefault(l, k)

    def has(layer, part=""):
        return layer in tag and part in tag[layer]

    checks, claimed = [], set()

    def add(stages, keys, drop=()):
        checks.append(Check(stages, drop))
        claimed.update(keys)

    add(["trunk"], ["LE.cond_trunk"])
    add(["trunk1"], ["LE.cond_trunk"])
    if has("LE.CondNet234.0", "+tail"):                  # CondNet2.2 + .4 in the epilogue: channels 0..63 never reach HBM
        add(["x192", "cond2"], ["LE.CondNet234.0"], drop=("x192a",))
    else:
        add(["x192"], ["LE.CondNet234.0"])
        add(["cond2"], ["LE.CondNet2.2+4"])
    if has("LE.CondNet3.2", "+tail"):                    # CondNet3.4 in the epilogue: h2a is not stored
        add(["h2a", "cond3"], ["LE.CondNet3.2"], drop=("h2a",))
    else:
        add(["h2a"], ["LE.CondNet3.2"])
        add(["cond3"], ["LE.CondNet3.4"])
    add(["h2b"], ["LE.CondNet4.2"])
    add(["cond4"], ["LE.CondNet4.4"])
    if has("LE.head"):                                   # le_head_rows: conv_first .. down_conv1
        add(["f0a", "fea0", "fea1a"], ["LE.head"], drop=("f0a",))
    else:
        if has("LE.HR_conv1", "c3+"):                    # conv_first inside HR_conv1's kernel
            add(["f0a", "fea0"], ["LE.HR_conv1"], drop=("f0a",))
        else:
            add(["f0a"], ["le.conv_first"])
            add(["fea0"], ["LE.HR_conv1"])
        add(["fea1a"], ["LE.down_conv1"])

    def block(tagname, base, mid_survives):
        if has(base):                                    # le_rb_rows: the block in one launch
            add([tagname + "a", tagname + "b"], [base], drop=(BY_NAME[tagname + "a"].outs[0],))
        elif mid_survives:
            add([tagname + "a"], [base + ".conv1"])
            add([tagname + "b"], [base + ".conv2"])
        else:
            add([tagname + "a", tagname + "b"], [base + ".conv1", base + ".conv2"])

    block("rt1", "LE.recon_trunk1.0", False)
    add(["fea2a"], ["LE.down_conv2"])
    block("rt2", "LE.recon_trunk2.0", False)
    add(["fea3"], ["LE.down_conv3"])
    keys3 = []
    for b in range(3):
        base = f"LE.recon_trunk3.{b}"
        keys3 += [base] if has(base) else [base + ".conv1", base + ".conv2"]
    add(["rt30a", "rt30b", "rt31a", "rt31b", "rt32a", "rt32b"], keys3)
    block("rt33", "LE.recon_trunk3.3", True)
    add(["up1"], ["LE.up_conv1.0"])
    block("rt4", "LE.recon_trunk4.0", True)
    add(["up2"], ["LE.up_conv2.0"])
    block("rt5", "LE.recon_trunk5.0", True)
    if has("LE.tail"):                                   # le_tail_rows: up_conv3 .. conv_last
        add(["up3", "f0b", "out"], ["LE.tail"], drop=("up3", "f0b"))
    else:
        add(["up3"], ["LE.up_conv3.0"])
        add(["f0b"], ["LE.HR_conv2"])
        add(["out"], ["LE.conv_last"])
    ran = {l for l, _ in recs}
    assert ran == claimed, ("LE launches without a check / checks without a launch", sorted(ran ^ claimed))
    return checks


def per_layer_profile():
    """The records of the per-layer form (every fusion off), for planning without a device."""
    return [(s.key, "") for s in STAGES]


def fused_profile(head=True, blocks=("LE.recon_trunk1.0", "LE.recon_trunk2.0", "LE.recon_trunk3.0", "LE.recon_trunk3.1", "LE.recon_trunk3.2",
                                     "LE.recon_trunk4.0", "LE.recon_trunk5.0"), tail=True):
    """The records of the default form with the given row kernels on (CondNet tails and conv_first always fused)."""
    out = []
    for s in STAGES:
        base = s.key.rsplit(".", 1)[0]
        if s.key in ("LE.CondNet2.2+4", "LE.CondNet3.4", "le.conv_first"):
            continue
        if head and s.key in ("LE.HR_conv1", "LE.down_conv1"):
            rec = ("LE.head", "le_head_rows")
        elif tail and s.key in ("LE.up_conv3.0", "LE.HR_conv2", "LE.conv_last"):
            rec = ("LE.tail", "le_tail_rows")
        elif base in blocks and s.key.endswith((".conv1", ".conv2")):
            rec = (base, "le_rb_rows")
        else:
            rec = (s.key, {"LE.CondNet234.0": "conv3x3s2_preg<192>+tail", "LE.CondNet3.2": "conv3x3s2_preg<64>+tail",
                           "LE.HR_conv1": "conv32s<1,c3+sft>"}.get(s.key, ""))
        if rec not in out:
            out.append(rec)
    return out


def full_graph(P, agcm, o=None):
    """Every stage in order on one input: {logical tensor: value}.  With the default o (no rounding) and pack(.., False) this is the
    oracle's network in float64."""
    o = o or Rounded(exact=True)
    e = {"agcm": o.inp(agcm)}
    for s in STAGES:
        s.fn(o, P, e)
    return {k: o.val(v) for k, v in e.items()}


def taps_from_graph(env):
    """A float64 environment rounded to f16: inputs of the kind the device hands out (exact f16 values)."""
    return {k: f16(v) for k, v in env.items()}


def evaluate(check, P, taps, model=None):
    """One check on `taps` -> {out: dict(v, d, model)}."""
    ref = check.run(Bounded(), P, taps)
    mod = check.run(model or Rounded(), P, taps)
    return {t: {"v": ref[t][0], "d": ref[t][1], "model": mod[t]} for t in check.outs}


def metrics(r, got):
    """Figures of one output: `got` (device or a mutated model) against v / d / the rounding model."""
    err = (got - r["v"]).abs()
    vp = r.get("v_prec", r["v"])        # tests/hg_layer_ref.py: the precision condition's own reference, where it differs from v
    perr, merr = (got - vp).abs(), (r["model"] - vp).abs()
    # d = 0 (an output the launch must reproduce exactly; no LE bound is ever 0): ratio 0 where it does, inf where it does not
    ratio = torch.where(r["d"] > 0, err / r["d"].clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return {
        "n": got.numel(),
        "max_ratio": float(ratio.max()),
        "violations": int((err > r["d"]).sum()),
        "mean_err": float(perr.mean()),
        "mean_model": float(merr.mean()),
        "bit_equal": float((got == r["model"]).double().mean()),
        "significant": float((r["v"].abs() > 8 * r["d"]).double().mean()),
    }


def input_condition(r):
    """The condition on the INPUTS of a comparison (not a measurement of the device): enough of the output must stand clear of the
    bound, |v| > 8 d, for the comparison not to be satisfied by the bound alone -> (ok, share of all elements, share of the
    elements the reference does not clamp to zero).  Asked: 25 % of all output elements.  An element the float64 reference
    clamps to exactly 0 (ReLU) can never count, under any bound, and the ReLU behind HR_conv1 or a ResBlock's conv1 leaves
    only 21 .. 25 % of the elements positive on the test frames: where fewer than 25 % / 0.8 of the elements are nonzero, 80 %
    of the nonzero ones must stand clear instead."""
    v, d = r["v"], r["d"]
    sig = v.abs() > 8 * d
    nz = v != 0
    share = float(sig.double().mean())
    share_nz = float(sig[nz].double().mean()) if bool(nz.any()) else 0.0
    ok = share >= 0.25 or (float(nz.double().mean()) < 0.25 / 0.8 and share_nz >= 0.8)
    return ok, share, share_nz


def split(checks, numel_of, parts):
    """The checks in `parts` groups of about equal float64 work (elements read and written x launches), order kept inside a group."""
    cost = [sum(numel_of(t) for t in c.ins + c.outs) * len(c.stages) for c in checks]
    load, groups = [0.0] * parts, [[] for _ in range(parts)]
    for i in sorted(range(len(checks)), key=lambda i: -cost[i]):
        g = load.index(min(load))
        load[g] += cost[i]
        groups[g].append(i)
    return [[checks[i] for i in sorted(g)] for g in groups]


# The frames of tests/test_gpu_le_layers.py: (H, W) -> seeds of the `noise` and the `gradient` frame (weights.synthetic_frame).
#   (270, 486)  half / quarter / eighth maps 135x243, 68x122, 34x61: odd maps, both one-pixel _align_to crops, 9 strips
#   (64, 122)   a 61-wide half map (last strip one column), quarter map 16x31
#   (46, 182)   maps 23x91, 12x46, 6x23
#   (61, 103)   odd full size: no row kernel
#   (8, 68), (68, 8)   the smallest frames hdrtv_reserve accepts
FRAMES = {(270, 486): (47, 147), (64, 122): (52, 152), (46, 182): (54, 154), (61, 103): (56, 156), (8, 68): (58, 158), (68, 8): (60, 160)}
SHORT = ((270, 486), (64, 122), (46, 182))          # of tests/test_gpu_le_rows.py's SHORT: also run with le_rows_min = 1
