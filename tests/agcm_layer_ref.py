"""Float64 reference of ONE launch of the AGCM front end's fp16 path, with an a-priori error bound.  TEST INFRASTRUCTURE ONLY.

CPU only (torch / numpy, nothing of the device), in the shape of tests/le_layer_ref.py, whose helpers it reuses (`f16`, `_half_ulp`,
`metrics`, `input_condition`, and its `Bounded.act` / `Bounded.store`).  Every launch is evaluated on the DEVICE'S OWN
input bits (exact f32 / f16 values read back from the workspace), so the error of the launches in front does not enter:

    Bounded   every output as a pair (v, d): v in float64 with no intermediate rounding, written as the NETWORK has it (conv, then
              pool, then activation -- not the kernel's commuted form), d an elementwise bound on |device - v| DERIVED from the
              kernel's arithmetic with  u = 2^-24 (fp32 unit roundoff),  gamma_K = K u / (1 - K u)  (K roundings on one term:
              a sum of K terms in any order, with or without fused multiply-adds),  fp16 half-ulp at the MLP's three stores:
                  cls_block   window sum of <= 9 terms (gamma_8); the norm's affine  a s + (beta - mean a) cnt,  a = rstd gamma
                              (gamma_3 on a s and on beta cnt, gamma_5 on mean a cnt); Ci products + the bias * cnt term + the
                              division by 9 (gamma_{Ci+2}; gamma_3 on the bias); the negative side of the LeakyReLU two more
                              (0.2f is not 0.2, and the product rounds)
                  cls_stats   PX-wide shuffle tree per workgroup (gamma_PX on the sum, gamma_{PX+1} on the squares, each rounded
                              once more as v * v), the fp64 combine ((nblk + 8) 2^-53), the casts to f32.  rstd = (var + eps)^-1/2:
                              the error e of E[x^2] - m^2 (+ |f32(1e-5) - 1e-5|: the kernel's eps is the f32 constant) is
                              amplified by  1 / (2 lo^{3/2}),  lo = max(var + eps - e, f32(1e-5))  -- the kernel clamps var at 0,
                              so its argument never falls below eps.  Carried explicitly: maps of two pixels exist
                  agcm_fold   fea6: 128 + 1 terms (gamma_129); each head 6 + 1 (gamma_7) on top of fea6's own bound; 1 + s, the
                              product with W (or b, then + t): one rounding each; a fragment element is then stored as f16
                  agcm_mlp    MFMA sums of K = 16 / 64 / 64 products and the bias in the fp32 accumulator (gamma_{K+1}); f16
                              stores at relu_pack (twice) and at the output
              No measured number enters d.
    Rounded   the "rounding model": the same launch with roundings where the kernel rounds -- plain float32 torch / numpy
              arithmetic in the kernel's (commuted) form and order for the classifier, the statistics and the fold, with a fused
              multiply-add (one rounding) where hipcc's default contraction compiles one (the v_fmac_f32 / v_fma_f32 of `acc += w *
              s`, `a * s + ..`, `nbeta - nmean * a`, `acc + bias * cnt`, `b * (1 + s) + t`; `W * (1 + s)` and `v * v` stay
              products), float64 with f16 stores for the MLP.  It is the yardstick of the precision condition  mean|device - v| <= 2 mean|model - v|  (which is plain
              equality wherever the model reproduces v exactly: an empty fragment slot, the mean of a one-pixel map), and, with a
              mutation switched on, the subject of tests/test_agcm_layer_ref_host.py.

STAGES (csrc/ = hdr-realtime-video-pipeline_amd/csrc/; one entry per launch `run_agcm`, api_graph.hip:291-354, issues), profile
key in brackets, and the kernel line behind each rounding:

  cls1        [cls_block]  cond (f16) -> u1.   agcm.hip:58-73 window sum in fp32 (`s += xv`, f16 -> f32 exact), :89 the Ci products,
                           :90 `(acc + bias[co] * s_cnt[px]) / 9.f`, :91 `v * 0.2f`, :92 stored as f32
  cls2..cls5  [cls_block]  (u_{i-1}, mean_{i-1}, rstd_{i-1}) -> u_i.   As cls1, and :75-76 `a = nrstd * ngamma; s = a * s + (nbeta -
                           nmean * a) * cnt`: InstanceNorm of the previous block applied to the window sum.  gamma / beta are
                           AGCM.classifier.model.{3,7,11,15}, the conv model.{0,4,8,12,16} (api_pack.hip:685-701)
  stats1..5   [cls_stats]  u_i -> (mean_i, rstd_i).   agcm.hip:95-102 per-workgroup (sum, sum of squares) in fp32 through a
                           PX-wide __shfl_xor tree, :134-141 combined in fp64, :143-147 m = s1 / n, var = s2 / n - m m clamped at
                           0, both cast to f32.  agcm.part is overwritten by every block, so for blocks 1-4 the statement is "the
                           statistics of the device's own u_i"; block 5's partials survive the frame and are checked themselves
                           (`part5`, [128, nblk, 2]) against float64 sums of u5, read with the launcher's nblk (agcm.hip:363-366:
                           PX = 4 up to 4096 output pixels, else 16)
  fold        [agcm_fold]  mean5 -> biasbuf[0:166], frags.   agcm.hip:169-172 fea6 = b20 + W20 mean5 (sequential), :180-185 the six
                           Linear heads, :193-195 b' = b (1 + s) + t, :205/:209/:212 `W * (1.f + sc)`, :214 `(f16)v`.  Fragment
                           layout (agcm.hip:158, :198-213): f16x8 per lane, tiles [0..1] layer 1, [2..9] layer 2 (mt * 4 + s),
                           [10..13] layer 3 (s); lane l holds row tile * 32 + (l & 31), slots p = 8 (l >> 5) + j of one 16-wide
                           k-step; k = p for layer 1, 16 s + acc_kperm16(p) for layers 2 and 3 (common.h:109, restated below).
                           Slots the layout leaves empty (k >= 3 in layer 1, rows >= 3 in layer 3) and biasbuf[131:160] are v = 0
                           with d = 0: exactly zero.  v of a fragment element is W (1 + s) unrounded, the f16 store is part of d
  mlp         [agcm_mlp]   (rgb f16, decoded device frags, device biasbuf) -> agcm_out.   agcm.hip:329-331 layer 1 (bias_tile in
                           the accumulator, one K = 16 MFMA), :283-284 relu_pack: `(f16)a[..]` FIRST, then the packed max with 0,
                           :334-339 layer 2 (4 x K = 16), :340 relu_pack, :342-344 layer 3, :346-348 `(f16)o[i]`: rounded once.
                           Weights are the decoded fragments -- all 16 k slots of layer 1, all 32 rows' worth of bias

Nothing in this path rounds weights except `frags`; all others are the checkpoint's fp32 tensors (api_pack.hip:685-719).

`plan(profile)` turns the (layer, kernel) records of one profiled frame into the list of checks and fails on an AGCM launch
(`cls_block`, `cls_stats`, `agcm_fold`, `agcm_mlp`, or anything else named cls* / agcm*) that no check claims: a classifier in fewer
launches does not run unchecked.  The W8A8 forms (`cls_block<fq>`, `agcm_fold<q8>`, `agcm_mlp<q8>`) are NOT covered here: a
profile that names them is rejected by name.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import le_layer_ref as L
from le_layer_ref import U32, _half_ulp, as_t, f16, input_condition, metrics  # noqa: F401  (re-exported for the tests)

U64 = 2.0 ** -53
SLOPE = 0.2
IN_EPS = 1e-5
IN_EPS_F32 = float(np.float32(1e-5))            # cls_stats_launch's `1e-5f` (api_graph.hip:320)
CLS_CI, CLS_CO, CLS_IDX = (3, 16, 32, 64, 128), (16, 32, 64, 128, 128), (0, 4, 8, 12, 16)
NFRAG = 14
LB = L.Bounded()


def g32(k):
    """gamma_k in fp32."""
    return k * U32 / (1.0 - k * U32)


# ----------------------------------------------------------------------------------------- the launchers' rules
def half_up(n):
    return (n - 1) // 2 + 1                     # api_workspace.hip:8


def maps_for(H, W):
    """shapes_for (api_workspace.hip:57-63): [(ch[i], cw[i])], i = 0 the condition map, i = 1..5 the block outputs."""
    m = [(max(H // 4, 1), max(W // 4, 1))]
    for _ in range(5):
        m.append((half_up(m[-1][0]), half_up(m[-1][1])))
    return m


def admits(H, W):
    """do_reserve's AGCM conditions (api_workspace.hip:84, :92)."""
    m = maps_for(H, W)
    return H >= 8 and W >= 8 and m[4][0] * m[4][1] >= 2


def px_of(npix):
    """cls_block_launch (agcm.hip:364-370): output pixels per workgroup."""
    return 4 if npix <= 4096 else 16


def nblk_of(npix):
    px = px_of(npix)
    return (npix + px - 1) // px


def mlp_grid(npix):
    """agcm_mlp_launch (agcm.hip:403-405) -> (groups of 32 pixels, waves in the grid, grid-stride trips of the busiest wave)."""
    ngrp = (npix + 31) // 32
    nwave = 4 * min((ngrp + 3) // 4, 2048)
    return ngrp, nwave, (ngrp + nwave - 1) // nwave


def acc_kperm16(p):
    """common.h:109: B-operand slot p of a 16-wide k-step -> accumulator row of the tile it was packed from."""
    return ((p >> 3) << 2) | (((p >> 2) & 1) << 3) | (p & 3)


def frag_layout(l2_natural=False, l3_shift=False):
    """(layer, row, k, used) int arrays of shape [14, 64, 8]: what agcm_fold_kernel writes at frags[(f * 64 + lane) * 8 + j].
    Every slot addresses an element of its layer's padded matrix (layer 1: [64, 16], 2: [64, 64], 3: [32, 64]); `used` is False
    where the kernel writes zero."""
    lay, row, col, used = (np.zeros((NFRAG, 64, 8), np.int64) for _ in range(4))
    for f in range(NFRAG):
        for lane in range(64):
            for j in range(8):
                r, p = lane & 31, 8 * (lane >> 5) + j
                if f < 2:
                    v = (0, f * 32 + r, p, p < 3)
                elif f < 10:
                    mt, s = (f - 2) >> 2, (f - 2) & 3
                    v = (1, mt * 32 + r, 16 * s + (p if l2_natural else acc_kperm16(p)), True)
                else:
                    k = 16 * (f - 10) + acc_kperm16(p)
                    v = (2, r, k, r < 3)
                lay[f, lane, j], row[f, lane, j], col[f, lane, j], used[f, lane, j] = v
    if l3_shift:                    # mutation: layer-3 rows shifted by one -- tile row r holds W3[r - 1]
        used[10:] = (row[10:] >= 1) & (row[10:] < 4)
    return lay, row, col, used.astype(bool)


_LAYOUT = frag_layout()


def scatter_frags(mats, layout=None, shift=False):
    """Logical matrices (W1' [64, 3], W2' [64, 64], W3' [3, 64]) -> the device's [14, 64, 8]."""
    lay, row, col, used = layout or _LAYOUT
    out = torch.zeros((NFRAG, 64, 8), dtype=torch.float64)
    for i, m in enumerate(mats):
        sel = torch.from_numpy((lay == i) & used)
        r = torch.from_numpy(row)[sel] - (1 if (shift and i == 2) else 0)
        out[sel] = m[r, torch.from_numpy(col)[sel]]
    return out


def decode_frags(fr):
    """The device's [14, 64, 8] -> the padded operand matrices A1 [64, 16], A2 [64, 64], A3 [32, 64], EVERY slot included."""
    lay, row, col, _ = _LAYOUT
    out = [torch.zeros(s, dtype=torch.float64) for s in ((64, 16), (64, 64), (32, 64))]
    for i in range(3):
        sel = torch.from_numpy(lay == i)
        out[i][torch.from_numpy(row)[sel], torch.from_numpy(col)[sel]] = fr[sel]
    return out


# ------------------------------------------------------------------------------------------------- weights
def pack(sd):
    """The AGCM tensors of a state dict as float64 (the checkpoint's fp32 values, api_pack.hip:685-719; 1x1 convs as matrices)."""
    P = {}
    for k, v in sd.items():
        if k.startswith("AGCM."):
            a = as_t(np.asarray(v, np.float32))
            P[k] = a.reshape(a.shape[0], -1) if a.dim() == 4 else a
    return P


def _cls_w(P, i):
    p = f"AGCM.classifier.model.{CLS_IDX[i]}"
    return P[p + ".weight"], P[p + ".bias"]


def _cls_norm(P, i):
    """gamma, beta of the InstanceNorm behind block i (0-based)."""
    p = f"AGCM.classifier.model.{CLS_IDX[i] + 3}"
    return P[p + ".weight"], P[p + ".bias"]


_HEADS = ("first", "HR", "last")
_CONVS = ("conv_first", "HRconv", "conv_last")


# ----------------------------------------------------------------------------------------------- primitives
def _win(x, clamp=False):
    """Sum over the in-image taps of the 3x3 / stride 2 / pad 1 window, in x's dtype and in the kernel's order (ky outer, kx
    inner; the skipped taps are added as exact zeros).  clamp (mutation): row Hi / column Wi taken by clamping."""
    C, H, W = x.shape
    Ho, Wo = half_up(H), half_up(W)
    pb, pr = 2 * Ho - H, 2 * Wo - W                 # 1 on an odd map: the window of the last output reaches row Hi / column Wi
    xp = F.pad(x, (1, pr, 1, pb))
    if clamp:
        if pb:
            xp[:, -1, :] = xp[:, -2, :]
        if pr:
            xp[:, :, -1] = xp[:, :, -2]
    s = torch.zeros((C, Ho, Wo), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            s = s + xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    return s


def _fma32(a, b, c):
    """A fused multiply-add of float32 tensors: the product of two f32 values is exact in float64, so this is one rounding (but for
    the rare double rounding of the float64 sum)."""
    return (a.double() * b.double() + c.double()).float()


def _groups(u, px, fill_last=False):
    """[C, h, w] -> [C, nblk, px]: the pixels of each workgroup, idle lanes 0 (fill_last: the last pixel again)."""
    C = u.shape[0]
    flat = u.reshape(C, -1)
    n = flat.shape[1]
    nblk = (n + px - 1) // px
    pad = nblk * px - n
    if pad:
        tail = flat[:, -1:].expand(C, pad) if fill_last else torch.zeros((C, pad), dtype=u.dtype)
        flat = torch.cat((flat, tail), 1)
    return flat.reshape(C, nblk, px)


def _tree(t):
    """What lane 0 holds after `s += __shfl_xor(s, o)`, o = 1, 2, 4, ..: the pairwise tree over the last axis."""
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


class Bounded:
    """Stage-sized primitives -> {output: (v, d)}; inputs are plain float64 tensors (the device's bits)."""

    def cls(self, x, norm, w, b):
        Ci = w.shape[1]
        cnt = _win(torch.ones((1,) + tuple(x.shape[1:]), dtype=torch.float64))
        S, A = _win(x), _win(x.abs())
        e = g32(8) * A
        if norm is None:
            xn, sp = x, S
        else:
            mean, rstd, gamma, beta = (t[:, None, None] for t in norm)
            a = rstd * gamma
            xn = (x - mean) * a + beta                                           # InstanceNorm with the device's own statistics
            sp = a * S + (beta - mean * a) * cnt
            e = (1 + g32(3)) * a.abs() * e + g32(3) * a.abs() * S.abs() + cnt * (g32(3) * beta.abs() + g32(5) * (mean * a).abs())
        # the network's order: 1x1 conv, AvgPool2d(3, 2, 1, count_include_pad), LeakyReLU
        y = torch.einsum("oc,chw->ohw", w, xn) + b[:, None, None]
        z = F.avg_pool2d(y[None], 3, 2, 1, count_include_pad=True)[0]
        gK = g32(Ci + 2)
        dz = (torch.einsum("oc,chw->ohw", w.abs(), (1 + gK) * e + gK * sp.abs()) + g32(3) * b.abs()[:, None, None] * cnt) / 9.0
        v, d = LB.act((z, dz), SLOPE)
        d = d + torch.where(z - dz < 0, g32(2) * SLOPE * (z.abs() + dz), torch.zeros_like(dz))
        return v, d

    def stats(self, u, with_part=False):
        C = u.shape[0]
        n = u.shape[1] * u.shape[2]
        px, nblk = px_of(n), nblk_of(n)
        flat = u.reshape(C, -1)
        m, ma, q = flat.mean(1), flat.abs().mean(1), (flat * flat).mean(1)
        var = ((flat - m[:, None]) ** 2).mean(1)
        c64 = (nblk + 8) * U64
        em = (g32(px) + c64) * ma                                                # of the fp64 m the variance uses
        d_mean = em + U32 * (m.abs() + em) + 2.0 ** -150
        e = (g32(px + 1) + c64) * q + 2 * m.abs() * em + em * em + 4 * U64 * (q + m * m) + abs(IN_EPS_F32 - IN_EPS)
        x = var + IN_EPS
        lo = torch.clamp(x - e, min=IN_EPS_F32)
        rstd = x ** -0.5
        dr = e / (2 * lo ** 1.5)
        d_rstd = dr + (U32 + 4 * U64) * (rstd + dr)
        out = {"mean": (m, d_mean), "rstd": (rstd, d_rstd)}
        if with_part:
            g = _groups(u, px)
            v = torch.stack((g.sum(2), (g * g).sum(2)), 2)
            d = torch.stack((g32(px) * g.abs().sum(2), g32(px + 1) * (g * g).sum(2)), 2)
            out["part"] = (v, d)
        return out

    def fold(self, P, mean5):
        w20, b20 = P["AGCM.classifier.model.20.weight"], P["AGCM.classifier.model.20.bias"]
        fea = w20 @ mean5 + b20
        d_fea = g32(129) * (w20.abs() @ mean5.abs() + b20.abs())
        bias_v, bias_d = torch.zeros(160, dtype=torch.float64), torch.zeros(160, dtype=torch.float64)
        mats_v, mats_d = [], []
        for st, (head, conv) in enumerate(zip(_HEADS, _CONVS)):
            hv = {}
            for kind in ("scale", "shift"):
                hw, hb = P[f"AGCM.cond_{kind}_{head}.weight"], P[f"AGCM.cond_{kind}_{head}.bias"]
                hv[kind] = (hw @ fea + hb, (1 + g32(7)) * (hw.abs() @ d_fea) + g32(7) * (hw.abs() @ fea.abs() + hb.abs()))
            (s, ds), (t, dt) = hv["scale"], hv["shift"]
            w, b = P[f"AGCM.{conv}.weight"], P[f"AGCM.{conv}.bias"]
            g = 1 + s
            eg = ds + U32 * (g.abs() + ds)
            n = b.shape[0]
            bias_v[64 * st:64 * st + n] = b * g + t
            bias_d[64 * st:64 * st + n] = b.abs() * eg + dt + g32(2) * (b.abs() * (g.abs() + eg) + t.abs() + dt)
            wv = w * g[:, None]
            ep = w.abs() * eg[:, None] + U32 * w.abs() * (g.abs() + eg)[:, None]
            mats_v.append(wv)
            mats_d.append(ep + _half_ulp(wv.abs() + ep))
        return {"fea6": (fea, d_fea), "bias": (bias_v, bias_d), "frags": (scatter_frags(mats_v), scatter_frags(mats_d))}

    def mlp(self, rgb, frags, bias, chunk=1 << 16):
        A1, A2, A3 = decode_frags(frags)
        C, H, W = rgb.shape
        x = rgb.reshape(3, -1)
        vs, ds = [], []

        def lin(xv, xd, w, b):
            g = g32(w.shape[1] + 1)
            return w @ xv + b[:, None], w.abs() @ (xd + g * (xv.abs() + xd)) + g * b.abs()[:, None]

        for i in range(0, x.shape[1], chunk):
            xv = torch.zeros((16, min(chunk, x.shape[1] - i)), dtype=torch.float64)
            xv[:3] = x[:, i:i + chunk]
            h = LB.act(LB.store(lin(xv, torch.zeros_like(xv), A1, bias[0:64])), 0.0)
            g = LB.act(LB.store(lin(h[0], h[1], A2, bias[64:128])), 0.0)
            o = LB.store(lin(g[0], g[1], A3, bias[128:160]))
            vs.append(o[0][:3])
            ds.append(o[1][:3])
        return torch.cat(vs, 1).reshape(3, H, W), torch.cat(ds, 1).reshape(3, H, W)


class Rounded:
    """The rounding model; `mut` switches ONE deliberate mistake on (tests/test_agcm_layer_ref_host.py)."""
    MUTATIONS = {
        # cls_block
        "pool_div_cnt": "the pool divides by the number of in-image taps instead of 9",
        "bias_x9": "the bias counted 9 times at the border instead of cnt times",
        "window_clamp": "the window takes row Hi / column Wi by clamping instead of skipping it (odd maps)",
        "slope01": "LeakyReLU slope 0.1 for 0.2",
        "wrong_gamma": "gamma / beta of another block's InstanceNorm",
        "idle_lanes": "idle lanes (p >= npix) recompute the last pixel and add it to s1 / s2",
        # cls_stats
        "drop_last_wg": "the last workgroup's partials left out of a channel's statistics",
        "no_eps": "eps missing from rstd",
        "unbiased": "unbiased variance (n - 1)",
        # agcm_fold
        "l2_natural_k": "layer-2 fragments in natural K order (no acc_kperm16)",
        "l3_row_shift": "layer-3 rows shifted by one",
        # agcm_mlp
        "no_relu3": "the ReLU in front of layer 3 missing",
        "bias_after_store": "a bias added after the f16 store instead of in the fp32 accumulator",
        "tail_not_written": "the last, partial group of 32 pixels not written",
        "pixel0_leak": "a lane that was masked when its colour was fetched (it read pixel 0) keeps that colour: the pixels of the "
                       "last, partial group take pixel 0's.  (The other reading -- pixel 0's colour in the B operand of the lanes "
                       "that hold k = 8 .. 15 -- changes no output as long as layer 1's slots k >= 3 are zero, which the fold check "
                       "holds to exactly 0.)",
    }

    def __init__(self, mut=None):
        assert mut is None or mut in self.MUTATIONS, mut
        self.mut = mut

    def cls(self, x, norm, w, b, wrong_norm=None):
        f = torch.float32
        x, w, b = x.to(f), w.to(f), b.to(f)
        clamp = self.mut == "window_clamp"
        s = _win(x, clamp)
        cnt = _win(torch.ones((1,) + tuple(x.shape[1:]), dtype=f), clamp)
        if norm is not None:
            mean, rstd, gamma, beta = (t.to(f)[:, None, None] for t in norm)
            if self.mut == "wrong_gamma":
                gamma, beta = (t.to(f)[:, None, None] for t in wrong_norm)
            a = rstd * gamma
            s = _fma32(a, s, _fma32(-a, mean, beta) * cnt)                       # s = a * s + (beta - mean * a) * cnt, as compiled
        acc = torch.zeros((w.shape[0],) + tuple(s.shape[1:]), dtype=f)
        for ci in range(w.shape[1]):                                             # `acc += w[ci] * s_sum[ci][px]`: one v_fmac_f32 each
            acc = _fma32(w[:, ci, None, None], s[ci][None], acc)
        nine = torch.full_like(cnt, 9.0)
        v = _fma32(b[:, None, None], nine if self.mut == "bias_x9" else cnt, acc) / (cnt if self.mut == "pool_div_cnt" else nine)
        v = torch.where(v >= 0, v, v * torch.tensor(0.1 if self.mut == "slope01" else SLOPE, dtype=f))
        return v.double()

    def stats(self, u, with_part=False):
        C = u.shape[0]
        n = u.shape[1] * u.shape[2]
        px = px_of(n)
        g = _groups(u.float(), px, fill_last=self.mut == "idle_lanes")
        part = torch.stack((_tree(g), _tree(g * g)), 2)                          # [C, nblk, 2] f32
        p64 = part.double()
        if self.mut == "drop_last_wg" and p64.shape[1] > 1:
            p64 = p64[:, :-1]
        s1, s2 = p64[..., 0].sum(1), p64[..., 1].sum(1)
        m = s1 / n
        var = torch.clamp(s2 / n - m * m, min=0.0)
        if self.mut == "unbiased" and n > 1:
            var = var * n / (n - 1)
        rstd = 1.0 / torch.sqrt(var + (0.0 if self.mut == "no_eps" else IN_EPS_F32))
        out = {"mean": m.float().double(), "rstd": rstd.float().double()}
        if with_part:
            out["part"] = part.double()
        return out

    def fold(self, P, mean5):
        f = np.float32
        n32 = lambda t: t.numpy().astype(f)
        # the compiled kernel fuses `a += w * x` and `b * g + t` (v_fmac_f32): one rounding, the f32 product being exact in float64
        fma = lambda a, b, c: (np.float64(a) * np.float64(b) + np.float64(c)).astype(f)
        m = n32(mean5)
        w20 = n32(P["AGCM.classifier.model.20.weight"])
        fea = n32(P["AGCM.classifier.model.20.bias"]).copy()
        for k in range(128):
            fea = fma(w20[:, k], m[k], fea)
        bias = np.zeros(160, f)
        mats = []
        for st, (head, conv) in enumerate(zip(_HEADS, _CONVS)):
            hv = []
            for kind in ("scale", "shift"):
                hw, a = n32(P[f"AGCM.cond_{kind}_{head}.weight"]), n32(P[f"AGCM.cond_{kind}_{head}.bias"]).copy()
                for k in range(6):
                    a = fma(hw[:, k], fea[k], a)
                hv.append(a)
            s, t = hv
            w, b = n32(P[f"AGCM.{conv}.weight"]), n32(P[f"AGCM.{conv}.bias"])
            g = f(1.0) + s
            bias[64 * st:64 * st + len(b)] = fma(b, g, t)
            mats.append(as_t((w * g[:, None]).astype(np.float16)))
        layout = frag_layout(self.mut == "l2_natural_k", self.mut == "l3_row_shift")
        return {"fea6": as_t(fea), "bias": as_t(bias), "frags": scatter_frags(mats, layout, shift=self.mut == "l3_row_shift")}

    def mlp(self, rgb, frags, bias, chunk=1 << 16):
        A1, A2, A3 = decode_frags(frags)
        C, H, W = rgb.shape
        x = rgb.reshape(3, -1).clone()
        n = x.shape[1]
        tail = (n // 32) * 32
        if self.mut == "pixel0_leak" and tail < n:
            x[:, tail:] = x[:, 0:1]
        late = self.mut == "bias_after_store"

        def lin(xv, w, b):
            if late:
                return f16(f16(w @ xv) + b[:, None])
            return f16(w @ xv + b[:, None])

        outs = []
        for i in range(0, n, chunk):
            xv = torch.zeros((16, min(chunk, n - i)), dtype=torch.float64)
            xv[:3] = x[:, i:i + chunk]
            h = torch.clamp(lin(xv, A1, bias[0:64]), min=0.0)
            g = lin(h, A2, bias[64:128])
            if self.mut != "no_relu3":
                g = torch.clamp(g, min=0.0)
            outs.append(lin(g, A3, bias[128:160])[:3])
        out = torch.cat(outs, 1)
        if self.mut == "tail_not_written" and tail < n:
            out[:, tail:] = 0.0
        return out.reshape(3, H, W)


# ---------------------------------------------------------------------------------------------------- stages
def _wrong_norm(P, i):
    """For the mutation: the norm parameters cls{i+1} must NOT read -- those of the following block (the preceding one's,
    repeated, for the last), cut to the channel count."""
    ci = CLS_CI[i]
    g, b = _cls_norm(P, i if i < 4 else i - 2)
    rep = (ci + g.shape[0] - 1) // g.shape[0]
    return g.repeat(rep)[:ci], b.repeat(rep)[:ci]


def _mk_cls(i):
    def fn(o, P, e):
        w, b = _cls_w(P, i)
        if i == 0:
            x, norm = e["cond"], None
        else:
            x, norm = e[f"u{i}"], (e[f"mean{i}"], e[f"rstd{i}"]) + _cls_norm(P, i - 1)
        if isinstance(o, Rounded):
            return {f"u{i + 1}": o.cls(x, norm, w, b, _wrong_norm(P, i) if i else None)}
        return {f"u{i + 1}": o.cls(x, norm, w, b)}
    return fn


def _mk_stats(i):
    def fn(o, P, e):
        r = o.stats(e[f"u{i}"], with_part=i == 5)
        out = {f"mean{i}": r["mean"], f"rstd{i}": r["rstd"]}
        if i == 5:
            out["part5"] = r["part"]
        return out
    return fn


def s_fold(o, P, e):
    return o.fold(P, e["mean5"])


def s_mlp(o, P, e):
    return {"out": o.mlp(e["rgb"], e["frags"], e["bias"])}


class Stage:
    def __init__(self, name, key, ins, outs, fn):
        self.name, self.key, self.ins, self.outs, self.fn = name, key, tuple(ins), tuple(outs), fn


def _stages():
    S = []
    for i in range(5):
        ins = ["cond"] if i == 0 else [f"u{i}", f"mean{i}", f"rstd{i}"]
        S.append(Stage(f"cls{i + 1}", "cls_block", ins, [f"u{i + 1}"], _mk_cls(i)))
        outs = [f"mean{i + 1}", f"rstd{i + 1}"] + (["part5"] if i == 4 else [])
        S.append(Stage(f"stats{i + 1}", "cls_stats", [f"u{i + 1}"], outs, _mk_stats(i + 1)))
    S.append(Stage("fold", "agcm_fold", ["mean5"], ["fea6", "bias", "frags"], s_fold))
    S.append(Stage("mlp", "agcm_mlp", ["rgb", "frags", "bias"], ["out"], s_mlp))
    return S


STAGES = _stages()
BY_NAME = {s.name: s for s in STAGES}


class Check:
    """One launch, evaluated on the taps `ins`, compared at `outs`; `launch` is its index among the frame's AGCM launches."""

    def __init__(self, stage, launch=None):
        self.stage = BY_NAME[stage]
        self.name, self.ins, self.outs, self.launch = stage, self.stage.ins, self.stage.outs, launch

    def run(self, o, P, taps):
        return self.stage.fn(o, P, {t: taps[t] for t in self.ins})


def _is_agcm(layer, kernel):
    return any(s.startswith(("cls", "agcm")) for s in (layer, kernel))


def plan(profile):
    """(layer, kernel) records of one profiled frame -> [Check], one per AGCM launch, in launch order.  Fails on a W8A8 kernel
    (by name: not covered here), on an AGCM launch that no check claims, and on a check without its launch."""
    recs = [(l, k) for l, k, *_ in profile if _is_agcm(l, k)]
    for l, k in recs:
        assert "<fq>" not in k and "<q8>" not in k, f"{k}: the W8A8 forms of the AGCM launches are not covered by agcm_layer_ref"
    checks, claimed = [], set()
    for want in STAGES:
        for i, (l, k) in enumerate(recs):
            if i not in claimed and l == want.key and k == want.key:
                # launch order is the data flow: a stage's launch comes after every launch already claimed
                assert not claimed or i > max(claimed), ("AGCM launches out of order", want.name, recs)
                claimed.add(i)
                checks.append(Check(want.name, i))
                break
        else:
            raise AssertionError(("no launch for the check", want.name, want.key, recs))
    unclaimed = [recs[i] for i in range(len(recs)) if i not in claimed]
    assert not unclaimed, ("AGCM launches without a check", unclaimed)
    return checks


def default_profile():
    """The records `run_agcm` leaves on the fp16 path, for planning without a device."""
    return [(s.key, s.key) for s in STAGES]


def evaluate(check, P, taps, model=None):
    """One check on `taps` -> {out: dict(v, d, model)}."""
    ref = check.run(Bounded(), P, taps)
    mod = check.run(model or Rounded(), P, taps)
    return {t: {"v": ref[t][0], "d": ref[t][1], "model": mod[t]} for t in check.outs}


def full_graph(P, rgb, cond, o=None):
    """Every stage in order on one input -> {logical tensor: value}.  o = None: Bounded's v alone, the network in float64 with
    no rounding at all; o = Rounded(): taps of the kind the device hands out."""
    e = {"rgb": rgb, "cond": cond}
    for s in STAGES:
        r = s.fn(o or Bounded(), P, {t: e[t] for t in s.ins})
        e.update({k: (v if o is not None else v[0]) for k, v in r.items()})
    return e


# The frames of tests/test_gpu_agcm_layers.py: (H, W) -> seeds of the `noise` and the `gradient` frame (weights.synthetic_frame),
# and PX of cls_block's five launches there (asserted against px_of / maps_for, not trusted).
#   (8, 68)       the smallest frame the classifier admits (ch[4] * cw[4] >= 2 needs a quarter-size side of 17): maps 1x9 .. 1x2, 1x1
#   (36, 72)      the smallest with two-dimensional maps: 5x9, 3x5, 2x3, 1x2, 1x1 -- statistics over two elements and over one
#   (61, 103)     cond 15x25, maps 8x13, 4x7, 2x4, 1x2: clipped windows right and bottom, npix % 4 != 0; 6283 pixels = 196 groups + 11
#   (69, 133)     cond 17x33, maps 9x17, 5x9, 3x5, 2x3: EVERY block reads a map that is odd in a dimension (61x103's 2x4 is not)
#   (270, 486)    block 1 is 34x61 = 2074 outputs: 519 partials per channel, more than one trip per thread in cls_stats
#   (520, 1016)   cond 130x254, block 1 65x127 = 8255 > 4096: <true,16>, 8255 % 16 = 15; 528320 pixels = 16510 groups on 8192
#                 waves: three grid-stride trips with the prefetch, the last one ragged
#   (1036, 1076)  block 1 130x135 = 17550 (% 16 = 14), block 2 65x68 = 4420 > 4096 (% 16 = 4): <false,16> with InstanceNorm on
#                 load, ragged; block 3 33x34 = 1122: back to PX = 4; 1114736 pixels: a partial last group of 16
FRAMES = {(8, 68): (71, 171), (36, 72): (72, 172), (61, 103): (73, 173), (69, 133): (74, 174), (270, 486): (75, 175),
          (520, 1016): (76, 176), (1036, 1076): (77, 177)}
FORMS = {(8, 68): (4, 4, 4, 4, 4), (36, 72): (4, 4, 4, 4, 4), (61, 103): (4, 4, 4, 4, 4), (69, 133): (4, 4, 4, 4, 4),
         (270, 486): (4, 4, 4, 4, 4), (520, 1016): (16, 4, 4, 4, 4), (1036, 1076): (16, 16, 4, 4, 4)}
HG_FRAME = (61, 103)            # the one size also run with the HG head's workspace around run_agcm
