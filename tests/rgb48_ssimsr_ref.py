"""The enlarging rule of hdrtv_post_rgb48_ssimsr (include/hdrtv_mi355x.h), restated in plain Python / numpy: a spline36 upscale of
the u16 codes (stage A, the integer rule of tests/rgb48_scale_ref.py with another kernel and no anti-ringing) and, with ssim, the
arithmetic of the reference's SSimSuperRes display shader on top of it (stage B, float32 operation by operation, with the
conventions of tests/rgb48_fsr_ref.py and rgb48_down_ref.py: NumPy rounds every elementwise multiply, add, subtract, divide and
square root on its own and fuses nothing, denormals are kept).

    stab(n, m)                         -> (start [m], q [m][6]): the spline36 taps of an axis, n source -> m destination samples
    spline36(codes, dH, dW)            -> u16 [dH][dW][3]: stage A, the codes P
    lowtab(n, m) / fintab(n, m)        -> the per-axis tables of stage B (n low, m high extent), see below
    lowres(pcodes, H, W)               -> float32 [H][W][4]: Lr.rgb and Lr.a, the two low-resolution passes over the P samples
    var(codes, lr)                     -> (vL, vH) float32 [H][W]
    final(codes, pcodes, lr, vl, vh)   -> u16 [dH][dW][3]
    scale(codes, dH, dW, ssim=False)

Sizes: equal sizes return the codes; otherwise H < dH <= 2 H and W < dW <= 2 W (both axes enlarged, as the reference's
_is_upscale_required asks; the shader's partial chains are out of scope).  Indices outside a frame read the clamped pixel.

Stage A.  c = (d + 0.5) n / m - 0.5, i0 = floor(c), t = c - i0, six taps k = -2 .. 3 with weight S(t - k) in double,
    S(x), x = |x|:  x < 1: ((13/11 x - 453/209) x - 3/209) x + 1;  x < 2, y = x - 1: ((-6/11 y + 270/209) y - 156/209) y;
                    x < 3, y = x - 2: ((1/11 y - 45/209) y + 26/209) y;  else 0
summed in tap order, q_k = floor(w_k / sum * 16384 + 0.5), the remainder to the largest q_k (the lowest k on a tie); horizontal
pass, vertical pass, (sum + 2^27) >> 28, clamp.  mpv is not part of the reference tree: parity with its spline36 is UNPINNED.

Stage B, a pure function of the source codes c and the spline36 codes P; the orders the shader leaves open fixed here:
    Sq(v)       (0.2126 (r r) + 0.7152 (g g)) + 0.0722 (b b), every square one rounded multiply
    samples     s = float32(c) / float32(65535), Ps = float32(P) / float32(65535)
    footprint   rgb48_down_ref.footprint(m, n, j) of low index j: taps k_lo .. k_hi (at most 9), x_k in low-resolution pixels;
                weight mn(|x_k|), B = 0.334, C = 0.333:  x < 1: ((2 - 1.5 B - C) x + (-3 + 2 B + C)) x x + (1 - B / 3), else
                (((-B / 6 - C) x + (B + 5 C)) x + (-2 B - 8 C)) x + (4 / 3 B + 4 C); summed in tap order, divided by the sum in
                double, rounded to float32 (the shader's division by W folded into the table)
    pass I      vertical, to [H][dW]: acc = acc + wy_k * v, k ascending from 0, for A.rgb (v = Ps) and A.q (v = Sq(Ps));
                e1 = max(|A.q - Sq(A.rgb)|, 5e-7)
    pass II     horizontal on A.rgb, to [H][W]: Lr.rgb, q2 = sum wx_k Sq(A.rgb), e2 = max(|q2 - Sq(Lr.rgb)|, 5e-7);
                u = (i + 0.5) dW / W - 0.5, b0 = floor(u), f = float32(u - b0);  e1i = ((1 - f) e1[b0]) + (f e1[b0 + 1]);  Lr.a = e2 + e1i
    var         neighbours (x-1, y), (x+1, y), (x, y-1), (x, y+1):  m = ((((v0 + 0.25 v1) + 0.25 v2) + 0.25 v3) + 0.25 v4) / 2,
                var = max(((((Sq(v0 - m) + 0.25 Sq(v1 - m)) + ...) + 0.25 Sq(v4 - m)) / 2, 1e-6): vL on s, vH on Lr.rgb
    final       p = (d + 0.5) n / m - 0.5, ip = floor(p + 0.5) (ties up), off = p - ip, kern[t] = float32(cos(pi (t - off) / 3)),
                t = -1, 0, 1.  c0 = Ps;  mV = (sum (wX wY) Lr.a[ip_y + Y][ip_x + X]) / 4, X outer, Y inner, w = 1 / 0.5;  per tap g:
                R = -1.5 sqrt(vL / (vH + mV));  wt = (kx[X] ky[Y]) / (Sq(c0 - Lr.rgb) + Lr.a);
                term = (s + Lr.rgb R) + ((-1 - R) c0);  D += wt term;  Ws += wt;  pix = sat(c0 + D / Ws);  code = (int)(pix 65535 + 0.5)
A texture unit's filter weights, the 16-bit float intermediates mpv keeps and what a GLSL compiler makes of the shader are UNPINNED.
"""
import functools
import math

import numpy as np

import rgb48_down_ref as D

F = np.float32
ONE = 16384
TAPS = 6
MAX_RATIO = 2
MAX_LOW_TAPS = 9
MN_B, MN_C = 0.334, 0.333
LUMA_R, LUMA_G, LUMA_B = F(0.2126), F(0.7152), F(0.0722)
E_FLOOR = F(5e-7)
V_FLOOR = F(1e-6)


def spline36_w(x):
    x = abs(x)
    if x < 1.0:
        return ((13.0 / 11.0 * x - 453.0 / 209.0) * x - 3.0 / 209.0) * x + 1.0
    if x < 2.0:
        y = x - 1.0
        return ((-6.0 / 11.0 * y + 270.0 / 209.0) * y - 156.0 / 209.0) * y
    if x < 3.0:
        y = x - 2.0
        return ((1.0 / 11.0 * y - 45.0 / 209.0) * y + 26.0 / 209.0) * y
    return 0.0


def mn_w(x):
    x = abs(x)
    b, c = MN_B, MN_C
    if x < 1.0:
        return ((2.0 - 1.5 * b - c) * x + (-3.0 + 2.0 * b + c)) * x * x + (1.0 - b / 3.0)
    return (((-b / 6.0 - c) * x + (b + 5.0 * c)) * x + (-2.0 * b - 8.0 * c)) * x + (4.0 / 3.0 * b + 4.0 * c)


def check_size(h, w, dh, dw):
    if (dh, dw) == (h, w) and h >= 1 and w >= 1:
        return
    if not (1 <= h < dh <= MAX_RATIO * h and 1 <= w < dw <= MAX_RATIO * w):
        raise ValueError(f"both axes enlarged, by at most {MAX_RATIO}x: {w}x{h} -> {dw}x{dh}")


@functools.lru_cache(maxsize=None)
def stab(n, m):
    start = np.zeros(m, dtype=np.int64)
    q = np.zeros((m, TAPS), dtype=np.int64)
    for d in range(m):
        c = (d + 0.5) * n / m - 0.5
        i0 = math.floor(c)
        t = c - i0
        w = [spline36_w(t - k) for k in range(-2, 4)]
        s = 0.0
        for v in w:
            s += v
        qk = [int(math.floor(v / s * ONE + 0.5)) for v in w]
        big = 0
        for k in range(TAPS):
            if qk[k] > qk[big]:          # the lowest k on a tie
                big = k
        qk[big] += ONE - sum(qk)
        start[d] = i0 - 2
        q[d] = qk
    start.setflags(write=False)
    q.setflags(write=False)
    return start, q


def spline36(codes, dH, dW):
    src = np.asarray(codes)
    assert src.dtype == np.uint16 and src.ndim == 3
    H, W = src.shape[:2]
    s = src.astype(np.int64)
    start, q = stab(W, dW)
    hor = np.zeros((H, dW, src.shape[2]), dtype=np.int64)
    for k in range(TAPS):
        hor += s[:, np.clip(start + k, 0, W - 1)] * q[:, k].reshape(1, dW, 1)
    start, q = stab(H, dH)
    acc = np.zeros((dH, dW, src.shape[2]), dtype=np.int64)
    for k in range(TAPS):
        acc += hor[np.clip(start + k, 0, H - 1)] * q[:, k].reshape(dH, 1, 1)
    return np.clip((acc + (1 << 27)) >> 28, 0, 65535).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def lowtab(n, m):
    """Per low index j of an axis with n low and m high samples: lo [n] (first high tap, unclamped), cnt [n], w [n][nt] float32
    (zero-padded), b0 [n] and f [n] float32 (the linear fetch of pass II), x [n] lists of the tap positions."""
    rows = []
    for j in range(n):
        lo, hi, _, xs = D.footprint(m, n, j)
        v = [mn_w(x) for x in xs]
        s = 0.0
        for t in v:
            s += t
        u = (j + 0.5) * m / n - 0.5
        b0 = math.floor(u)
        rows.append((lo, hi - lo + 1, [t / s for t in v], b0, u - b0, xs))
    nt = max(r[1] for r in rows)
    w = np.zeros((n, nt), dtype=F)
    for j, r in enumerate(rows):
        w[j, :r[1]] = np.array(r[2], dtype=np.float64).astype(F)
    lo = np.array([r[0] for r in rows], dtype=np.int64)
    cnt = np.array([r[1] for r in rows], dtype=np.int64)
    b0 = np.array([r[3] for r in rows], dtype=np.int64)
    f = np.array([r[4] for r in rows], dtype=np.float64).astype(F)
    for a in (lo, cnt, w, b0, f):
        a.setflags(write=False)
    return {"lo": lo, "cnt": cnt, "w": w, "b0": b0, "f": f, "x": [r[5] for r in rows]}


@functools.lru_cache(maxsize=None)
def fintab(n, m):
    """Per high index d: ip [m] (the nearest low pixel, ties up), off [m] double, kern [m][3] float32 (the Hann window at -1, 0, 1)."""
    ip = np.zeros(m, dtype=np.int64)
    off = np.zeros(m, dtype=np.float64)
    kern = np.zeros((m, 3), dtype=F)
    for d in range(m):
        p = (d + 0.5) * n / m - 0.5
        ip[d] = math.floor(p + 0.5)
        off[d] = p - ip[d]
        kern[d] = [F(math.cos(math.pi * (t - off[d]) / 3.0)) for t in (-1, 0, 1)]
    for a in (ip, off, kern):
        a.setflags(write=False)
    return {"ip": ip, "off": off, "kern": kern}


def samples(codes):
    return np.asarray(codes).astype(F) / F(65535)


def sq(v):
    """The shader's Luma: squares first."""
    return (LUMA_R * (v[..., 0] * v[..., 0]) + LUMA_G * (v[..., 1] * v[..., 1])) + LUMA_B * (v[..., 2] * v[..., 2])


def lowres(pcodes, H, W):
    ps = samples(pcodes)
    dH, dW = ps.shape[:2]
    ty, tx = lowtab(H, dH), lowtab(W, dW)
    psq = sq(ps)
    a = np.zeros((H, dW, 3), F)
    aq = np.zeros((H, dW), F)
    for k in range(ty["w"].shape[1]):
        rows = np.clip(ty["lo"] + k, 0, dH - 1)
        a = a + ty["w"][:, k].reshape(H, 1, 1) * ps[rows]
        aq = aq + ty["w"][:, k].reshape(H, 1) * psq[rows]
    e1 = np.maximum(np.abs(aq - sq(a)), E_FLOOR)
    asq = sq(a)
    lr = np.zeros((H, W, 3), F)
    q2 = np.zeros((H, W), F)
    for k in range(tx["w"].shape[1]):
        cols = np.clip(tx["lo"] + k, 0, dW - 1)
        lr = lr + tx["w"][:, k].reshape(1, W, 1) * a[:, cols]
        q2 = q2 + tx["w"][:, k].reshape(1, W) * asq[:, cols]
    e2 = np.maximum(np.abs(q2 - sq(lr)), E_FLOOR)
    f = tx["f"].reshape(1, W)
    e1i = ((F(1) - f) * e1[:, np.clip(tx["b0"], 0, dW - 1)]) + (f * e1[:, np.clip(tx["b0"] + 1, 0, dW - 1)])
    return np.concatenate([lr, (e2 + e1i)[..., None]], axis=2).astype(F)


def _var(v):
    h, w = v.shape[:2]
    xm, xp = np.clip(np.arange(w) - 1, 0, w - 1), np.clip(np.arange(w) + 1, 0, w - 1)
    ym, yp = np.clip(np.arange(h) - 1, 0, h - 1), np.clip(np.arange(h) + 1, 0, h - 1)
    nb = (v[:, xm], v[:, xp], v[ym], v[yp])
    m = v
    for t in nb:
        m = m + F(0.25) * t
    m = m / F(2)
    acc = sq(v - m)
    for t in nb:
        acc = acc + F(0.25) * sq(t - m)
    return np.maximum(acc / F(2), V_FLOOR)


def var(codes, lr):
    return _var(samples(codes)), _var(np.asarray(lr, F)[..., :3])


def _sat(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def final_parts(codes, pcodes, lr, vl, vh):
    """(pix float32 [dH][dW][3], Ws float32 [dH][dW]): the corrected pixel before the quantiser and the weight sum."""
    s = samples(codes)
    c0 = samples(pcodes)
    H, W = s.shape[:2]
    dH, dW = c0.shape[:2]
    ty, tx = fintab(H, dH), fintab(W, dW)
    lr = np.asarray(lr, F)
    wts = (F(0.5), F(1), F(0.5))
    gy = [np.clip(ty["ip"] + t, 0, H - 1) for t in (-1, 0, 1)]
    gx = [np.clip(tx["ip"] + t, 0, W - 1) for t in (-1, 0, 1)]
    mv = np.zeros((dH, dW), F)
    for X in range(3):
        for Y in range(3):
            mv = mv + (wts[X] * wts[Y]) * lr[gy[Y]][:, gx[X], 3]
    mv = mv / F(4)
    dsum = np.zeros((dH, dW, 3), F)
    ws = np.zeros((dH, dW), F)
    for X in range(3):
        for Y in range(3):
            g = lr[gy[Y]][:, gx[X]]
            r = F(-1.5) * np.sqrt(vl[gy[Y]][:, gx[X]] / (vh[gy[Y]][:, gx[X]] + mv))
            kk = tx["kern"][:, X].reshape(1, dW) * ty["kern"][:, Y].reshape(dH, 1)
            wt = kk / (sq(c0 - g[..., :3]) + g[..., 3])
            term = (s[gy[Y]][:, gx[X]] + g[..., :3] * r[..., None]) + ((F(-1) - r)[..., None] * c0)
            dsum = dsum + wt[..., None] * term
            ws = ws + wt
    return _sat(c0 + dsum / ws[..., None]), ws


def quant(img):
    return (np.asarray(img, F) * F(65535) + F(0.5)).astype(np.int32).astype(np.uint16)


def final(codes, pcodes, lr, vl, vh):
    return quant(final_parts(codes, pcodes, lr, vl, vh)[0])


def scale(codes, dH, dW, ssim=False):
    """hdrtv_post_rgb48_ssimsr on (H, W, 3) u16 codes."""
    codes = np.asarray(codes)
    assert codes.dtype == np.uint16 and codes.ndim == 3 and codes.shape[2] == 3
    h, w = codes.shape[:2]
    check_size(h, w, dH, dW)
    if (dH, dW) == (h, w):
        return codes.copy()
    p = spline36(codes, dH, dW)
    if not ssim:
        return p
    lr = lowres(p, h, w)
    vl, vh = var(codes, lr)
    return final(codes, p, lr, vl, vh)
