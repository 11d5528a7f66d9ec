"""The shrinking rule of hdrtv_post_rgb48_down (include/hdrtv_mi355x.h), restated in plain Python / numpy: a Mitchell downscale of
the u16 codes (stage A, an integer rule built like tests/rgb48_scale_ref.py, with the anti-ringing `_pull` of
tests/rgb48_antiring_ref.py) and, with ssim, the structure-preserving correction of the reference's display chain on top of it
(stage B, float32 operation by operation, with the conventions of tests/rgb48_fsr_ref.py: NumPy rounds every elementwise multiply,
add, subtract, divide and square root on its own and fuses nothing, denormals are kept).

    tab(n, m)                          -> per-axis tables as a Tab (lo, cnt, k2, q, w), see below
    mitchell(codes, dH, dW, a=0)       -> u16 [dH][dW][3]: stage A, the Mitchell codes M
    l2(codes, dH, dW)                  -> float32 [dH][dW][3]: the Catmull-Rom mean of squares of the source samples
    ssim(codes, mcodes, dH, dW)        -> u16 [dH][dW][3]: stage B, a pure function of the source codes and the Mitchell codes
    scale(codes, dH, dW, a=0, ssim=False)

Footprint of an axis with n source and m destination samples, n / 4 <= m <= n, in double for d = 0 .. m - 1:
    ctr = (d + 0.5) * n / m;  hw = 2.0 * n / m;  k_lo = ceil(ctr - hw - 0.5);  k_hi = floor(ctr + hw - 0.5)
    tap k lies at x_k = (k + 0.5 - ctr) * m / n (destination pixels);  k2 = floor(ctr - 0.5), the left of the two bracketing samples
The kernel is stretched by the ratio (mpv's correct-downscaling); at most floor(4 n / m) + 1 <= 17 taps.  Tables are padded to the
axis' largest count with zero coefficients.  m == n is one tap, k = d, weight one, in both stages.

Stage A.  weight mitchell(x_k), B = C = 1/3, written so that a C++ double evaluation gives the same bits:
    |x| < 1:  ((7 |x| - 12) |x| |x| + 16/3) / 6;   |x| < 2:  ((((-7/3) |x| + 12) |x| - 20) |x| + 32/3) / 6;   else 0
summed in tap order, q_k = floor(v_k / s * 16384 + 0.5), the remainder to the largest coefficient (the lowest k on a tie).
Horizontal pass, pull, vertical pass, pull, (acc + 2^27) >> 28, clamp: the Lanczos rule's shapes; the two inner taps of the pull
are the source samples k2 and k2 + 1, clamped to the frame.  mpv is not part of the reference tree: parity with its own Mitchell
arithmetic is UNPINNED.

Stage B, the orders the display shader leaves open fixed here:
    samples     s = float32(c) / float32(65535), Ms = float32(M) / float32(65535)
    L2 weight   cr(|x_k|) in double, cr(x) = (1.5 x - 2.5) x x + 1 for x < 1, ((-0.5 x + 2.5) x - 4) x + 2 otherwise; divided by
                the sum (in double, tap order), then rounded to float32: the shader's division by W is folded into the table
    L2 pass 1   vertical on s * s (one rounded multiply): acc = acc + wy_k * (s * s), k ascending from acc = 0
    L2 pass 2   horizontal on pass 1's float32 values, likewise; no anti-ringing
    mean3(v)    taps -1, 0, 1, weights 0.5, 1, 0.5, neighbours clamped to the image: inside a row h = ((0.5 v[-1] + v[0]) + 0.5 v[1]) / 2,
                then over the rows ((0.5 h[-1] + h[0]) + 0.5 h[1]) / 2
    MR          mM = mean3(Ms), mQ = mean3(Ms * Ms), mL = mean3(L2) per channel;  Sl = luma(max(mQ - mM mM, 0)),
                Sh = luma(max(mL - mM mM, 0)),  luma = (0.2126 r + 0.7152 g) + 0.0722 b,  sigma = float32(10 / (255 * 255))
                R = Sl > Sh ? min(max(Sh / Sl, 0), 1) : sqrt((Sh + sigma) / (Sl + sigma))          (a select)
    final       a0 = mean3(R * mM), a1 = mean3(mM), a2 = mean3(R);  pix = sat((a1 + a2 * Ms) - a0);  code = (int)(pix * 65535 + 0.5)
A flat frame returns its code (the sums are exact, Sl = Sh = 0, R = 1).  What a display's GLSL compiler makes of the shader is
UNPINNED.
"""
import collections
import functools
import math

import numpy as np

import rgb48_antiring_ref as AR

F = np.float32
ONE = 16384
MAX_RATIO = 4
MAX_TAPS = 4 * MAX_RATIO + 1
LUMA_R, LUMA_G, LUMA_B = F(0.2126), F(0.7152), F(0.0722)
SIGMA = F(10.0 / (255.0 * 255.0))
AUTO_ANTIRING = 51            # floor(0.20 * 256 + 0.5): the reference's dscale-antiring as a strength code

# lo [m]: first tap (unclamped), cnt [m]: taps of that index, k2 [m]: the left bracketing sample (unclamped), q [m][nt] int64 (sum
# 16384) and w [m][nt] float32 (the L2 weights), nt = the axis' largest count
Tab = collections.namedtuple("Tab", "lo cnt k2 q w")


def mitchell_w(x):
    x = abs(x)
    if x < 1.0:
        return ((7.0 * x - 12.0) * x * x + 16.0 / 3.0) / 6.0
    if x < 2.0:
        return ((((-7.0 / 3.0) * x + 12.0) * x - 20.0) * x + 32.0 / 3.0) / 6.0
    return 0.0


def catrom_w(x):
    x = abs(x)
    if x < 1.0:
        return (1.5 * x - 2.5) * x * x + 1.0
    return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0


def footprint(n, m, d):
    """(k_lo, k_hi, k2, [x_k]) of destination index d."""
    ctr = (d + 0.5) * n / m
    hw = 2.0 * n / m
    lo, hi = math.ceil(ctr - hw - 0.5), math.floor(ctr + hw - 0.5)
    return lo, hi, math.floor(ctr - 0.5), [(k + 0.5 - ctr) * m / n for k in range(lo, hi + 1)]


@functools.lru_cache(maxsize=None)
def _tab(n, m):
    if m == n:
        idx = np.arange(m, dtype=np.int64)
        rows = [(int(d), 1, int(d), [ONE], [1.0]) for d in idx]
    else:
        rows = []
        for d in range(m):
            lo, hi, k2, xs = footprint(n, m, d)
            v = [mitchell_w(x) for x in xs]
            s = 0.0
            for t in v:
                s += t
            q = [int(math.floor(t / s * ONE + 0.5)) for t in v]
            big = 0
            for k in range(len(q)):
                if q[k] > q[big]:          # the lowest k on a tie
                    big = k
            q[big] += ONE - sum(q)
            c = [catrom_w(x) for x in xs]
            cs = 0.0
            for t in c:
                cs += t
            rows.append((lo, hi - lo + 1, k2, q, [t / cs for t in c]))
    nt = max(r[1] for r in rows)
    lo = np.array([r[0] for r in rows], dtype=np.int64)
    cnt = np.array([r[1] for r in rows], dtype=np.int64)
    k2 = np.array([r[2] for r in rows], dtype=np.int64)
    q = np.zeros((m, nt), dtype=np.int64)
    w = np.zeros((m, nt), dtype=F)
    for d, r in enumerate(rows):
        q[d, :r[1]] = r[3]
        w[d, :r[1]] = np.array(r[4], dtype=np.float64).astype(F)
    for a in (lo, cnt, k2, q, w):
        a.setflags(write=False)
    return Tab(lo, cnt, k2, q, w)


def tab(n, m):
    n, m = int(n), int(m)
    if n < 1 or m < 1 or m > n or MAX_RATIO * m < n:
        raise ValueError(f"shrinking by 1 .. {MAX_RATIO} per axis: {n} -> {m}")
    return _tab(n, m)


def hor_pass(src, dW):
    """int64 [H][dW][C] = sum_k src[y][clamp(lo + k)][c] * qx_k, rgb48_scale_ref.hor_pass with this rule's tables."""
    W = src.shape[1]
    t = tab(W, dW)
    s = src.astype(np.int64)
    out = np.zeros((src.shape[0], dW) + src.shape[2:], dtype=np.int64)
    for k in range(t.q.shape[1]):
        out += s[:, np.clip(t.lo + k, 0, W - 1)] * t.q[:, k].reshape((1, dW) + (1,) * (src.ndim - 2))
    return out


def passes(codes, dH, dW, a=0):
    """Stage A's intermediate values as a dict of int64 arrays (raw_h, hor, v), for the bound tests."""
    src = np.asarray(codes)
    assert src.dtype == np.uint16 and src.ndim == 3 and 0 <= int(a) <= AR.FULL
    a = int(a)
    H, W = src.shape[:2]
    tx, ty = tab(W, dW), tab(H, dH)
    s = src.astype(np.int64)
    raw_h = hor_pass(src, dW)
    hor, _ = AR._pull(raw_h, s[:, np.clip(tx.k2, 0, W - 1)], s[:, np.clip(tx.k2 + 1, 0, W - 1)], a)
    raw_v = np.zeros((dH, dW, src.shape[2]), dtype=np.int64)
    for k in range(ty.q.shape[1]):
        raw_v += hor[np.clip(ty.lo + k, 0, H - 1)] * ty.q[:, k].reshape(dH, 1, 1)
    v, _ = AR._pull(raw_v, hor[np.clip(ty.k2, 0, H - 1)], hor[np.clip(ty.k2 + 1, 0, H - 1)], a)
    return {"raw_h": raw_h, "hor": hor, "v": v}


def mitchell(codes, dH, dW, a=0):
    v = passes(codes, dH, dW, a)["v"]
    return np.clip((v + (1 << 27)) >> 28, 0, 65535).astype(np.uint16)


def samples(codes):
    return np.asarray(codes).astype(F) / F(65535)


def l2(codes, dH, dW):
    s = samples(codes)
    H, W = s.shape[:2]
    tx, ty = tab(W, dW), tab(H, dH)
    sq = s * s
    v1 = np.zeros((dH, W, s.shape[2]), F)
    for k in range(ty.w.shape[1]):
        v1 = v1 + ty.w[:, k].reshape(dH, 1, 1) * sq[np.clip(ty.lo + k, 0, H - 1)]
    out = np.zeros((dH, dW, s.shape[2]), F)
    for k in range(tx.w.shape[1]):
        out = out + tx.w[:, k].reshape(1, dW, 1) * v1[:, np.clip(tx.lo + k, 0, W - 1)]
    return out


def mean3(v):
    """The 0.5 / 1 / 0.5 mean over the 3 x 3 neighbourhood, neighbours clamped to the image; float32, rows first."""
    v = np.asarray(v, F)
    h, w = v.shape[:2]
    xm, xp = np.clip(np.arange(w) - 1, 0, w - 1), np.clip(np.arange(w) + 1, 0, w - 1)
    ym, yp = np.clip(np.arange(h) - 1, 0, h - 1), np.clip(np.arange(h) + 1, 0, h - 1)
    r = ((F(0.5) * v[:, xm] + v) + F(0.5) * v[:, xp]) / F(2)
    return ((F(0.5) * r[ym] + r) + F(0.5) * r[yp]) / F(2)


def _luma(c):
    return (LUMA_R * c[..., 0] + LUMA_G * c[..., 1]) + LUMA_B * c[..., 2]


def _sat(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def ratio(ms, l2v):
    """(mM, R): the 3 x 3 mean of the Mitchell samples and the shader's variance ratio, float32."""
    mm, mq, ml = mean3(ms), mean3(ms * ms), mean3(l2v)
    sq = mm * mm
    sl = _luma(np.maximum(mq - sq, F(0)))
    sh = _luma(np.maximum(ml - sq, F(0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = _sat(sh / sl)
        b = np.sqrt((sh + SIGMA) / (sl + SIGMA))
    return mm, np.where(sl > sh, a, b).astype(F)


def quant(img):
    return (np.asarray(img, F) * F(65535) + F(0.5)).astype(np.int32).astype(np.uint16)


def ssim(codes, mcodes, dH, dW):
    ms = samples(mcodes)
    assert ms.shape[:2] == (dH, dW)
    mm, r = ratio(ms, l2(codes, dH, dW))
    a0, a1, a2 = mean3(r[..., None] * mm), mean3(mm), mean3(r)
    return quant(_sat((a1 + a2[..., None] * ms) - a0))


_stage_b = ssim          # scale's keyword shadows the function


def scale(codes, dH, dW, a=0, ssim=False):
    """hdrtv_post_rgb48_down on (H, W, 3) u16 codes.  Equal sizes return the codes; enlarging on either axis, or more than 4x, is
    refused."""
    codes = np.asarray(codes)
    h, w = codes.shape[:2]
    if dH > h or dW > w or MAX_RATIO * dH < h or MAX_RATIO * dW < w or dH < 1 or dW < 1:
        raise ValueError(f"shrinking by 1 .. {MAX_RATIO} per axis: {w}x{h} -> {dW}x{dH}")
    if (dH, dW) == (h, w):
        return codes.astype(np.uint16)
    m = mitchell(codes, dH, dW, a)
    return _stage_b(codes, m, dH, dW) if ssim else m
