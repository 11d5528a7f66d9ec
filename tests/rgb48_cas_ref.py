"""The contrast-adaptive sharpening rule of hdrtv_post_rgb48_scaled_cas (include/hdrtv_mi355x.h, step 1s), restated in plain
numpy on int64.

    code(s)                           -> the CAS code of a strength in [0, 1]: 0 = off, else K = 1032 .. 4084 (lib.cas_code restated)
    parts(src_u16_hwc, K)             -> the intermediate values as a dict of int64 arrays (mn, mx, q, r, A, den, t, num, out)
    sharpen(src_u16_hwc, K)           -> u16 [H][W][3]: the rule on every pixel of the FRAME, its edge pixels repeated
    scale(src_u16_hwc, dH, dW, K, a=0) -> u16 [dH][dW][3]: sharpen, then the two passes of rgb48_antiring_ref.scale with the
                                         anti-ringing code a (a = 0: rgb48_scale_ref.scale).  The scaler's taps outside the frame
                                         therefore read the SHARPENED edge pixel; K = 0 does not sharpen.
    ffmpeg_float(src_u16_hwc, s)      -> float64 [H][W][3]: ffmpeg's cas filter formula in floating point, unrounded, for orientation

This is FidelityFX CAS as ffmpeg's cas filter has it, (e + w (b + d + f + h)) / (1 + 4 w) with w = -amp / lerp(16, 4.03, s) and
amp = sqrt(clip(min(mn, 2 max - mx) / mx, 0, 1)), written as e + A t / den in integers.  ffmpeg is not part of the reference tree:
parity with it is UNPINNED.  For orientation only, measured in numpy (ffmpeg_float below against sharpen, a 200 x 300 x 3 frame of
full-range noise, seed 0) and asserted nowhere: the float formula lies within 49 codes of this rule at the reference's strengths
(46.3 / 47.9 / 48.8 at 0.16 / 0.20 / 0.22) and within 163 codes at s = 1, where 1 + 4 w falls to 0.0074 -- the largest differences
sit where q / mx is tiny and the 15-bit quotient under the root is coarse.  A 16384 / 49152 vertical step at K = 3426 becomes ... 16384, 14676, 50860, 49152 ... across the edge.
"""
import numpy as np

import rgb48_antiring_ref as A

K_MIN, K_MAX = 1032, 4096            # the codes the entry point takes beside 0


def code(s):
    c = int(float(s) * 256 + 0.5)
    return 0 if c == 0 else 4096 - ((c * 3064 + 128) >> 8)


def _isqrt(x):
    """floor(sqrt(x)) of an int64 array, exact: the float root, then corrected by its squares."""
    a = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    a -= (a * a > x)
    a += ((a + 1) * (a + 1) <= x)
    return a


def parts(src_u16_hwc, K):
    src = np.asarray(src_u16_hwc)
    assert src.dtype == np.uint16 and src.ndim == 3 and K_MIN <= int(K) <= K_MAX
    K = int(K)
    H, W = src.shape[:2]
    p = np.pad(src.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")          # the frame's edge pixels repeated
    n = {(dy, dx): p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    a, b, c, d, e, f, g, h, i = (n[k] for k in sorted(n))
    cross, diag = np.stack([b, d, e, f, h]), np.stack([a, c, g, i])
    mn5, mx5 = cross.min(axis=0), cross.max(axis=0)
    mn = mn5 + np.minimum(mn5, diag.min(axis=0))
    mx = mx5 + np.maximum(mx5, diag.max(axis=0))
    q = np.minimum(mn, 131070 - mx)
    r = np.where(mx > 0, (q << 15) // np.maximum(mx, 1), 0)
    amp = _isqrt(r << 9)
    den = 16 * K - 4 * amp
    t = 4 * e - (b + d + f + h)
    num = amp * t + (den >> 1)
    out = np.clip(e + num // den, 0, 65535)                                            # numpy's // on int64 floors
    return {"mn": mn, "mx": mx, "q": q, "r": r, "A": amp, "den": den, "t": t, "num": num, "out": out}


def sharpen(src_u16_hwc, K):
    return parts(src_u16_hwc, K)["out"].astype(np.uint16)


def scale(src_u16_hwc, dH, dW, K, a=0):
    src = np.asarray(src_u16_hwc)
    return A.scale(sharpen(src, K) if K else src, dH, dW, a)


def ffmpeg_float(src_u16_hwc, s):
    src = np.asarray(src_u16_hwc).astype(np.float64)
    H, W = src.shape[:2]
    p = np.pad(src, ((1, 1), (1, 1), (0, 0)), mode="edge")
    n = {(dy, dx): p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    a, b, c, d, e, f, g, h, i = (n[k] for k in sorted(n))
    cross, diag = np.stack([b, d, e, f, h]), np.stack([a, c, g, i])
    mn5, mx5 = cross.min(axis=0), cross.max(axis=0)
    mn = mn5 + np.minimum(mn5, diag.min(axis=0))
    mx = mx5 + np.maximum(mx5, diag.max(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.sqrt(np.clip(np.where(mx > 0, np.minimum(mn, 2 * 65535.0 - mx) / mx, 0.0), 0.0, 1.0))
    w = -amp / (16.0 + (4.03 - 16.0) * float(s))
    return np.clip((e + w * (b + d + f + h)) / (1.0 + 4.0 * w), 0.0, 65535.0)

