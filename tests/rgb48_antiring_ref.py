"""The anti-ringing rule of hdrtv_post_rgb48_scaled_ex (include/hdrtv_mi355x.h, steps 3a / 3b), restated in plain Python / numpy
on the tables and the horizontal sum of tests/rgb48_scale_ref.py.

    scale(src_u16_hwc, dH, dW, a)   -> u16 [dH][dW][3]: both passes, each pulled towards the interval of its two inner taps with
                                       the strength a = 0..256 (256 = full); a = 0 is rgb48_scale_ref.scale
    passes(src_u16_hwc, dH, dW, a)  -> the intermediate values as a dict of int64 arrays (hor, d_h, v, d_v), for the bound tests
    envelope(src_u16_hwc, dH, dW)   -> (lo, hi) u16 [dH][dW][3]: min / max of the 2 x 2 source codes around every output sample
                                       (the inner taps of the two axes), from the tables alone and not through scale

Modelled on mpv's separable scale-antiring; mpv is not part of the reference tree, parity with it is UNPINNED.  Python integers
behind numpy's int64: the largest product here is |d| * 256 < 2^54.
"""
import numpy as np

import rgb48_scale_ref as S

FULL = 256           # the strength code of 1.0


def _pull(raw, t2, t3, a):
    """raw + ((clamp(raw, lo, hi) - raw) * a + 128) >> 8 with lo / hi = min / max(t2, t3) << 14 -> (value, d)."""
    lo, hi = np.minimum(t2, t3) << 14, np.maximum(t2, t3) << 14
    d = np.clip(raw, lo, hi) - raw
    return raw + ((d * a + 128) >> 8), d           # numpy's >> on int64 floors


def passes(src_u16_hwc, dH, dW, a):
    src = np.asarray(src_u16_hwc)
    assert src.dtype == np.uint16 and src.ndim == 3 and 0 <= int(a) <= FULL
    a = int(a)
    H, W = src.shape[:2]
    s = src.astype(np.int64)
    xs, _ = S.tab(W, dW)
    raw_h = S.hor_pass(src, dW)
    hor, d_h = _pull(raw_h, s[:, np.clip(xs + 2, 0, W - 1)], s[:, np.clip(xs + 3, 0, W - 1)], a)
    ys, qy = S.tab(H, dH)
    raw_v = np.zeros((dH, dW, src.shape[2]), dtype=np.int64)
    for k in range(S.TAPS):
        raw_v += hor[np.clip(ys + k, 0, H - 1)] * qy[:, k].reshape(dH, 1, 1)
    v, d_v = _pull(raw_v, hor[np.clip(ys + 2, 0, H - 1)], hor[np.clip(ys + 3, 0, H - 1)], a)
    return {"hor": hor, "d_h": d_h, "v": v, "d_v": d_v}


def scale(src_u16_hwc, dH, dW, a):
    v = passes(src_u16_hwc, dH, dW, a)["v"]
    return np.clip((v + (1 << 27)) >> 28, 0, 65535).astype(np.uint16)


def envelope(src_u16_hwc, dH, dW):
    src = np.asarray(src_u16_hwc)
    assert src.dtype == np.uint16 and src.ndim == 3
    H, W = src.shape[:2]
    xs, _ = S.tab(W, dW)
    ys, _ = S.tab(H, dH)
    x2, x3 = np.clip(xs + 2, 0, W - 1), np.clip(xs + 3, 0, W - 1)
    y2, y3 = np.clip(ys + 2, 0, H - 1), np.clip(ys + 3, 0, H - 1)
    four = np.stack([src[y][:, x] for y in (y2, y3) for x in (x2, x3)])
    return four.min(axis=0), four.max(axis=0)
