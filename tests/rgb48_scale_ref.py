"""The resampling rule of hdrtv_post_rgb48_scaled (include/hdrtv_mi355x.h), restated in plain Python / numpy.

    tab(n, m)                -> (start [m] int64, q [m][6] int64): first of the six source taps (i0 - 2, unclamped) and the
                                coefficients, sum 16384, of every destination index of one axis
    scale(src_u16_hwc, dH, dW) -> u16 [dH][dW][3]: the two integer passes over the CODES of an [H][W][3] frame

Nothing here comes from the reference (which leaves this resize to mpv or OpenCV: parity with either is UNPINNED).  The weights
are evaluated with math.sin / math.floor on Python floats (IEEE double), one tap at a time and summed in tap order, exactly as
the rule is written, so that the library's host tables can be held to them bit for bit.
"""
import functools
import math

import numpy as np

TAPS = 6
ONE = 16384          # 2^14: coefficient scale of one pass; the two passes together shift by 28


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def lanczos3(x):
    return _sinc(x) * _sinc(x / 3.0) if abs(x) < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def _tab(n, m):
    start = np.zeros(m, dtype=np.int64)
    q = np.zeros((m, TAPS), dtype=np.int64)
    for d in range(m):
        c = (d + 0.5) * n / m - 0.5
        i0 = math.floor(c)
        t = c - i0
        w = [lanczos3(t - k) for k in range(-2, 4)]
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


def tab(n, m):
    if m < n or n < 1:
        raise ValueError("enlarging only: m >= n >= 1")
    return _tab(int(n), int(m))


def hor_pass(src, dW):
    """int64 [H][dW][C] = sum_k src[y][clamp(start + k)][c] * qx_k (fits int32: asserted by the host tests)."""
    W = src.shape[1]
    start, q = tab(W, dW)
    s = src.astype(np.int64)
    out = np.zeros((src.shape[0], dW) + src.shape[2:], dtype=np.int64)
    for k in range(TAPS):
        idx = np.clip(start + k, 0, W - 1)
        out += s[:, idx] * q[:, k].reshape((1, dW) + (1,) * (src.ndim - 2))
    return out


def scale(src_u16_hwc, dH, dW):
    src = np.asarray(src_u16_hwc)
    assert src.dtype == np.uint16 and src.ndim == 3
    H = src.shape[0]
    hor = hor_pass(src, dW)
    start, q = tab(H, dH)
    acc = np.zeros((dH, dW, src.shape[2]), dtype=np.int64)
    for k in range(TAPS):
        idx = np.clip(start + k, 0, H - 1)
        acc += hor[idx] * q[:, k].reshape(dH, 1, 1)
    out = (acc + (1 << 27)) >> 28          # numpy's >> on int64 floors
    return np.clip(out, 0, 65535).astype(np.uint16)
