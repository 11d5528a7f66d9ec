"""numpy restatement of the 8-bit 4:2:0 Y'CbCr -> BGR rule of include/hdrtv_mi355x.h (hdrtv_yuv420_to_bgr_u8), the one the
YUV tests hold the device to, bit for bit.  Not a test module: the test files import it."""
import math

import numpy as np

KRKB = {601: (0.299, 0.114), 709: (0.2126, 0.0722), 2020: (0.2627, 0.0593)}


def coefficients(matrix=709, full_range=False):
    """(A, RV, GU, GV, BU) from (Kr, Kb): rnd(v) = floor(v + 0.5) in double."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    rnd = lambda v: int(math.floor(v + 0.5))        # noqa: E731
    return (rnd(sy * 2 ** 16), rnd(2 * (1 - kr) * sc * 2 ** 13), rnd(2 * (1 - kb) * kb / kg * sc * 2 ** 13),
            rnd(2 * (1 - kr) * kr / kg * sc * 2 ** 13), rnd(2 * (1 - kb) * sc * 2 ** 13))


def upsample8(c, h, w):
    """8 x chroma at every luma pixel of an h x w frame from one (h/2, w/2) chroma plane: MPEG-2 / H.264 siting."""
    c = c.astype(np.int32)
    hc, wc = c.shape
    y = np.arange(h)
    j = y >> 1
    n = np.where(y & 1, np.minimum(j + 1, hc - 1), np.maximum(j - 1, 0))
    v4 = 3 * c[j] + c[n]                                           # (h, wc)
    x = np.arange(w)
    i = x >> 1
    i2 = np.where(x & 1, np.minimum(i + 1, wc - 1), i)
    return v4[:, i] + v4[:, i2]


def matrix_rgb(Y, c8u, c8v, matrix=709, full_range=False):
    """The matrix step: u8 (R, G, B) from luma bytes and 8 x chroma."""
    A, RV, GU, GV, BU = coefficients(matrix, full_range)
    y = Y.astype(np.int32) - (0 if full_range else 16)
    cb, cr = np.asarray(c8u, np.int32) - 1024, np.asarray(c8v, np.int32) - 1024
    r = (A * y + RV * cr + 32768) >> 16
    g = (A * y - GU * cb - GV * cr + 32768) >> 16
    b = (A * y + BU * cb + 32768) >> 16
    return tuple(np.clip(v, 0, 255).astype(np.uint8) for v in (r, g, b))


def planes_to_bgr(Y, U, V, matrix=709, full_range=False):
    """u8 (h, w, 3) B, G, R from the three planes."""
    h, w = Y.shape
    r, g, b = matrix_rgb(Y, upsample8(U, h, w), upsample8(V, h, w), matrix, full_range)
    return np.stack([b, g, r], axis=-1)


def split(frame, layout="i420"):
    """(Y, U, V) of a packed (H*3//2, W) frame: ffmpeg's yuv420p (I420) or nv12 layout."""
    h, w = frame.shape[0] // 3 * 2, frame.shape[1]
    Y = frame[:h]
    c = frame[h:].reshape(-1)
    if layout in ("i420", "yuv420p"):
        U = c[: (h // 2) * (w // 2)].reshape(h // 2, w // 2)
        V = c[(h // 2) * (w // 2):].reshape(h // 2, w // 2)
    else:
        uv = c.reshape(h // 2, w)
        U, V = uv[:, 0::2], uv[:, 1::2]
    return Y, U, V


def pack(Y, U, V, layout="i420"):
    """The packed (H*3//2, W) frame of three planes."""
    h, w = Y.shape
    if layout in ("i420", "yuv420p"):
        c = np.concatenate([U.reshape(-1), V.reshape(-1)]).reshape(h // 2, w)
    else:
        c = np.empty((h // 2, w), np.uint8)
        c[:, 0::2], c[:, 1::2] = U, V
    return np.ascontiguousarray(np.concatenate([Y, c], axis=0))


def to_bgr(frame, layout="i420", matrix=709, full_range=False):
    """The rule applied to a packed frame."""
    return planes_to_bgr(*split(frame, layout), matrix=matrix, full_range=full_range)


def random_frame(h, w, seed, layout="i420"):
    """A packed frame of seeded noise over the whole code range (so that every clamp is exercised)."""
    rng = np.random.default_rng(seed)
    Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    U = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    V = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    return pack(Y, U, V, layout)
