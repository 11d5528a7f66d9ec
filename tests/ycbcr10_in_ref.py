"""numpy restatement of the 10-bit Y'CbCr -> RGB rule of include/hdrtv_mi355x.h (hdrtv_ycbcr10_to_rgb10), the one the 10-bit input
tests hold the device to, bit for bit.  Not a test module: the test files import it.  Frames are u16 arrays with the planes back to
back at minimum pitch: (H*3//2, W) for p010le / yuv420p10le, (2*H, W) for yuv422p10le."""
import math

import numpy as np

KRKB = {601: (0.299, 0.114), 709: (0.2126, 0.0722), 2020: (0.2627, 0.0593)}
FMT = {"p010le": 0, "yuv420p10le": 1, "yuv422p10le": 2}          # HDRTV_YCC_P010 / _YUV420P10 / _YUV422P10
PIX_FMTS = tuple(FMT)


def coefficients(matrix=709, full_range=False):
    """(A, RV, GU, GV, BU) from (Kr, Kb): rnd(v) = floor(v + 0.5) in double; sY = 1023/876, sC = 1023/896 (limited)."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (1023.0 / 876.0, 1023.0 / 896.0)
    rnd = lambda v: int(math.floor(v + 0.5))        # noqa: E731
    return (rnd(sy * 2 ** 16), rnd(2 * (1 - kr) * sc * 2 ** 13), rnd(2 * (1 - kb) * kb / kg * sc * 2 ** 13),
            rnd(2 * (1 - kr) * kr / kg * sc * 2 ** 13), rnd(2 * (1 - kb) * sc * 2 ** 13))


def upsample8(c, h, w):
    """8 x chroma at every luma pixel of an h x w frame from one chroma plane of ten-bit values: (h/2, w/2) -- 4:2:0, MPEG-2
    siting -- or (h, w/2) -- 4:2:2."""
    c = c.astype(np.int32)
    hc, wc = c.shape
    y = np.arange(h)
    if hc == h:
        v4 = 4 * c
    else:
        j = y >> 1
        n = np.where(y & 1, np.minimum(j + 1, hc - 1), np.maximum(j - 1, 0))
        v4 = 3 * c[j] + c[n]                                       # (h, wc)
    x = np.arange(w)
    i = x >> 1
    i2 = np.where(x & 1, np.minimum(i + 1, wc - 1), i)
    return v4[:, i] + v4[:, i2]


def matrix_rgb(Y, c8u, c8v, matrix=709, full_range=False):
    """The matrix step: ten-bit (R, G, B) as u16 from ten-bit luma and 8 x chroma.  int64 here; every intermediate fits int32."""
    A, RV, GU, GV, BU = coefficients(matrix, full_range)
    y = np.asarray(Y, np.int64) - (0 if full_range else 64)
    cb, cr = np.asarray(c8u, np.int64) - 4096, np.asarray(c8v, np.int64) - 4096
    terms = (A * y + RV * cr + 32768, A * y - GU * cb - GV * cr + 32768, A * y + BU * cb + 32768)
    assert all(np.abs(t).max(initial=0) < 2 ** 28 for t in terms)
    return tuple(np.clip(t >> 16, 0, 1023).astype(np.uint16) for t in terms)


def exact_rgb(Y, c8u, c8v, matrix=709, full_range=False):
    """The formula the rule approximates, in double, clamped to [0, 1023] and not rounded."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (1023.0 / 876.0, 1023.0 / 896.0)
    y = (np.asarray(Y, np.float64) - (0 if full_range else 64)) * sy
    cb, cr = (np.asarray(c8u, np.float64) / 8 - 512) * sc, (np.asarray(c8v, np.float64) / 8 - 512) * sc
    r = y + 2 * (1 - kr) * cr
    g = y - 2 * (1 - kb) * kb / kg * cb - 2 * (1 - kr) * kr / kg * cr
    b = y + 2 * (1 - kb) * cb
    return tuple(np.clip(v, 0, 1023) for v in (r, g, b))


def frame_shape(pix_fmt, h, w):
    return (2 * h, w) if pix_fmt == "yuv422p10le" else (h * 3 // 2, w)


def frame_hw(frame, pix_fmt):
    return (frame.shape[0] // 2 if pix_fmt == "yuv422p10le" else frame.shape[0] // 3 * 2), frame.shape[1]


def split(frame, pix_fmt):
    """(Y, U, V) sample WORDS (not yet shifted or masked) of a packed frame."""
    h, w = frame_hw(frame, pix_fmt)
    hc = h if pix_fmt == "yuv422p10le" else h // 2
    Y = frame[:h]
    c = frame[h:].reshape(-1)
    if pix_fmt == "p010le":
        uv = c.reshape(hc, w)
        return Y, uv[:, 0::2], uv[:, 1::2]
    return Y, c[: hc * (w // 2)].reshape(hc, w // 2), c[hc * (w // 2):].reshape(hc, w // 2)


def pack(Y, U, V, pix_fmt):
    """The packed frame of three planes of sample words."""
    h, w = Y.shape
    hc = U.shape[0]
    if pix_fmt == "p010le":
        c = np.empty((hc, w), np.uint16)
        c[:, 0::2], c[:, 1::2] = U, V
    else:
        c = np.concatenate([U.reshape(-1), V.reshape(-1)]).reshape(hc, w)
    return np.ascontiguousarray(np.concatenate([Y.astype(np.uint16), c.astype(np.uint16)], axis=0))


def values(words, pix_fmt):
    """Ten-bit values of sample words: word >> 6 (P010; the low six bits are ignored) or word & 0x3ff (planar)."""
    words = np.asarray(words, np.uint16)
    return (words >> 6) if pix_fmt == "p010le" else (words & 0x3FF)


def planes_to_rgb10(Y, U, V, matrix=709, full_range=False):
    """u16 (h, w, 3) R, G, B codes 0..1023 from the three planes of ten-bit VALUES."""
    h, w = Y.shape
    r, g, b = matrix_rgb(Y, upsample8(U, h, w), upsample8(V, h, w), matrix, full_range)
    return np.stack([r, g, b], axis=-1)


def to_rgb10(frame, pix_fmt, matrix=709, full_range=False):
    """The rule applied to a packed frame."""
    Y, U, V = (values(p, pix_fmt) for p in split(frame, pix_fmt))
    return planes_to_rgb10(Y, U, V, matrix, full_range)


def tensor_f16(codes):
    """The network's input tensor [3][H][W] of (h, w, 3) codes: fp16(float(code) * fp32(1/1023))."""
    t = codes.astype(np.float32) * np.float32(1.0 / 1023.0)
    return np.ascontiguousarray(t.astype(np.float16).transpose(2, 0, 1))


def tensor_f32(codes):
    return np.ascontiguousarray((codes.astype(np.float32) * np.float32(1.0 / 1023.0)).transpose(2, 0, 1))


def from_values(Y, U, V, pix_fmt, rng=None):
    """A packed frame holding the given ten-bit values; with ``rng`` the six unused bits of every word are noise."""
    def words(v):
        v = np.asarray(v, np.uint16)
        pad = rng.integers(0, 64, v.shape, dtype=np.uint16) if rng is not None else np.zeros(v.shape, np.uint16)
        return ((v << 6) | pad) if pix_fmt == "p010le" else (v | (pad << 10))
    return pack(words(Y), words(U), words(V), pix_fmt)


def random_frame(h, w, seed, pix_fmt, noisy_pad=False):
    """A packed frame of seeded noise over the whole ten-bit range (so that every clamp is exercised)."""
    rng = np.random.default_rng(seed)
    hc = h if pix_fmt == "yuv422p10le" else h // 2
    Y = rng.integers(0, 1024, (h, w), dtype=np.uint16)
    U = rng.integers(0, 1024, (hc, w // 2), dtype=np.uint16)
    V = rng.integers(0, 1024, (hc, w // 2), dtype=np.uint16)
    return from_values(Y, U, V, pix_fmt, rng if noisy_pad else None)


def grey_frame(Yvals, pix_fmt):
    """A frame with Cb = Cr = 512 and the given luma values."""
    h, w = Yvals.shape
    hc = h if pix_fmt == "yuv422p10le" else h // 2
    C = np.full((hc, w // 2), 512, np.uint16)
    return from_values(Yvals, C, C, pix_fmt)
