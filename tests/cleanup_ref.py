"""numpy restatement of the output-cleanup rules of include/hdrtv_mi355x.h: the deband rule of hdrtv_rgb48_deband (RGB48 codes ->
RGB48 codes) and the ordered-dither form of the 10-bit Y'CbCr rule (hdrtv_post_ycbcr10_ex / hdrtv_rgb48_to_ycbcr10_ex), the ones the
cleanup tests hold the device to, bit for bit.  The undithered rule and the frame layouts are tests/ycbcr10_ref.py's.
Not a test module: the test files import it."""
import numpy as np

import ycbcr10_ref as R

RANGE, THRESHOLD = 16, 1311                 # the defaults: the largest reach, rnd(0.02 * 65535)
assert THRESHOLD == int(np.floor(0.02 * 65535 + 0.5))


# ---------------------------------------------------------------------------------------------------------------- deband
def deband_offsets(h, w, rng=RANGE, seed=0):
    """(dx, dy) of every pixel, int64 (h, w), each in [-rng, rng]: the rule's hash of S * 0x9E3779B9 + y * W + x in u32."""
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    v = (np.uint64(seed & 0xFFFFFFFF) * np.uint64(0x9E3779B9) + y * np.uint64(w) + x) & m
    v ^= v >> np.uint64(16)
    v = (v * np.uint64(0x7FEB352D)) & m
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x846CA68B)) & m
    v ^= v >> np.uint64(16)
    span = np.uint64(2 * rng + 1)
    dx = (((v & np.uint64(0xFFFF)) * span) >> np.uint64(16)).astype(np.int64) - rng
    dy = (((v >> np.uint64(16)) * span) >> np.uint64(16)).astype(np.int64) - rng
    return dx, dy


def deband_refs(h, w, rng=RANGE, seed=0):
    """The four reference positions of every pixel, clamped to the frame: [(ys, xs)] * 4 of int64 (h, w)."""
    dx, dy = deband_offsets(h, w, rng, seed)
    y, x = np.mgrid[0:h, 0:w]
    cx = lambda v: np.clip(v, 0, w - 1)        # noqa: E731
    cy = lambda v: np.clip(v, 0, h - 1)        # noqa: E731
    return [(cy(y + dy), cx(x + dx)), (cy(y + dy), cx(x - dx)), (cy(y - dy), cx(x - dx)), (cy(y - dy), cx(x + dx))]


def deband(rgb, rng=RANGE, threshold=THRESHOLD, seed=0):
    """The debanded frame of u16 codes (H, W, 3); a new array."""
    if rgb.dtype != np.uint16 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("u16 (H, W, 3)")
    if not 1 <= rng <= 16 or not 1 <= threshold <= 65535:
        raise ValueError((rng, threshold))
    h, w = rgb.shape[:2]
    src = rgb.astype(np.int64)
    refs = [src[ys, xs] for ys, xs in deband_refs(h, w, rng, seed)]
    flat = np.ones((h, w), bool)
    for r in refs:
        flat &= (np.abs(r - src) < threshold).all(axis=2)
    avg = (refs[0] + refs[1] + refs[2] + refs[3] + 2) >> 2
    return np.where(flat[..., None], avg, src).astype(np.uint16)


def staircase():
    """The 64 x 512 test picture of the rule: steps of 514 codes every 32 columns from 10000, a 4-pixel line at code 60000 in columns
    254 .. 257 -> (frame, boolean (H, W) mask of the line)."""
    h, w = 64, 512
    f = np.empty((h, w, 3), np.uint16)
    f[...] = (10000 + (np.arange(w) // 32) * 514).astype(np.uint16)[None, :, None]
    line = np.zeros((h, w), bool)
    line[:, 254:258] = True
    f[line] = 60000
    return f, line


# ---------------------------------------------------------------------------------------------------------------- ordered dither
def bayer_index(x, y):
    """M(x, y) in 0..255: bit i of (x ^ y) & 15 at bit 7 - 2i, bit i of y & 15 at bit 6 - 2i."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    a, b = (x ^ y) & 15, y & 15
    m = np.zeros(np.broadcast(a, b).shape, np.int64)
    for i in range(4):
        m |= ((a >> i) & 1) << (7 - 2 * i)
        m |= ((b >> i) & 1) << (6 - 2 * i)
    return m


def bayer_recursive(n=16):
    """The n x n ordered-dither matrix built from [[0, 2], [3, 1]]: M_2n = [[4 M, 4 M + 2], [4 M + 3, 4 M + 1]], indexed [y][x]."""
    m = np.zeros((1, 1), np.int64)
    while m.shape[0] < n:
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m


def luma_sum(rgb):
    """YR R + YG G + YB B of u16 codes (..., 3), int64: Y is 64 + (sum + rounding) >> 20."""
    (yr, yg, yb), _, _ = R.coefficients()
    c = rgb.astype(np.int64)
    return yr * c[..., 0] + yg * c[..., 1] + yb * c[..., 2]


def luma(rgb, dither=0):
    if not dither:
        return R.luma(rgb)
    h, w = rgb.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    t = (2 * bayer_index(x, y) + 1) << 11
    return (64 + ((luma_sum(rgb) + t) >> 20)).astype(np.uint16)


def chroma(rgb, pix_fmt="yuv420p10le", siting="left", dither=0):
    """(Cb, Cr): tests/ycbcr10_ref.chroma's sums and shift, the constant (2 M(i, j) + 1) << (SH - 9) over the chroma plane."""
    if not dither:
        return R.chroma(rgb, pix_fmt, siting)
    if pix_fmt not in R.FORMATS or siting not in R.SITINGS:
        raise ValueError((pix_fmt, siting))
    h, w = rgb.shape[:2]
    v422 = pix_fmt == "yuv422p10le"
    if w % 2 or (not v422 and h % 2) or (v422 and siting != "left"):
        raise ValueError((h, w, pix_fmt, siting))
    _, cu, cv = R.coefficients()
    c = rgb.astype(np.int64)
    out = []
    for k in (cu, cv):
        p = k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2]
        x = np.arange(0, w, 2)
        hor = p[:, np.maximum(x - 1, 0)] + 2 * p[:, x] + p[:, np.minimum(x + 1, w - 1)]
        if v422:
            s, sh = hor, 22
        elif siting == "left":
            y = np.arange(0, h, 2)
            s, sh = hor[y] + hor[np.minimum(y + 1, h - 1)], 23
        else:
            y = np.arange(0, h, 2)
            s, sh = hor[np.maximum(y - 1, 0)] + 2 * hor[y] + hor[np.minimum(y + 1, h - 1)], 24
        j, i = np.mgrid[0:s.shape[0], 0:s.shape[1]]
        out.append((512 + ((s + ((2 * bayer_index(i, j) + 1) << (sh - 9))) >> sh)).astype(np.uint16))
    return out[0], out[1]


def planes(rgb, pix_fmt="p010le", siting="left", dither=0):
    y = luma(rgb, dither)
    cb, cr = chroma(rgb, pix_fmt, siting, dither)
    if pix_fmt == "p010le":
        return y << 6, cb << 6, cr << 6
    return y, cb, cr


def pack(rgb, pix_fmt="p010le", siting="left", dither=0):
    """The contiguous frame (1-D u16, planes back to back), as tests/ycbcr10_ref.pack; dither 0 = none, 1 = ordered."""
    y, cb, cr = planes(rgb, pix_fmt, siting, dither)
    if pix_fmt == "p010le":
        c = np.empty((cb.shape[0], cb.shape[1] * 2), np.uint16)
        c[:, 0::2], c[:, 1::2] = cb, cr
        return np.concatenate([y.reshape(-1), c.reshape(-1)])
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])


def cleanup(rgb, pix_fmt, siting="left", deband_on=False, rng=RANGE, threshold=THRESHOLD, dither=0):
    """What the output stage delivers for RGB48 codes: deband (seed 0) first, then rgb48le as it is or the (dithered) planes."""
    if deband_on:
        rgb = deband(rgb, rng, threshold, 0)
    return rgb if pix_fmt == "rgb48le" else pack(rgb, pix_fmt, siting, dither)
