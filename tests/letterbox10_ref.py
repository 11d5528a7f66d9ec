"""numpy restatement of the 10-bit letterbox rule of include/hdrtv_mi355x.h (hdrtv_letterbox_ycbcr10), the one the tests hold the
device to, bit for bit.  Not a test module: the test files import it.

letterbox10(frame, dw, dh) is the reference's order of operations -- decode to RGB, then _letterbox_bgr -- at ten bits: the RGB10 codes
of every source pixel by ycbcr10_in_ref's rule (chroma clamps at the edges of the SOURCE frame), the geometry and tables of
oracle/letterbox_oracle.py, and that file's two resize loops restated here with u16 codes and a clamp to 1023 where it has u8 and 255.
Parity with OpenCV's own 16-bit resize is not claimed (its u16 cubic path is a float one)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import ycbcr10_in_ref as R                                                      # noqa: E402
from oracle.letterbox_oracle import AREA, CUBIC, _cv_round, area_tab, cubic_tab, geometry      # noqa: E402,F401

CODE_MAX = 1023
MAX_SHRINK = 4          # per axis: hdrtv_letterbox_ycbcr10 refuses sw > 4 new_w or sh > 4 new_h


def mode_of(sw, sh, dw, dh):
    """The path a geometry takes: 'copy', 'area_int', 'area_frac' or 'cubic' (LB_COPY .. LB_CUBIC of csrc/common.h)."""
    new_w, new_h, _, _, interp = geometry(sw, sh, dw, dh)
    if (new_w, new_h) == (sw, sh):
        return "copy"
    if interp == CUBIC:
        return "cubic"
    sx, sy = sw / new_w, sh / new_h
    eps = np.finfo(np.float64).eps
    return "area_int" if abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps else "area_frac"


def resize_area(src, new_w, new_h, top=CODE_MAX):
    """oracle.letterbox_oracle.resize_area on u16 codes, clamped to [0, top]."""
    h, w = src.shape[:2]
    sx, sy = w / new_w, h / new_h
    ix, iy = int(round(sx)), int(round(sy))
    if abs(sx - ix) < np.finfo(np.float64).eps and abs(sy - iy) < np.finfo(np.float64).eps:
        blk = src[: new_h * iy, : new_w * ix].reshape(new_h, iy, new_w, ix, -1).astype(np.int32).sum(axis=(1, 3), dtype=np.int32)
        if ix == 2 and iy == 2:
            return ((blk + 2) >> 2).astype(np.uint16)
        scale = np.float32(1.0) / np.float32(ix * iy)
        return np.clip(_cv_round(blk.astype(np.float32) * scale), 0, top).astype(np.uint16)
    xt, yt = area_tab(w, new_w), area_tab(h, new_h)
    s = src.astype(np.float32)
    buf = np.zeros((h, new_w, src.shape[2]), np.float32)         # horizontal sums, accumulated from 0 in table order
    for dx, sxk, alpha in xt:
        buf[:, dx] = buf[:, dx] + s[:, sxk] * alpha
    out = np.zeros((new_h, new_w, src.shape[2]), np.float32)
    first = [True] * new_h
    for dy, syk, beta in yt:
        if first[dy]:
            out[dy] = beta * buf[syk]
            first[dy] = False
        else:
            out[dy] = out[dy] + beta * buf[syk]
    return np.clip(_cv_round(out), 0, top).astype(np.uint16)


def resize_cubic(src, new_w, new_h, top=CODE_MAX):
    """oracle.letterbox_oracle.resize_cubic on u16 codes (int64 sums: 1023 x 2560 x 2560 exceeds 2^31), clamped to [0, top]."""
    h, w = src.shape[:2]
    xo, xc = cubic_tab(w, new_w)
    yo, yc = cubic_tab(h, new_h)
    s = src.astype(np.int64)
    hor = np.zeros((h, new_w, src.shape[2]), np.int64)
    for k in range(4):
        hor += s[:, np.clip(xo + k, 0, w - 1)] * xc[:, k][None, :, None]
    out = np.zeros((new_h, new_w, src.shape[2]), np.int64)
    for k in range(4):
        out += hor[np.clip(yo + k, 0, h - 1)] * yc[:, k][:, None, None]
    return np.clip((out + (1 << 21)) >> 22, 0, top).astype(np.uint16)


def letterbox_codes(codes, dw, dh, top=CODE_MAX):
    """The resize stage on its own: (sh, sw, 3) u16 codes -> (dh, dw, 3), code 0 outside the rectangle.  Unlike
    oracle.letterbox_bgr, equal sizes take the general path too (a COPY with no bars): the same array."""
    sh, sw = codes.shape[:2]
    new_w, new_h, x0, y0, interp = geometry(sw, sh, dw, dh)
    if (new_w, new_h) == (sw, sh):
        resized = codes
    elif interp == AREA:
        resized = resize_area(codes, new_w, new_h, top)
    else:
        resized = resize_cubic(codes, new_w, new_h, top)
    canvas = np.zeros((dh, dw, 3), np.uint16)
    canvas[y0:y0 + new_h, x0:x0 + new_w] = resized
    return canvas


def letterbox10(frame, dw, dh, pix_fmt, matrix=709, full_range=False):
    """The rule applied to a packed 10-bit frame (ycbcr10_in_ref's layout): (dh, dw, 3) u16 R, G, B codes 0..1023."""
    return letterbox_codes(R.to_rgb10(frame, pix_fmt, matrix, full_range), dw, dh)
