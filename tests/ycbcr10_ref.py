"""numpy restatement of the RGB48 -> 10-bit limited-range BT.2020nc Y'CbCr rule of include/hdrtv_mi355x.h (hdrtv_post_ycbcr10 /
hdrtv_rgb48_to_ycbcr10), the one the Y'CbCr tests hold the device to, bit for bit.  Takes the u16 RGB48 codes, returns the planes.
Not a test module: the test files import it."""
import math

import numpy as np

KR, KB = 0.2627, 0.0593
FORMATS = ("p010le", "yuv420p10le", "yuv422p10le")
SITINGS = ("left", "topleft")


def coefficients():
    """((YR, YG, YB), (UR, UG, UB), (VR, VG, VB)) at scale 2^20: rnd(v) = floor(v + 0.5) in double, green the remainder."""
    rnd = lambda v: int(math.floor(v + 0.5))        # noqa: E731
    sy, sc = 876.0 * 2 ** 20 / 65535.0, 896.0 * 2 ** 20 / 65535.0
    a, hc = rnd(sy), rnd(sc / 2)
    yr, yb = rnd(KR * sy), rnd(KB * sy)
    ur = rnd(-KR / (2 * (1 - KB)) * sc)
    vb = rnd(-KB / (2 * (1 - KR)) * sc)
    return (yr, a - yr - yb, yb), (ur, -hc - ur, hc), (hc, -hc - vb, vb)


def luma(rgb):
    """Y of every pixel of u16 codes (..., 3)."""
    (yr, yg, yb), _, _ = coefficients()
    c = rgb.astype(np.int64)
    return (64 + ((yr * c[..., 0] + yg * c[..., 1] + yb * c[..., 2] + (1 << 19)) >> 20)).astype(np.uint16)


def chroma(rgb, pix_fmt="yuv420p10le", siting="left"):
    """(Cb, Cr) planes of u16 codes (H, W, 3): the unrounded per-pixel u, v, the taps with edge repeat, one flooring shift."""
    if pix_fmt not in FORMATS or siting not in SITINGS:
        raise ValueError((pix_fmt, siting))
    h, w = rgb.shape[:2]
    v422 = pix_fmt == "yuv422p10le"
    if w % 2 or (not v422 and h % 2) or (v422 and siting != "left"):
        raise ValueError((h, w, pix_fmt, siting))
    _, cu, cv = coefficients()
    c = rgb.astype(np.int64)
    out = []
    for k in (cu, cv):
        p = k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2]
        x = np.arange(0, w, 2)
        hor = p[:, np.maximum(x - 1, 0)] + 2 * p[:, x] + p[:, np.minimum(x + 1, w - 1)]           # weight 4
        if v422:
            s, lg = hor, 2
        elif siting == "left":
            y = np.arange(0, h, 2)
            s, lg = hor[y] + hor[np.minimum(y + 1, h - 1)], 3
        else:
            y = np.arange(0, h, 2)
            s, lg = hor[np.maximum(y - 1, 0)] + 2 * hor[y] + hor[np.minimum(y + 1, h - 1)], 4
        out.append((512 + ((s + (1 << (19 + lg))) >> (20 + lg))).astype(np.uint16))
    return out[0], out[1]


def planes(rgb, pix_fmt="p010le", siting="left"):
    """(Y, Cb, Cr) u16 planes as the layout stores them: P010 carries the value in the high ten bits."""
    y = luma(rgb)
    cb, cr = chroma(rgb, pix_fmt, siting)
    if pix_fmt == "p010le":
        return y << 6, cb << 6, cr << 6
    return y, cb, cr


def frame_bytes(pix_fmt, h, w):
    """Bytes of a contiguous frame (hdrtv_ycbcr10_bytes)."""
    return h * w * (4 if pix_fmt == "yuv422p10le" else 3)


def plane_offsets(pix_fmt, h, w):
    """u16 offsets (y, u, v) of the planes of a contiguous frame and the chroma plane's (rows, u16 per row); P010: v is None and
    the one chroma plane holds Cb Cr pairs."""
    if pix_fmt == "p010le":
        return (0, h * w, None), (h // 2, w)
    ch = h if pix_fmt == "yuv422p10le" else h // 2
    return (0, h * w, h * w + ch * (w // 2)), (ch, w // 2)


def pack(rgb, pix_fmt="p010le", siting="left"):
    """The contiguous frame (1-D u16, planes back to back) the rule gives for RGB48 codes (H, W, 3)."""
    y, cb, cr = planes(rgb, pix_fmt, siting)
    if pix_fmt == "p010le":
        c = np.empty((cb.shape[0], cb.shape[1] * 2), np.uint16)
        c[:, 0::2], c[:, 1::2] = cb, cr
        return np.concatenate([y.reshape(-1), c.reshape(-1)])
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])


def exact(rgb):
    """(Y, Cb, Cr) of single pixels in double, unrounded: the formula the integer rule approximates."""
    c = rgb.astype(np.float64) / 65535.0
    yl = KR * c[..., 0] + (1 - KR - KB) * c[..., 1] + KB * c[..., 2]
    return 64 + 876 * yl, 512 + 896 * (c[..., 2] - yl) / (2 * (1 - KB)), 512 + 896 * (c[..., 0] - yl) / (2 * (1 - KR))
