"""numpy restatement of the Floyd-Steinberg error-diffusion rule of include/hdrtv_mi355x.h (hdrtv_post_ycbcr10_fs /
hdrtv_rgb48_to_ycbcr10_fs), the one the error-diffusion tests hold the device to, bit for bit.  Takes the u16 RGB48 codes, returns
the planes.  The rule is this project's own integer rule: parity with zimg's error diffusion (which diffuses in float) is UNPINNED.
The diffusion is stated twice: a scalar raster loop (``diffuse_scalar``: the rule as written) and a skewed wavefront over
s = x + 2 y with vector operations (``diffuse``: what the tests can afford at their sizes); tests/test_fs_host.py holds the two to
each other.  Coefficients and layouts are those of tests/ycbcr10_ref.py.  Not a test module: the test files import it."""
import numpy as np

import ycbcr10_ref as R

LUMA = (20, 64, 0, 876)             # SH, base, lowest and highest k
CHROMA_RANGE = (512, -448, 448)     # base, lowest and highest k; SH is 22 (4:2:2), 23 (4:2:0 left) or 24 (4:2:0 top-left)
E_BOUND = 2050                      # 2047 + 3: what a carried error can reach (a, b, c, d of up to four residuals)


def sums(rgb, pix_fmt="p010le", siting="left"):
    """((S_y, SH_y), (S_cb, SH_c), (S_cr, SH_c)): the integer sums the undithered rule forms per sample (int64 planes) and their
    shifts -- ycbcr10_ref.luma / chroma without the rounding constant and the shift."""
    if pix_fmt not in R.FORMATS or siting not in R.SITINGS:
        raise ValueError((pix_fmt, siting))
    h, w = rgb.shape[:2]
    v422 = pix_fmt == "yuv422p10le"
    if w % 2 or (not v422 and h % 2) or (v422 and siting != "left"):
        raise ValueError((h, w, pix_fmt, siting))
    ky, cu, cv = R.coefficients()
    c = rgb.astype(np.int64)
    out = [(ky[0] * c[..., 0] + ky[1] * c[..., 1] + ky[2] * c[..., 2], LUMA[0])]
    for k in (cu, cv):
        p = k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2]
        x = np.arange(0, w, 2)
        hor = p[:, np.maximum(x - 1, 0)] + 2 * p[:, x] + p[:, np.minimum(x + 1, w - 1)]
        y = np.arange(0, h, 2)
        if v422:
            s, lg = hor, 2
        elif siting == "left":
            s, lg = hor[y] + hor[np.minimum(y + 1, h - 1)], 3
        else:
            s, lg = hor[np.maximum(y - 1, 0)] + 2 * hor[y] + hor[np.minimum(y + 1, h - 1)], 4
        out.append((s, 20 + lg))
    return tuple(out)


def samples(s, sh):
    """u: the sample in 1/4096 code, (S + (1 << (SH - 13))) >> (SH - 12) with an arithmetic shift."""
    return (s + (1 << (sh - 13))) >> (sh - 12)


def _split(r):
    a, b, c = (7 * r) >> 4, (3 * r) >> 4, (5 * r) >> 4
    return a, b, c, r - a - b - c


def diffuse_scalar(u, lo, hi, with_error=False):
    """The rule as written: raster order, E = 0 at the start.  u: (h, w) integers.  -> k (int64), and max |E| on request."""
    h, w = u.shape
    e = [[0] * (w + 2) for _ in range(h + 1)]        # column x at index x + 1: terms outside the plane land in unused cells
    k = np.zeros((h, w), np.int64)
    emax = 0
    for j in range(h):
        for i in range(w):
            emax = max(emax, abs(e[j][i + 1]))
            v = int(u[j, i]) + e[j][i + 1]
            q = min(max((v + 2048) >> 12, lo), hi)
            r = min(max(v - 4096 * q, -2048), 2047)
            a, b, c, d = _split(r)
            e[j][i + 2] += a
            e[j + 1][i] += b
            e[j + 1][i + 1] += c
            e[j + 1][i + 2] += d
            k[j, i] = q
    return (k, emax) if with_error else k


def diffuse(u, lo, hi, with_error=False):
    """The same rule as a skewed wavefront: all samples with x + 2 y = s depend only on samples of smaller s, so one vector
    operation per s handles them together."""
    h, w = u.shape
    u = u.astype(np.int64)
    e = np.zeros((h + 1, w + 2), np.int64)
    k = np.zeros((h, w), np.int64)
    emax = 0
    for s in range(w + 2 * (h - 1)):
        y = np.arange(max(0, (s - w + 2) // 2), min(h - 1, s // 2) + 1)
        x = s - 2 * y
        y, x = y[(x >= 0) & (x < w)], x[(x >= 0) & (x < w)]
        if not len(y):              # a plane one sample wide has nothing on odd s
            continue
        if with_error:
            emax = max(emax, int(np.abs(e[y, x + 1]).max()))
        v = u[y, x] + e[y, x + 1]
        q = np.clip((v + 2048) >> 12, lo, hi)
        a, b, c, d = _split(np.clip(v - 4096 * q, -2048, 2047))
        e[y, x + 2] += a            # distinct rows: no index repeats within one statement
        e[y + 1, x] += b
        e[y + 1, x + 1] += c
        e[y + 1, x + 2] += d
        k[y, x] = q
    return (k, emax) if with_error else k


def planes(rgb, pix_fmt="p010le", siting="left", diffuse_fn=diffuse):
    """(Y, Cb, Cr) u16 planes as the layout stores them: P010 carries the value in the high ten bits."""
    (sy, shy), (su, shc), (sv, _) = sums(rgb, pix_fmt, siting)
    base, lo, hi = CHROMA_RANGE
    y = LUMA[1] + diffuse_fn(samples(sy, shy), LUMA[2], LUMA[3])
    cb = base + diffuse_fn(samples(su, shc), lo, hi)
    cr = base + diffuse_fn(samples(sv, shc), lo, hi)
    shl = 6 if pix_fmt == "p010le" else 0
    return tuple((p << shl).astype(np.uint16) for p in (y, cb, cr))


def pack(rgb, pix_fmt="p010le", siting="left"):
    """The contiguous frame (1-D u16, planes back to back, ycbcr10_ref.pack's layout) the rule gives for RGB48 codes (H, W, 3)."""
    y, cb, cr = planes(rgb, pix_fmt, siting)
    if pix_fmt == "p010le":
        c = np.empty((cb.shape[0], cb.shape[1] * 2), np.uint16)
        c[:, 0::2], c[:, 1::2] = cb, cr
        return np.concatenate([y.reshape(-1), c.reshape(-1)])
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
