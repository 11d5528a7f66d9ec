"""The content light level record of include/hdrtv_mi355x.h (hdrtv_light_stats / hdrtv_rgb48_light_stats), restated in numpy: the
yardstick the GPU tests hold the kernels to bit for bit.  Input: the RGB48 codes a sink receives, u16 ``[H][W][3]``."""
import numpy as np

BINS, WORDS = 4096, 4104


def record(rgb48, rect=None):
    """The record (``WORDS`` u32) of the rectangle ``rect = (x0, y0, rw, rh)`` (default: the whole frame) of ``rgb48``."""
    a = np.asarray(rgb48)
    assert a.dtype == np.uint16 and a.ndim == 3 and a.shape[2] == 3
    h, w = a.shape[:2]
    x0, y0, rw, rh = (0, 0, w, h) if rect is None else rect
    assert rw > 0 and rh > 0 and 0 <= x0 <= w - rw and 0 <= y0 <= h - rh
    px = a[y0:y0 + rh, x0:x0 + rw].astype(np.uint32).reshape(-1, 3)
    m = px.max(axis=1)
    out = np.zeros(WORDS, dtype=np.uint32)
    out[:BINS] = np.bincount(m >> 4, minlength=BINS)
    out[4096:4099] = px.max(axis=0)
    out[4099] = m.max()
    s = int(m.astype(np.uint64).sum())
    out[4100], out[4101] = s & 0xFFFFFFFF, s >> 32
    out[4102] = rw * rh
    return out


def record_loop(rgb48, rect=None):
    """The same, pixel by pixel in plain Python: what ``record`` is checked against."""
    h, w = len(rgb48), len(rgb48[0])
    x0, y0, rw, rh = (0, 0, w, h) if rect is None else rect
    out = [0] * WORDS
    total = 0
    for y in range(y0, y0 + rh):
        for x in range(x0, x0 + rw):
            r, g, b = (int(v) for v in rgb48[y][x])
            m = max(r, g, b)
            out[m >> 4] += 1
            out[4096], out[4097], out[4098] = max(out[4096], r), max(out[4097], g), max(out[4098], b)
            out[4099] = max(out[4099], m)
            total += m
    out[4100], out[4101], out[4102] = total & 0xFFFFFFFF, total >> 32, rw * rh
    return np.array(out, dtype=np.uint32)
