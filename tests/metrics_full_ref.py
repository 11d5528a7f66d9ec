"""numpy restatement of rules R1 .. R6 of include/hdrtv_mi355x.h (hdrtv_full_reference_metrics and its pieces): what the reference's
_compute_full_reference_metrics (src/gui_objective_metrics.py:617-677) does to two RGB48 frames u16 [H][W][3].  Not a test module:
the test files import it.

The integer stages (border counts and bounds, evaluation size, 16-bit INTER_AREA, histograms, gain / bias, normalised codes) are the
rules the device is held to bit for bit; the three formulas are oracle/metrics_oracle.py's.  Parity with OpenCV's own 16-bit
INTER_AREA is not claimed (cv2 is not part of the reference tree), as for the 8-bit rule of oracle/letterbox_oracle.py.

One deliberate departure from the reference's literal text: it takes np.mean / np.std of float32 arrays (pairwise float32 sums in
numpy's own order); R5 takes them from exact histograms in float64.  ``grade_match_literal`` is the literal text, and
tests/test_metrics_full_host.py measures the distance between the two."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from oracle import metrics_oracle as M                                          # noqa: E402
from oracle.letterbox_oracle import _cv_round, area_tab                         # noqa: E402

SIGNAL_MIN = 132        # max(R, G, B) > max(2, 65535 * 0.002) = 131.07
MIN_BORDER = 8
MAX_SIDE = 512
MAX_SHRINK = 16
NOTE = "Computed (raw + normalized; PSNR/SSIM linear, DeltaEITP/HDR-VDP3 color-managed; DeltaEITP-N normalized pre-PQ{})"
NOTE_CROPPED = "; shared black borders cropped"


# ------------------------------------------------------------------------------------------------------------------ R1
def border_counts(frame):
    """-> (signal pixels per row [H], per column [W]) as uint32."""
    sig = frame.max(axis=2) >= SIGNAL_MIN
    return np.count_nonzero(sig, axis=1).astype(np.uint32), np.count_nonzero(sig, axis=0).astype(np.uint32)


def counts_record(pred, ref):
    """The record hdrtv_rgb48_border_counts writes: u32 [2][H + W]."""
    return np.stack([np.concatenate(border_counts(f)) for f in (pred, ref)])


def bounds_from_counts(rows, cols):
    """gui_objective_metrics.py:344-357 -> (top, bottom, left, right) or None."""
    h, w = len(rows), len(cols)
    row_has = rows >= max(4, int(round(w * 0.01)))
    col_has = cols >= max(4, int(round(h * 0.01)))
    if not row_has.any() or not col_has.any():
        return None
    top, bottom = int(np.argmax(row_has)), h - int(np.argmax(row_has[::-1]))
    left, right = int(np.argmax(col_has)), w - int(np.argmax(col_has[::-1]))
    if bottom - top < 2 or right - left < 2:
        return None
    return top, bottom, left, right


def crop_rect(pred, ref):
    """gui_objective_metrics.py:359-384 -> ((top, bottom, left, right), cropped)."""
    h, w = pred.shape[:2]
    full = (0, h, 0, w)
    bp, br = bounds_from_counts(*border_counts(pred)), bounds_from_counts(*border_counts(ref))
    if bp is None and br is None:
        return full, False
    if bp is None or br is None:
        top, bottom, left, right = br if bp is None else bp
    else:
        top, bottom, left, right = max(bp[0], br[0]), min(bp[1], br[1]), max(bp[2], br[2]), min(bp[3], br[3])
    if max(top, h - bottom, left, w - right) < MIN_BORDER or bottom - top < 2 or right - left < 2:
        return full, False
    return (top, bottom, left, right), True


# ------------------------------------------------------------------------------------------------------------------ R2
def eval_size(h, w, max_side=MAX_SIDE):
    """_prepare_metric_pair's size -> (nh, nw)."""
    if max(h, w) > max_side:
        scale = float(max_side) / float(max(h, w))
        return max(2, int(round(h * scale))), max(2, int(round(w * scale)))
    return h, w


# ------------------------------------------------------------------------------------------------------------------ R3
def area_path(sh, sw, nh, nw):
    """'2x2', 'int' or 'tab': the case of R3 a geometry takes."""
    sx, sy = sw / nw, sh / nh
    eps = np.finfo(np.float64).eps
    if abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps:
        return "2x2" if (round(sx), round(sy)) == (2, 2) else "int"
    return "tab"


def resize_area16(src, nw, nh):
    """oracle.letterbox_oracle.resize_area on 16-bit codes."""
    h, w = src.shape[:2]
    if w > MAX_SHRINK * nw or h > MAX_SHRINK * nh or nw > w or nh > h:
        raise ValueError("not a shrink of at most 16x per axis")
    path = area_path(h, w, nh, nw)
    if path != "tab":
        ix, iy = w // nw, h // nh
        blk = src.reshape(nh, iy, nw, ix, -1).astype(np.int64).sum(axis=(1, 3))
        if path == "2x2":
            return ((blk + 2) >> 2).astype(np.uint16)
        scale = np.float32(1.0) / np.float32(ix * iy)
        return np.clip(_cv_round(blk.astype(np.float32) * scale), 0, 65535).astype(np.uint16)
    xt, yt = area_tab(w, nw), area_tab(h, nh)
    s = src.astype(np.float32)
    buf = np.zeros((h, nw, src.shape[2]), np.float32)
    for dx, sxk, alpha in xt:
        buf[:, dx] = buf[:, dx] + s[:, sxk] * alpha
    out = np.zeros((nh, nw, src.shape[2]), np.float32)
    first = [True] * nh
    for dy, syk, beta in yt:
        if first[dy]:
            out[dy] = beta * buf[syk]
            first[dy] = False
        else:
            out[dy] = out[dy] + beta * buf[syk]
    return np.clip(_cv_round(out), 0, 65535).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------ R4
def unit_planes(frame):
    """_to_unit_float of an RGB48 frame, as the [3][H][W] planes oracle/metrics_oracle.py takes."""
    return np.ascontiguousarray((frame.astype(np.float32) / np.float32(65535.0)).transpose(2, 0, 1))


def raw_metrics(pred, ref, peak_nits=1000.0):
    return M.metrics(unit_planes(pred), unit_planes(ref), peak_nits)


# ------------------------------------------------------------------------------------------------------------------ R5
def abs_of_code(peak_nits):
    """v(c) for every code: float32(clip(float32(c) / 65535, 0, 1) * peak_nits)."""
    c = np.arange(65536, dtype=np.float32)
    return (np.clip(c / np.float32(65535.0), np.float32(0), np.float32(1)) * np.float32(peak_nits)).astype(np.float32)


def channel_hist(frame):
    """-> int64 [3][65536]."""
    return np.stack([np.bincount(frame[:, :, c].ravel(), minlength=65536) for c in range(3)]).astype(np.int64)


def hist_mean_std(h, x):
    """mean and std of the samples a histogram ``h`` counts at values ``x``: float64, ascending code order."""
    h = h.astype(np.float64)
    x = x.astype(np.float64)
    n = float(int(h.sum()))
    mean = np.cumsum(h * x)[-1] / n
    d = x - mean
    return mean, np.sqrt(np.cumsum(h * (d * d))[-1] / n)


def gain_bias(mp, sp, mr, sr):
    gain = 1.0 if sp < 1e-6 else sr / sp
    bias = mr - gain * mp
    return np.float32(gain), np.float32(bias)


def grade_match(pred, ref, peak_nits=1000.0):
    """-> float32 [12]: gain[3], bias[3] on the codes, gain[3], bias[3] on absolute RGB (what hdrtv_rgb48_grade_match returns)."""
    hp, hr = channel_hist(pred), channel_hist(ref)
    out = np.zeros(12, np.float32)
    for dom, x in enumerate((np.arange(65536, dtype=np.float64), abs_of_code(peak_nits))):
        for c in range(3):
            mp, sp = hist_mean_std(hp[c], x)
            mr, sr = hist_mean_std(hr[c], x)
            out[dom * 6 + c], out[dom * 6 + 3 + c] = gain_bias(mp, sp, mr, sr)
    return out


def grade_match_literal(pred, ref, peak_nits=1000.0):
    """The reference's literal text (_grade_normalize_pred_to_ref / _grade_normalize_absolute_rgb_to_ref): float32 np.mean / np.std."""
    out = np.zeros(12, np.float32)
    v = abs_of_code(peak_nits)
    for dom in range(2):
        for c in range(3):
            p = pred[:, :, c].astype(np.float32) if dom == 0 else v[pred[:, :, c]]
            r = ref[:, :, c].astype(np.float32) if dom == 0 else v[ref[:, :, c]]
            out[dom * 6 + c], out[dom * 6 + 3 + c] = gain_bias(float(np.mean(p)), float(np.std(p)), float(np.mean(r)), float(np.std(r)))
    return out


# ------------------------------------------------------------------------------------------------------------------ R6
def normalised_codes(pred, g):
    """trunc(clip(float32(code) * gain + bias, 0, 65535)) per channel, multiply and add separate."""
    p = pred.astype(np.float32)
    out = np.empty_like(p)
    for c in range(3):
        out[:, :, c] = (p[:, :, c] * np.float32(g[c])) + np.float32(g[3 + c])
    return np.clip(out, np.float32(0), np.float32(65535)).astype(np.uint16)


def normalised_metrics(pred, ref, g, peak_nits=1000.0):
    """-> (psnr_norm_db, sssim_norm, delta_e_itp_norm) with the gains / biases ``g`` of grade_match."""
    a, b = unit_planes(normalised_codes(pred, g)), unit_planes(ref)
    v = abs_of_code(peak_nits)
    peak = np.float32(max(1.0, float(peak_nits)))
    pa = np.stack([np.clip(v[pred[:, :, c]] * np.float32(g[6 + c]) + np.float32(g[9 + c]), np.float32(0), peak) for c in range(3)])
    pb = np.stack([np.clip(v[ref[:, :, c]], np.float32(0), peak) for c in range(3)])
    i1, t1, p1 = M.itp(pa.astype(np.float32))
    i2, t2, p2 = M.itp(pb.astype(np.float32))
    de = 720.0 * np.sqrt((i1 - i2) ** 2 + (t1 - t2) ** 2 + (p1 - p2) ** 2 + 1e-12)
    return M.psnr(a, b), M.ssim(a, b), float(np.mean(de, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------ the chain
def evaluation_pair(pred, ref, max_side=MAX_SIDE, crop=True):
    """-> (eval_pred, eval_ref, (top, bottom, left, right), cropped): steps 1 and 2 of _compute_full_reference_metrics."""
    h, w = pred.shape[:2]
    rect, cropped = crop_rect(pred, ref) if crop else ((0, h, 0, w), False)
    t, b, l, r = rect
    p, q = pred[t:b, l:r], ref[t:b, l:r]
    nh, nw = eval_size(b - t, r - l, max_side)
    if (nh, nw) != (b - t, r - l):
        p, q = resize_area16(p, nw, nh), resize_area16(q, nw, nh)
    return np.ascontiguousarray(p), np.ascontiguousarray(q), rect, cropped


def full_reference(pred, ref, max_side=MAX_SIDE, peak_nits=1000.0, crop=True, normalized=True, literal=False):
    """The dict HDRTVNetMI355X.full_reference_metrics returns.  ``literal``: the reference's float32 statistics in place of R5."""
    p, q, rect, cropped = evaluation_pair(pred, ref, max_side, crop)
    out = dict(raw_metrics(p, q, peak_nits))
    out.update(psnr_norm_db=None, sssim_norm=None, delta_e_itp_norm=None)
    if normalized:
        g = (grade_match_literal if literal else grade_match)(p, q, peak_nits)
        out["psnr_norm_db"], out["sssim_norm"], out["delta_e_itp_norm"] = normalised_metrics(p, q, g, peak_nits)
    out["obj_note"] = NOTE.format(NOTE_CROPPED if cropped else "")
    out["crop_rect"] = rect
    out["eval_size"] = p.shape[:2]
    return out


# ------------------------------------------------------------------------------------------------------ the test frames
def ramp_pair(h, w, seed, bars=0, noise=600.0, grade=(0.9, 900.0)):
    """Seeded noise on a smooth ramp: a ground truth and a prediction that is a regraded, noisier copy (so SSIM and the grade match
    have something to do), with ``bars`` black rows at the top and the bottom of both."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([8000 + 40000 * xx / max(w - 1, 1), 6000 + 36000 * yy / max(h - 1, 1),
                     5000 + 20000 * (xx + yy) / max(h + w - 2, 1)], axis=2)
    ref = base + rng.normal(0, noise, base.shape)
    pred = grade[0] * base + grade[1] + rng.normal(0, 1.5 * noise, base.shape)
    ref, pred = (np.clip(np.rint(a), 0, 65535).astype(np.uint16) for a in (ref, pred))
    if bars:
        for a in (ref, pred):
            a[:bars] = 0
            a[h - bars:] = 0
    return pred, ref


# (source H, W, max_side, bars, the path of R3 it exercises): the shapes tests/test_gpu_metrics_full.py holds the device to
GPU_SHAPES = [
    (64, 96, 48, 0, "2x2"),
    (96, 144, 48, 0, "int"),
    (57, 83, 24, 0, "tab"),       # fractional on both axes: 83 -> 24, 57 -> 16
    (51, 96, 48, 0, "tab"),       # mixed: 96 -> 48 exact, 51 -> 26 by half-to-even
    (32, 512, 32, 0, "int"),      # 16x, the limit
    (72, 96, 48, 10, "2x2"),      # 10-row bars in both frames: a crop offset in front of a reduction (52 x 96 -> 26 x 48)
    (75, 99, 40, 10, "tab"),      # the same in front of the table path (55 x 99 -> 22 x 40)
]
