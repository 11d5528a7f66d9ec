"""HDR10 content light level (CTA-861.3 MaxCLL / MaxFALL; x265 ``max-cll=``, HEVC SEI 144) from the per-frame records
``hdrtv_light_stats`` / ``hdrtv_rgb48_light_stats`` leave in device memory (include/hdrtv_mi355x.h states the record and the rule).

Host arithmetic only, in double; no GPU import.  A record is ``LIGHT_WORDS`` = 4104 little-endian u32 words: the 4096-bin
histogram of m = max(R, G, B) >> 4 over the measured rectangle, the largest R, G, B and m, the u64 sum of m and the pixel count.
"""
from __future__ import annotations

import math

import numpy as np

LIGHT_BINS, LIGHT_WORDS = 4096, 4104

# ST.2084 (the constants of gui_objective_metrics.py:486-491)
_M1 = 2610.0 / 16384.0
_M2 = 2523.0 / 32.0
_C1 = 3424.0 / 4096.0
_C2 = 2413.0 / 128.0
_C3 = 2392.0 / 128.0


def pq_nits(code):
    """ST.2084 EOTF of a full-range u16 code (scalar or array): nits(c) = 10000 (max(p - c1, 0) / (c2 - c3 p))^(1/m1) with
    p = (c / 65535)^(1/m2).  nits(0) = 0, nits(65535) = 10000."""
    c = np.asarray(code, dtype=np.float64)
    p = np.power(c / 65535.0, 1.0 / _M2)
    v = 10000.0 * np.power(np.maximum(p - _C1, 0.0) / (_C2 - _C3 * p), 1.0 / _M1)
    return float(v) if v.ndim == 0 else v


_BIN_NITS = None


def bin_nits():
    """nits(16 b + 8), b = 0 .. 4095: the light level a histogram bin stands for (its middle code)."""
    global _BIN_NITS
    if _BIN_NITS is None:
        _BIN_NITS = pq_nits(16 * np.arange(LIGHT_BINS) + 8)
        _BIN_NITS.setflags(write=False)
    return _BIN_NITS


def round_half_up(v):
    """floor(v + 0.5): how MaxCLL / MaxFALL become the integers a container carries."""
    return int(math.floor(float(v) + 0.5))


class FrameLight:
    """One frame's record, parsed.  ``cll`` is exact (the EOTF of the largest code); ``fall`` is the histogram's mean, off the exact
    per-pixel mean by at most the widest deviation inside a bin."""

    def __init__(self, hist, max_rgb, max_code, sum_code, pixels):
        self.hist = hist
        self.max_rgb = tuple(int(v) for v in max_rgb)       # the largest R, G, B code (MaxSCL)
        self.max_code = int(max_code)
        self.sum_code = int(sum_code)
        self.pixels = int(pixels)

    @classmethod
    def from_record(cls, words):
        w = np.asarray(words).astype(np.uint32, copy=False).reshape(-1)
        if w.shape != (LIGHT_WORDS,):
            raise ValueError(f"a light level record has {LIGHT_WORDS} u32 words (got {w.shape})")
        hist = w[:LIGHT_BINS].astype(np.int64)
        pixels = int(w[4102])
        if pixels <= 0 or int(hist.sum()) != pixels:
            raise ValueError(f"malformed light level record: {pixels} pixels, histogram holds {int(hist.sum())}")
        return cls(hist, w[4096:4099], w[4099], int(w[4100]) | (int(w[4101]) << 32), pixels)

    @property
    def cll(self):
        """nits of the brightest pixel's largest channel."""
        return pq_nits(self.max_code)

    @property
    def fall(self):
        """Frame-average light level in nits: sum_b hist[b] nits(16 b + 8) / pixels."""
        return float(np.dot(self.hist.astype(np.float64), bin_nits()) / self.pixels)

    @property
    def mean_code(self):
        return self.sum_code / self.pixels

    def percentile_code(self, p):
        """The code below or at which ``p`` per cent of the pixels lie, at the bin's upper code (16 b + 15), never above the
        frame's largest code; p >= 100 is that largest code itself."""
        p = float(p)
        if not 0.0 < p <= 100.0:
            raise ValueError("percentile must lie in (0, 100]")
        if p >= 100.0:
            return self.max_code
        v = p * self.pixels / 100.0
        need = math.ceil(v - 1e-9 * max(1.0, v))       # 99.9 % of 1000 pixels is 999 of them, not 999.0000000000001 -> 1000
        b = int(np.searchsorted(np.cumsum(self.hist), max(1, need), side="left"))
        return min(16 * b + 15, self.max_code)

    def percentile(self, p):
        """The frame's light level in nits at percentile ``p`` of the histogram: what mastering tools use in place of the
        maximum to ignore a handful of outlier pixels."""
        return pq_nits(self.percentile_code(p))


class ContentLightLevel:
    """Stream totals: MaxCLL = the largest frame CLL, MaxFALL = the largest frame FALL.  ``cll_percentile`` (default 100: the
    maximum) takes each frame's CLL at that percentile of its histogram instead."""

    def __init__(self, cll_percentile=100.0):
        self.cll_percentile = float(cll_percentile)
        if not 0.0 < self.cll_percentile <= 100.0:
            raise ValueError("cll_percentile must lie in (0, 100]")
        self.frames = 0
        self.max_cll = 0.0
        self.max_fall = 0.0
        self.max_rgb = (0, 0, 0)

    def update(self, record):
        """Adds one frame (a record, or a ``FrameLight``); returns its ``FrameLight``."""
        f = record if isinstance(record, FrameLight) else FrameLight.from_record(record)
        self.frames += 1
        self.max_cll = max(self.max_cll, f.percentile(self.cll_percentile))
        self.max_fall = max(self.max_fall, f.fall)
        self.max_rgb = tuple(max(a, b) for a, b in zip(self.max_rgb, f.max_rgb))
        return f

    @property
    def max_cll_int(self):
        return round_half_up(self.max_cll)

    @property
    def max_fall_int(self):
        return round_half_up(self.max_fall)

    def x265_params(self):
        """``max-cll=<MaxCLL>,<MaxFALL>`` for ``ffmpeg -x265-params`` / ``x265 --max-cll``."""
        return f"max-cll={self.max_cll_int},{self.max_fall_int}"

    def as_dict(self):
        return {"frames": self.frames, "max_cll": self.max_cll, "max_fall": self.max_fall, "max_cll_int": self.max_cll_int,
                "max_fall_int": self.max_fall_int, "max_rgb_code": list(self.max_rgb), "cll_percentile": self.cll_percentile,
                "x265_params": self.x265_params()}
