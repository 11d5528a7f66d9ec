"""The tone curves of the delivered frames, on the host in float64: PQ signal in, PQ signal out, and the
``gain[65536]`` float32 table that ``hdrtv_rgb48_tonemap`` / ``hdrtv_post_rgb48_tonemap`` apply (include/hdrtv_mi355x.h states the
pixel rule the device is held to).  No GPU and no library is needed here: numpy alone.

Three curves from a source range ``[source_min, source_peak]`` nits to a target range ``[target_min, target_peak]``; with
``smin, smax, dmin, dmax`` the ST.2084 signals of the four, the input is clamped to ``[smin, smax]`` and the result to ``[dmin, dmax]``:

``"clip"``      ``T(e) = min(e, dmax)``.
``"bt.2390"``   the EETF of Report ITU-R BT.2390: the identity below the knee ``KS = 1.5 maxLum - 0.5`` (normalised signals), a Hermite
                spline from there to ``maxLum``, then the black lift ``E3 = E2 + minLum (1 - E2)^4``.
``"spline"``    the reference's choice (mpv ``tone-mapping=spline``, ``tone-mapping-param=0.45``): a parabola below a knee and a cubic
                above it, meeting with one slope.  This is the library's OWN restatement, modelled on mpv / libplacebo's spline: their
                source is not part of this project, so parity with mpv is UNPINNED (as tests/fs_ref.py says of zimg).  tests/
                test_tonemap_host.py pins the formulas below to a prototype's digits, which is a guard against a transcription error,
                not an outside reference.

Out of scope: desaturation, gamut mapping, an SDR target, and a measured per-scene source peak (mpv's ``hdr-compute-peak``) --
``source_avg`` is the hook for a caller that has scene metadata."""
from __future__ import annotations

import math

import numpy as np

KINDS = ("spline", "bt.2390", "clip")
SOURCE_PEAK = 1000.0                       # the reference's own expectation of the model's output (EXPORT_HDR_TARGET_PEAK_NITS)
SPLINE_PARAM = 0.45                        # the reference's tone-mapping-param

_M1, _M2, _C1, _C2, _C3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875
# the spline's constants
KNEE_ADAPTATION, KNEE_MINIMUM, KNEE_MAXIMUM, KNEE_DEFAULT, SLOPE_TUNING, SLOPE_OFFSET = 0.4, 0.1, 0.8, 0.4, 1.5, 0.2


def pq_oetf(nits):
    """ST.2084: nits -> signal in [0, 1], float64, vectorised."""
    y = np.power(np.asarray(nits, dtype=np.float64) / 10000.0, _M1)
    return np.power((_C1 + _C2 * y) / (1.0 + _C3 * y), _M2)


def pq_eotf(e):
    """ST.2084: signal -> nits, float64, vectorised."""
    t = np.power(np.asarray(e, dtype=np.float64), 1.0 / _M2)
    return 10000.0 * np.power(np.maximum(t - _C1, 0.0) / (_C2 - _C3 * t), 1.0 / _M1)


def _mix(a, b, t):
    return a + (b - a) * t


def _clamp(x, lo, hi):
    return min(max(x, lo), hi)


def _smoothstep(e0, e1, x):
    t = _clamp((x - e0) / (e1 - e0), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def _number(name, v):
    if isinstance(v, (bool, str, bytes)) or v is None:
        raise ValueError(f"{name} must be a number (got {v!r})")
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number (got {v!r})") from None
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite (got {v!r})")
    return v


class ToneCurve:
    """One validated curve: ``.T(e)`` (PQ signal -> PQ signal, float64, vectorised) and ``.gain_table()`` (float32[65536]).
    ``.off``: the target peak is not below the source peak, so nothing is tone-mapped (mpv does not either): ``T`` is the identity
    and the table all ones."""

    def __init__(self, kind, target_peak, source_peak, target_min, source_min, source_avg, param):
        self.kind, self.target_peak, self.source_peak = kind, target_peak, source_peak
        self.target_min, self.source_min, self.source_avg, self.param = target_min, source_min, source_avg, param
        self.off = target_peak >= source_peak
        self.smin, self.smax = float(pq_oetf(source_min)), float(pq_oetf(source_peak))
        self.dmin, self.dmax = float(pq_oetf(target_min)), float(pq_oetf(target_peak))
        if kind == "spline" and not self.off:
            self._spline_setup()

    def _spline_setup(self):
        smin, smax, dmin, dmax = self.smin, self.smax, self.dmin, self.dmax
        sk = float(pq_oetf(self.source_avg)) if self.source_avg is not None else _mix(smin, smax, KNEE_DEFAULT)
        sk = _clamp(sk, _mix(smin, smax, KNEE_MINIMUM), _mix(smin, smax, KNEE_MAXIMUM))
        target = (sk - smin) / (smax - smin)
        adapted = _mix(dmin, dmax, target)
        tuning = 1.0 - _smoothstep(KNEE_MAXIMUM, KNEE_DEFAULT, target) * _smoothstep(KNEE_MINIMUM, KNEE_DEFAULT, target)
        dk = _mix(sk, adapted, _mix(KNEE_ADAPTATION, 1.0, tuning))
        dk = _clamp(dk, _mix(dmin, dmax, KNEE_MINIMUM), _mix(dmin, dmax, KNEE_MAXIMUM))
        slope = (dk - dmin) / (sk - smin)
        ratio = _clamp(SLOPE_TUNING * (self.source_peak / self.target_peak - 1.0), SLOPE_OFFSET, 1.0 + SLOPE_OFFSET)
        slope = slope ** ((1.0 - self.param) * ratio)
        in_min, in_max, out_min, out_max = smin - sk, smax - sk, dmin - dk, dmax - dk
        self.sk, self.dk, self.slope = sk, dk, slope
        self._P = ((out_min - slope * in_min) / (in_min * in_min), slope)
        t = 2.0 * in_max * in_max
        self._Q = ((slope * in_max - out_max) / (in_max * t), -3.0 * (slope * in_max - out_max) / t, slope)

    def T(self, e):
        e = np.asarray(e, dtype=np.float64)
        if self.off:
            return e.copy()
        x = np.clip(e, self.smin, self.smax)
        if self.kind == "clip":
            y = np.minimum(x, self.dmax)
        elif self.kind == "bt.2390":
            span = self.smax - self.smin
            e1 = (x - self.smin) / span
            max_lum, min_lum = (self.dmax - self.smin) / span, (self.dmin - self.smin) / span
            ks = 1.5 * max_lum - 0.5
            t = np.maximum(e1 - ks, 0.0) / (1.0 - ks)
            t2, t3 = t * t, t * t * t
            p = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum
            e2 = np.where(e1 < ks, e1, p)
            e3 = e2 + min_lum * np.power(1.0 - e2, 4)
            y = e3 * span + self.smin
            if min_lum == 0.0:
                y = np.where(e1 < ks, x, y)      # below the knee the curve IS the identity: the signal itself, not its round trip
        else:
            d = x - self.sk
            (pa, pb), (qa, qb, qc) = self._P, self._Q
            y = self.dk + np.where(d > 0, ((qa * d + qb) * d + qc) * d, (pa * d + pb) * d)
        return np.clip(y, self.dmin, self.dmax)

    def gain_table(self):
        """``gain[m] = float32(EOTF(T(m / 65535)) / EOTF(m / 65535))`` for m >= 1, exactly 1 where ``T(e) == e``; ``gain[0] = 1``."""
        gain = np.ones(65536, dtype=np.float32)
        if self.off:
            return gain
        e = np.arange(1, 65536, dtype=np.float64) / 65535.0
        te = self.T(e)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = pq_eotf(te) / pq_eotf(e)
        gain[1:] = np.where(te == e, 1.0, g).astype(np.float32)
        return gain


def tone_curve(kind, target_peak, source_peak=SOURCE_PEAK, target_min=0.0, source_min=0.0, source_avg=None, param=None):
    """The validated ``ToneCurve`` of ``kind`` (one of ``KINDS``) from ``[source_min, source_peak]`` to ``[target_min, target_peak]``
    nits.  ``param``: the spline's contrast in [0, 1] (default ``SPLINE_PARAM``; the other curves take none).  ``source_avg``: the
    scene's average in nits, which places the spline's knee (default: ``KNEE_DEFAULT`` of the source range).  ``target_peak >=
    source_peak`` resolves to off.  ``ValueError``: an unknown kind, a peak that is not finite, a range outside ``0 <= min < peak <=
    10000``, a ``param`` outside [0, 1] or given to another curve, a ``source_avg`` outside the source range."""
    kind = kind.lower() if isinstance(kind, str) else kind
    if kind not in KINDS:
        raise ValueError(f"tone curve must be one of {list(KINDS)} (got {kind!r})")
    target_peak, source_peak = _number("target_peak", target_peak), _number("source_peak", source_peak)
    target_min, source_min = _number("target_min", target_min), _number("source_min", source_min)
    for name, lo, hi in (("target", target_min, target_peak), ("source", source_min, source_peak)):
        if not 0.0 <= lo < hi <= 10000.0:
            raise ValueError(f"{name} range must satisfy 0 <= min < peak <= 10000 nits (got {lo!r} .. {hi!r})")
    if param is None:
        param = SPLINE_PARAM if kind == "spline" else None
    else:
        if kind != "spline":
            raise ValueError(f"param is the spline's contrast: the {kind} curve takes none (got {param!r})")
        param = _number("param", param)
        if not 0.0 <= param <= 1.0:
            raise ValueError(f"param must be in [0, 1] (got {param!r})")
    if source_avg is not None:
        source_avg = _number("source_avg", source_avg)
        if not source_min <= source_avg <= source_peak:
            raise ValueError(f"source_avg must lie in the source range {source_min!r} .. {source_peak!r} (got {source_avg!r})")
    return ToneCurve(kind, target_peak, source_peak, target_min, source_min, source_avg, param)
