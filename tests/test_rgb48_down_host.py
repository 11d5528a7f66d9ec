"""The shrinking rule of hdrtv_post_rgb48_down on the host: the tables and the content behaviour of tests/rgb48_down_ref.py, its float32
stage against a float64 evaluation of the same formulas, and the Python surface that carries the downscaler (option checkers, the
playback command line, the worker's and the dispatcher's validation).  tests/test_gpu_rgb48_down.py holds the device to the same
reference bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import rgb48_down_ref as D

U = 2.0 ** -24                  # the unit roundoff of float32


def gamma(n):
    """The standard bound on the relative error of n chained float32 roundings."""
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------- tables
PAIRS = [(8, 4), (9, 3), (16, 4), (12, 8), (101, 37), (34, 33), (41, 11), (64, 53), (3840, 2560), (2160, 1440), (2160, 1080), (2160, 540),
         (4, 1), (3, 1), (2, 1), (1, 1), (7, 7)]


@pytest.mark.parametrize("n,m", PAIRS, ids=lambda v: str(v))
def test_tables(n, m):
    t = D.tab(n, m)
    nt = t.q.shape[1]
    assert t.lo.shape == t.cnt.shape == t.k2.shape == (m,) and t.w.shape == (m, nt) and t.w.dtype == np.float32
    assert (t.q.sum(axis=1) == D.ONE).all()
    assert 1 <= t.cnt.min() and t.cnt.max() == nt <= 4 * n // m + 1 <= D.MAX_TAPS == 17
    assert np.abs(t.q).max() < 32768                                                   # every coefficient fits int16
    assert int(np.abs(t.q).sum(axis=1).max()) * 65535 < 2 ** 31                        # the horizontal sum fits int32 for any codes
    for d in range(m):                                                                  # zero padding behind the last tap
        assert not t.q[d, t.cnt[d]:].any() and not t.w[d, t.cnt[d]:].any()
    if m == n:
        assert nt == 1 and (t.lo == np.arange(m)).all() and (t.k2 == np.arange(m)).all() and (t.q == D.ONE).all() and (t.w == 1).all()
        return
    assert (np.diff(t.lo) >= 0).all() and (np.diff(t.lo + t.cnt) >= 0).all()           # both ends of the footprint rise with d
    assert (t.lo <= t.k2).all() and (t.k2 + 1 <= t.lo + t.cnt - 1).all()               # the bracketing samples are taps
    assert np.allclose(t.w.sum(axis=1), 1.0, atol=nt * U)
    for d in range(m):                                                                  # the footprint formulas, restated
        ctr = (d + 0.5) * n / m
        assert t.lo[d] == math.ceil(ctr - 2 * n / m - 0.5) and t.lo[d] + t.cnt[d] - 1 == math.floor(ctr + 2 * n / m - 0.5)
        assert t.k2[d] == math.floor(ctr - 0.5)
    if n % m == 0:                                                                      # an exact ratio: one row of coefficients
        r = n // m
        assert (t.q == t.q[0]).all() and (t.w == t.w[0]).all() and (np.diff(t.lo) == r).all()


def test_tables_refuse_enlarging_and_more_than_4x():
    for n, m in ((8, 9), (9, 2), (0, 0), (4, 0), (100, 24)):
        with pytest.raises(ValueError):
            D.tab(n, m)
    assert D.tab(100, 25).cnt.max() == 16 and D.tab(9, 3).cnt.max() == 13
    assert D.mitchell_w(0.0) == 16.0 / 18.0 and D.mitchell_w(2.0) == 0.0 and abs(D.mitchell_w(1.0) - 1.0 / 18.0) < 1e-15
    assert D.catrom_w(0.0) == 1.0 and D.catrom_w(1.0) == 0.0 and D.catrom_w(2.0) == 0.0


def test_horizontal_sum_fits_int32_on_the_worst_frames():
    rng = np.random.default_rng(5)
    for (h, w), (dh, dw) in (((41, 43), (11, 11)), ((34, 71), (33, 70)), ((64, 96), (32, 48))):
        for x in (rng.integers(0, 2, (h, w, 3)).astype(np.uint16) * 65535, rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)):
            for a in (0, 51, 256):
                p = D.passes(x, dh, dw, a)
                assert np.abs(p["raw_h"]).max() < 2 ** 31 and np.abs(p["hor"]).max() < 2 ** 31 and np.abs(p["v"]).max() < 2 ** 62


# --------------------------------------------------------------------------------------------------------------- content
def test_a_flat_frame_returns_its_code():
    for code in (0, 1, 32768, 65535):
        x = np.full((41, 43, 3), code, np.uint16)
        for dh, dw in ((11, 11), (20, 43), (40, 22), (41, 43)):
            for a in (0, 51, 256):
                for ssim in (False, True):
                    assert (D.scale(x, dh, dw, a, ssim) == code).all(), (code, dh, dw, a, ssim)


def test_equal_sizes_return_the_codes_and_bad_sizes_raise():
    x = np.random.default_rng(1).integers(0, 65536, (12, 20, 3)).astype(np.uint16)
    assert np.array_equal(D.scale(x, 12, 20, 51, True), x)
    for dh, dw in ((13, 20), (12, 21), (13, 10), (6, 21), (2, 20), (12, 4), (0, 20)):
        with pytest.raises(ValueError):
            D.scale(x, dh, dw)
    assert D.scale(x, 3, 5, 0, True).shape == (3, 5, 3)


def _step(h=24, w=64):
    x = np.full((h, w, 3), 16384, np.uint16)                  # the 0.25 / 0.75 step along x
    x[:, w // 2:] = 49151
    return x


def test_antiringing_removes_the_overshoot_of_the_step():
    x = _step()
    over = {}
    for a in (0, 51, 128, 256):
        y = D.mitchell(x, 24, 27, a).astype(int)
        over[a] = max(int(y.max()) - 49151, 0) + max(16384 - int(y.min()), 0)
    print("overshoot of the 0.25 / 0.75 step by strength:", over)
    assert over[0] > over[51] > over[128] > over[256] == 0
    lo, hi = x.min(), x.max()
    assert D.mitchell(x, 9, 27, 256).min() >= lo and D.mitchell(x, 9, 27, 256).max() <= hi


def _local_variance(img):
    v = img.astype(np.float64) / 65535.0
    m = sum(v[1 + dy:v.shape[0] - 1 + dy, 1 + dx:v.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    q = sum(v[1 + dy:v.shape[0] - 1 + dy, 1 + dx:v.shape[1] - 1 + dx] ** 2 for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return float((q - m * m).mean())


def test_ssim_differs_from_mitchell_and_restores_local_variance_on_a_fine_texture():
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 65536, (72, 104, 3)).astype(np.uint16)
    assert not np.array_equal(D.scale(noise, 36, 52), D.scale(noise, 36, 52, 0, True))
    texture = (32768 + 12000 * rng.standard_normal((96, 128, 1)) * np.ones((1, 1, 3))).clip(0, 65535).astype(np.uint16)
    for dh, dw in ((48, 64), (64, 85), (32, 43)):
        mit, ss = D.scale(texture, dh, dw), D.scale(texture, dh, dw, 0, True)
        vm, vs = _local_variance(mit), _local_variance(ss)
        print(f"{dh}x{dw}: local variance mitchell {vm:.6f}, ssim {vs:.6f}, source {_local_variance(texture):.6f}")
        assert vs > vm


# ------------------------------------------------------------------------------------------- float32 stage against float64
def _tab64(n, m):
    """The L2 weights in double (no rounding to float32) on the footprint of D.tab."""
    t = D.tab(n, m)
    w = np.zeros(t.w.shape, np.float64)
    for d in range(m):
        if m == n:
            w[d, 0] = 1.0
            continue
        c = [D.catrom_w(x) for x in D.footprint(n, m, d)[3]]
        w[d, :len(c)] = np.array(c) / sum(c)
    return t, w


def _l2_64(codes, dh, dw):
    s = codes.astype(np.float64) / 65535.0
    h, w = s.shape[:2]
    (ty, wy), (tx, wx) = _tab64(h, dh), _tab64(w, dw)
    v1 = sum(wy[:, k].reshape(dh, 1, 1) * (s * s)[np.clip(ty.lo + k, 0, h - 1)] for k in range(wy.shape[1]))
    return sum(wx[:, k].reshape(1, dw, 1) * v1[:, np.clip(tx.lo + k, 0, w - 1)] for k in range(wx.shape[1]))


def _l2_bound(h, w, dh, dw):
    """|l2 float32 - l2 float64| from the tap counts T and the largest absolute weight sums A of the two axes.  Pass 1: a term
    wy * (s * s) carries 5 roundings (the weight, the sample, the square's two factors share the sample's: 1 + 2 + 1, the product)
    and at most T1 - 1 additions, on terms of magnitude <= |wy|: e1 = gamma(T1 + 5) A1.  Pass 2: its input is off by e1 and of
    magnitude <= A1 + e1; a term carries the weight's and the product's rounding and T2 - 1 additions."""
    (ty, wy), (tx, wx) = _tab64(h, dh), _tab64(w, dw)
    a1, a2 = float(np.abs(wy).sum(axis=1).max()), float(np.abs(wx).sum(axis=1).max())
    t1, t2 = int(ty.cnt.max()), int(tx.cnt.max())
    e1 = gamma(t1 + 5) * a1
    return a2 * e1 + gamma(t2 + 2) * a2 * (a1 + e1), a1 * a2


def _mean3_64(v):
    h, w = v.shape[:2]
    xm, xp = np.clip(np.arange(w) - 1, 0, w - 1), np.clip(np.arange(w) + 1, 0, w - 1)
    ym, yp = np.clip(np.arange(h) - 1, 0, h - 1), np.clip(np.arange(h) + 1, 0, h - 1)
    r = (0.5 * v[:, xm] + v + 0.5 * v[:, xp]) / 2
    return (0.5 * r[ym] + r + 0.5 * r[yp]) / 2


def _ssim_64(codes, mcodes, dh, dw, e_l2, l2max):
    """The final pass in float64 and, per value, a bound on what float32 may differ by, propagated from e_l2 (see _l2_bound), the unit
    roundoff and the values themselves.  mean3 halves exactly and adds four times: mean3(v) is off by mean3(e_v) + 4 U max|v|."""
    luma = lambda c: 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]      # noqa: E731
    sigma = 10.0 / (255.0 * 255.0)
    ms = mcodes.astype(np.float64) / 65535.0                                           # float32: one rounding, e = U
    mm, mq, ml = _mean3_64(ms), _mean3_64(ms * ms), _mean3_64(_l2_64(codes, dh, dw))
    e_mm, e_mq, e_ml = 5 * U, 3 * U + 4 * U, e_l2 + 4 * U * l2max
    e_sq = 2 * e_mm + e_mm ** 2 + U * 1.01                                             # mM * mM
    sl, sh = luma(np.maximum(mq - mm * mm, 0)), luma(np.maximum(ml - mm * mm, 0))
    # the difference (one rounding on a value <= 1 or l2max), then luma: three constants, three products, two additions
    e_sl = (e_mq + e_sq + U) * 1.0 + 6 * U * 1.01
    e_sh = (e_ml + e_sq + U * l2max) * 1.0 + 6 * U * l2max * 1.01
    r1 = np.clip(sh / np.maximum(sl, 1e-300), 0, 1)
    r2 = np.sqrt((sh + sigma) / (sl + sigma))
    r = np.where(sl > sh, r1, r2)
    # ratio branch: |d(sh / sl)| <= (e_sh + r1 e_sl) / (sl - e_sl), never more than 1 after the clamp, plus the division's rounding
    d1 = np.minimum((e_sh + r1 * e_sl) / np.maximum(sl - e_sl, 1e-300), 1.0) + U
    d1 = np.where(sl - e_sl > 0, d1, 1.0)
    # root branch: relative error x of the quotient (numerator, denominator, the two additions, the division), sqrt halves it
    x = (e_sh + U * (sh + sigma)) / (sh + sigma) + (e_sl + U * (sl + sigma)) / (sl + sigma) + U
    x = x / (1 - x)
    d2 = r2 * (x / (2 * (1 - x)) + U) * 1.01
    e_r = np.where(sl > sh, d1, d2)
    e_r = e_r + np.where(np.abs(sl - sh) <= e_sl + e_sh, np.abs(r1 - r2) + d1 + d2, 0.0)      # float32 may take the other branch
    rmax = float((r + e_r).max())
    e_rm = e_r[..., None] * mm + (r[..., None] + e_r[..., None]) * e_mm + U * (r[..., None] + e_r[..., None]) * 1.01      # R * mM
    a0, a1, a2 = _mean3_64(r[..., None] * mm), _mean3_64(mm), _mean3_64(r)
    e_a0 = _mean3_64(e_rm) + 4 * U * rmax * 1.01
    e_a1 = e_mm + 4 * U * 1.01
    e_a2 = _mean3_64(e_r) + 4 * U * rmax
    pix = (a1 + a2[..., None] * ms) - a0
    t = np.abs(a2[..., None] * ms)
    e_pix = (e_a1 + e_a2[..., None] * ms + (a2 + e_a2)[..., None] * U + U * (t + e_a2[..., None]) + e_a0
             + U * (np.abs(a1) + t + 1e-3) + U * (np.abs(pix) + 1e-3))
    return np.clip(pix, 0, 1), e_pix


@pytest.mark.parametrize("src,dst", [((40, 56), (17, 23)), ((36, 52), (18, 26)), ((33, 41), (9, 11)), ((24, 40), (24, 13))], ids=str)
def test_float32_stage_against_float64(src, dst):
    (h, w), (dh, dw) = src, dst
    rng = np.random.default_rng(h * w)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = {
        "noise": rng.integers(0, 65536, (h, w, 3)).astype(np.uint16),
        "texture": (30000 + 9000 * rng.standard_normal((h, w, 3))).clip(0, 65535).astype(np.uint16),
        "step": _step(h, w),
        "ramp": np.broadcast_to(((xx * 65535) // max(w - 1, 1)).astype(np.uint16)[..., None], (h, w, 3)).copy(),
        "dark": rng.integers(0, 4, (h, w, 3)).astype(np.uint16),
    }
    e_l2, l2max = _l2_bound(h, w, dh, dw)
    print(f"{src} -> {dst}: |l2 - float64| <= {e_l2:.3e}")
    assert e_l2 < 1e-5                                                        # the derivation gives a few units of 2^-24 per tap
    for name, x in frames.items():
        got, want = D.l2(x, dh, dw).astype(np.float64), _l2_64(x, dh, dw)
        err = float(np.abs(got - want).max())
        print(f"  {name}: l2 off by {err:.3e}")
        assert err <= e_l2, name
        for a in (0, 51):
            m = D.mitchell(x, dh, dw, a)
            pix, e_pix = _ssim_64(x, m, dh, dw, e_l2, l2max * (1 + 1e-6) + e_l2)
            code64 = pix * 65535.0
            bound = np.ceil(65535.0 * e_pix + 65535.0 * U * 2) + 1                # the quantiser's product and addition, then one code of rounding
            diff = np.abs(D.ssim(x, m, dh, dw).astype(np.float64) - np.floor(code64 + 0.5))
            print(f"  {name} a={a}: ssim off by at most {int(diff.max())} codes, bound {int(bound.min())} .. {int(bound.max())}")
            assert (diff <= bound).all(), (name, a)


# -------------------------------------------------------------------------------------------------------- Python surface
def test_option_checkers():
    from hdrtv_mi355x import lib as L
    assert L.DOWNSCALERS == ("mitchell", "ssim") and L.DOWN_MAX_RATIO == 4 and L.DOWN_ANTIRING == 0.20
    assert L.check_downscaler() is None and L.check_downscaler(None) is None
    assert L.check_downscaler("mitchell") == "mitchell" and L.check_downscaler("SSIM") == "ssim"
    for v in ("", "lanczos", "fsr", "area", True, 1, 0.5, b"ssim", ["ssim"]):
        with pytest.raises(ValueError):
            L.check_downscaler(v)
    assert L.check_down_antiring() == 0.0 and L.check_down_antiring("auto") == 0.20 and L.check_down_antiring("AUTO") == 0.20
    assert L.check_down_antiring(1) == 1.0 and L.antiring_code(L.check_down_antiring("auto")) == D.AUTO_ANTIRING == 51
    for v in (True, "strong", None, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            L.check_down_antiring(v)
    for ok in ((3840, 2160, 2560, 1440), (3840, 2160, 1920, 1080), (3840, 2160, 960, 540), (96, 64, 96, 32), (96, 64, 48, 64), (41, 43, 11, 11)):
        L.check_down_size(*ok)
    for bad, what in (((96, 64, 97, 32), "one axis up"), ((96, 64, 48, 65), "one axis up"), ((96, 64, 192, 128), "enlarging"),
                      ((96, 64, 23, 64), "4x"), ((96, 64, 96, 15), "4x"), ((41, 43, 10, 11), "4x"), ((96, 64, 96, 64), "equals"),
                      ((96, 64, 0, 32), "positive")):
        with pytest.raises(ValueError, match=what):
            L.check_down_size(*bad)
    sizes = (96, 64, 48, 32)
    assert L.down_options(None, 0.0, *sizes) is None and L.down_options(None, "auto", 96, 64, 192, 128) is None
    assert L.down_options("mitchell", 0.0, *sizes) == (0, 0) and L.down_options("ssim", "auto", *sizes) == (51, 1)
    assert L.down_options("SSIM", 1.0, *sizes, "lanczos", "auto", "auto") == (256, 1) and L.down_options("ssim", 0.5, *sizes, "Lanczos", 0, 0.0) == (128, 1)
    for args in (("ssim", 0.0, *sizes, "fsr"), ("ssim", 0.0, *sizes, "lanczos", 0.3), ("ssim", 0.0, *sizes, "lanczos", 0.0, 0.2),
                 ("ssim", 0.0, 96, 64, 96, 64), ("ssim", 0.0, 96, 64, 192, 128), ("ssim", 0.0, 96, 64, 100, 32), ("ssim", 0.0, 96, 64, 23, 32),
                 ("ssim", 2.0, *sizes), ("bicubic", 0.0, *sizes), (None, 0.3, *sizes), ("ssim", 0.0, *sizes, "ewa")):
        with pytest.raises(ValueError):
            L.down_options(*args)


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "192x128"]
    small = base + ["--out-size", "96x64"]
    a = P.parse_args(base)
    assert (a.downscaler, a.down_antiring) == (None, 0.0)                                        # off by default
    a = P.parse_args(small + ["--downscaler", "ssim"])
    assert (a.downscaler, a.down_antiring, a.out_wh, a.scaler, a.antiring, a.cas) == ("ssim", 0.0, (96, 64), "lanczos", 0.0, 0.0)
    assert P.parse_args(small + ["--downscaler", "mitchell", "--down-antiring", "auto"]).down_antiring == 0.20
    assert P.parse_args(small + ["--downscaler", "ssim", "--down-antiring", "AUTO"]).down_antiring == 0.20
    assert P.parse_args(small + ["--downscaler", "ssim", "--down-antiring", "1"]).down_antiring == 1.0
    assert P.parse_args(small + ["--downscaler", "ssim", "--antiring", "auto", "--cas", "auto"]).downscaler == "ssim"
    assert P.parse_args(base + ["--out-size", "192x64", "--downscaler", "ssim"]).out_wh == (192, 64)      # one axis at identity still shrinks
    assert P.parse_args(base + ["--out-size", "48x32", "--downscaler", "mitchell"]).out_wh == (48, 32)     # exactly 4x
    bad = [small, small + ["--scaler", "fsr"], small + ["--antiring", "auto"],                    # as before: a smaller size is refused
           base + ["--downscaler", "ssim"], base + ["--out-size", "192x128", "--downscaler", "ssim"],     # nothing to shrink
           base + ["--out-size", "384x256", "--downscaler", "ssim"],                              # enlarging
           base + ["--out-size", "96x129", "--downscaler", "ssim"], base + ["--out-size", "193x64", "--downscaler", "ssim"],      # mixed
           base + ["--out-size", "47x64", "--downscaler", "ssim"], base + ["--out-size", "96x31", "--downscaler", "ssim"],        # more than 4x
           small + ["--downscaler", "ssim", "--scaler", "fsr"], small + ["--downscaler", "ssim", "--cas", "0.2"],
           small + ["--downscaler", "ssim", "--antiring", "0.3"], small + ["--downscaler", "ssim", "--fsr-sharpness", "0.2"],
           small + ["--downscaler", "ssim", "--down-antiring", "1.5"], small + ["--downscaler", "ssim", "--down-antiring", "-0.1"],
           small + ["--downscaler", "ssim", "--down-antiring", "nan"], small + ["--downscaler", "ssim", "--down-antiring", "strong"],
           small + ["--downscaler", "ssim", "--down-antiring", ""], small + ["--down-antiring", "0.2"],      # belongs to --downscaler
           base + ["--down-antiring", "auto"], small + ["--downscaler", "lanczos"], small + ["--downscaler", "SSIM"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(argv)
        assert e.value.code == 2, argv


def test_worker_validates(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=192, proc_h=128, **{"out_w": 96, "out_h": 64, **kw})      # noqa: E731
    wk = mk(downscaler="ssim")
    assert (wk._downscaler, wk._down_antiring, wk._out.w, wk._out.h) == ("ssim", 0.0, 96, 64)
    assert mk(downscaler="MITCHELL", down_antiring="auto", antiring="auto", cas="auto")._downscaler == "mitchell"
    assert mk(downscaler="ssim", out_w=192, out_pix_fmt="p010le")._out.pix_fmt == "p010le"
    wk = mk()                                             # no downscaler: constructed as before, the smaller size refused per frame
    assert wk._downscaler is None
    for kw in (dict(downscaler="area"), dict(downscaler=True), dict(downscaler="ssim", scaler="fsr"), dict(downscaler="ssim", cas=0.2),
               dict(downscaler="ssim", antiring=0.3), dict(downscaler="ssim", down_antiring=2), dict(downscaler="ssim", down_antiring="x"),
               dict(downscaler="ssim", out_w=192, out_h=128), dict(downscaler="ssim", out_w=193), dict(downscaler="ssim", out_w=384, out_h=256),
               dict(downscaler="ssim", out_w=47), dict(downscaler="ssim", out_h=31), dict(down_antiring=0.2)):
        with pytest.raises(ValueError):
            mk(**kw)


def _echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    s, v = init_args.get("downscaler"), init_args.get("down_antiring", "absent")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = 7 if s is None else 1 if s == "ssim" else 2
        out.flat[2] = 9999 if v == "absent" else int(round(float(v) * 1000))
        out.flat[3] = 1 if "scaler" in keys or "cas" in keys or "antiring" in keys else 0
    return process


def test_dispatcher_validates_and_hands_the_downscaler_to_its_workers():
    from hdrtv_mi355x import dispatch as Dp
    h, w = 12, 20
    run = dict(make_worker=_echo_worker, slots=2, numa=False, out_height=6, out_width=10)
    for kw in (dict(), dict(downscaler=None), dict(scaler="fsr"), dict(antiring="auto"),           # as before: a smaller size raises
               dict(downscaler="area"), dict(downscaler=1), dict(downscaler="ssim", scaler="fsr"), dict(downscaler="ssim", cas=0.2),
               dict(downscaler="ssim", antiring=0.3), dict(downscaler="ssim", down_antiring=1.5), dict(downscaler="ssim", down_antiring="x"),
               dict(downscaler="ssim", out_width=21), dict(downscaler="ssim", out_height=12, out_width=20), dict(downscaler="ssim", out_width=4),
               dict(downscaler="ssim", out_height=2), dict(downscaler="ssim", out_height=24, out_width=40), dict(down_antiring=0.2)):
        with pytest.raises(ValueError):
            Dp.FrameDispatcher(1, h, w, lambda i, v: None, **{**run, **kw})
    for kw, want in (({"downscaler": "ssim"}, [3, 1, 0, 0]), ({"downscaler": "SSIM", "down_antiring": "auto"}, [3, 1, 200, 0]),
                     ({"downscaler": "mitchell", "down_antiring": 0.5, "cas": "auto", "antiring": "auto"}, [3, 2, 500, 0]),
                     ({"downscaler": "ssim", "out_height": 12}, [3, 1, 0, 0])):
        got = {}
        with Dp.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **{**run, **kw}) as d:
            assert d.downscaler == kw["downscaler"].lower() and d._out_b == kw.get("out_height", 6) * 10 * 6
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:4].tolist() == want, kw
    got = {}                                              # without a downscaler the init_args keep their keys
    with Dp.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, make_worker=_echo_worker, slots=2,
                            numa=False) as d:
        assert d.downscaler is None and d.down_antiring == 0.0
        d.submit(np.zeros((h, w, 3), np.uint8))
        d.flush(timeout=60)
    assert got[0].reshape(-1)[:4].tolist() == [1, 7, 9999, 0]


def test_dispatcher_delivers_shrunk_slots_with_the_host_stand_in():
    from hdrtv_mi355x import dispatch as Dp
    h, w, oh, ow = 16, 24, 8, 12
    got = {}
    with Dp.FrameDispatcher(2, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=Dp.host_sim_worker, init_args={"device_ms": 1.0},
                            slots=2, numa=False, out_height=oh, out_width=ow, downscaler="ssim", down_antiring="auto") as d:
        assert (d.downscaler, d.down_antiring, d.out_h, d.out_w) == ("ssim", 0.20, oh, ow)
        for i in range(4):
            d.submit(np.full((h, w, 3), i + 1, np.uint8))
        d.flush(timeout=60)
    assert d.exit_codes == [0, 0] and sorted(got) == [0, 1, 2, 3]
    for i in range(4):
        assert got[i].shape == (oh, ow, 3) and got[i].reshape(-1)[0] == (i + 1) * 257


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    for ar in (0, 51, 257, -1):            # a NULL context is refused whatever else is given
        for ssim in (0, 1, 2):
            assert so.hdrtv_post_rgb48_down(None, None, a, lib.F32, 4, 4, 0, 0.0, a, 2, 2, ar, ssim) == lib.EINVAL
    assert so.hdrtv_post_rgb48_down(None, None, a, lib.F32, 4, 4, 0, 0.0, a, 5, 2, 0, 0) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)          # bad arguments with a live context: tests/test_gpu_rgb48_down.py
