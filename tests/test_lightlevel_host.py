"""HDR10 content light level, host side (no GPU): the ST.2084 EOTF, the record parser and the MaxCLL / MaxFALL accumulator of
hdrtv_mi355x/lightlevel.py, and tests/lightlevel_ref.py (the numpy restatement the GPU tests use) against a per-pixel loop."""
import math

import numpy as np
import pytest

import lightlevel_ref as R
from hdrtv_mi355x import lib as L
from hdrtv_mi355x import lightlevel as LL


def _record(max_code, hist_bins, max_rgb=None, sum_code=None):
    """A hand-built record: hist_bins = {bin: count}."""
    w = np.zeros(LL.LIGHT_WORDS, dtype=np.uint32)
    for b, n in hist_bins.items():
        w[b] = n
    w[4096:4099] = max_rgb if max_rgb is not None else (max_code, 0, 0)
    w[4099] = max_code
    s = sum_code if sum_code is not None else sum((16 * b + 8) * n for b, n in hist_bins.items())
    w[4100], w[4101] = s & 0xFFFFFFFF, s >> 32
    w[4102] = sum(hist_bins.values())
    return w


def test_constants_agree_with_the_library_binding():
    assert (LL.LIGHT_BINS, LL.LIGHT_WORDS) == (L.LIGHT_BINS, L.LIGHT_WORDS) == (R.BINS, R.WORDS) == (4096, 4104)
    names = [s[0] for s in L.SYMBOLS]
    assert "hdrtv_light_stats" in names and "hdrtv_rgb48_light_stats" in names


def test_eotf_known_answers():
    assert LL.pq_nits(0) == 0.0
    assert LL.pq_nits(65535) == 10000.0
    assert abs(LL.pq_nits(33297) - 100.0012) < 1e-3
    assert abs(LL.pq_nits(49271) - 1000.0) < 0.3
    # array form, monotonic over every code
    t = LL.pq_nits(np.arange(65536))
    assert t.shape == (65536,) and t[0] == 0.0 and t[-1] == 10000.0 and np.all(np.diff(t) >= 0.0)
    # against the ST.2084 OETF in double: the round trip returns the code
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 32, 3424 / 4096, 2413 / 128, 2392 / 128
    for c in (1, 4096, 33297, 49271, 65000):
        y = (LL.pq_nits(c) / 10000.0) ** m1
        assert abs(((c1 + c2 * y) / (1 + c3 * y)) ** m2 * 65535 - c) < 1e-6


def test_record_parser():
    rec = _record(50000, {0: 10, 3125: 5}, max_rgb=(50000, 41000, 7), sum_code=5 * 50000 + 3)
    f = LL.FrameLight.from_record(rec)
    assert f.pixels == 15 and f.max_rgb == (50000, 41000, 7) and f.max_code == 50000
    assert f.cll == LL.pq_nits(50000)
    assert f.fall == pytest.approx((10 * LL.pq_nits(8) + 5 * LL.pq_nits(16 * 3125 + 8)) / 15, rel=1e-12)
    assert f.mean_code == (5 * 50000 + 3) / 15
    assert f.hist.shape == (4096,) and int(f.hist.sum()) == 15
    # the u64 sum: both words
    big = _record(65535, {4095: 70000}, sum_code=70000 * 65535)
    assert 70000 * 65535 > 2 ** 32 and LL.FrameLight.from_record(big).mean_code == 65535.0
    # a list is taken as well; wrong lengths and inconsistent histograms are refused
    assert LL.FrameLight.from_record([int(v) for v in rec]).pixels == 15
    with pytest.raises(ValueError):
        LL.FrameLight.from_record(rec[:-1])
    bad = rec.copy()
    bad[4102] = 16
    with pytest.raises(ValueError):
        LL.FrameLight.from_record(bad)
    with pytest.raises(ValueError):
        LL.FrameLight.from_record(np.zeros(LL.LIGHT_WORDS, dtype=np.uint32))


def test_percentile_takes_the_upper_code_of_the_bin():
    # 990 pixels in bin 100, 9 in bin 2000, 1 outlier at code 60001 (bin 3750)
    f = LL.FrameLight.from_record(_record(60001, {100: 990, 2000: 9, 3750: 1}))
    assert f.percentile_code(100) == 60001 and f.percentile(100) == f.cll
    assert f.percentile_code(99.95) == 60001                      # the upper code of bin 3750 is 60015: never above the maximum
    assert f.percentile_code(99.9) == 16 * 2000 + 15              # ceil(999.0) = 999 pixels: the last of bin 2000
    assert f.percentile_code(99.0) == 16 * 100 + 15
    assert f.percentile_code(50) == 16 * 100 + 15
    assert f.percentile(99.9) == LL.pq_nits(32015)
    for p in (0, -1, 100.5):
        with pytest.raises(ValueError):
            f.percentile_code(p)


def test_accumulator_max_over_frames_rounding_and_string():
    cl = LL.ContentLightLevel()
    assert cl.frames == 0 and cl.max_cll == 0.0 and cl.max_fall == 0.0 and cl.x265_params() == "max-cll=0,0"
    assert cl.as_dict()["frames"] == 0
    a = _record(49271, {3079: 100})                               # about 1000 nits peak, flat
    b = _record(33297, {2081: 50, 0: 50})                         # 100 nits peak, half black
    c = _record(40000, {2500: 1, 10: 99})
    fa = cl.update(a)
    cl.update(b)
    fc = cl.update(LL.FrameLight.from_record(c))                  # a parsed frame is taken as it is
    assert cl.frames == 3
    assert cl.max_cll == fa.cll == LL.pq_nits(49271)
    assert cl.max_fall == fa.fall == pytest.approx(LL.pq_nits(16 * 3079 + 8))
    assert fc.fall < fa.fall and cl.max_rgb == (49271, 0, 0)
    assert cl.max_cll_int == math.floor(cl.max_cll + 0.5) == 1000
    assert cl.x265_params() == "max-cll=%d,%d" % (cl.max_cll_int, cl.max_fall_int)
    d = cl.as_dict()
    assert d["max_cll"] == cl.max_cll and d["max_fall"] == cl.max_fall and d["x265_params"] == cl.x265_params() and d["frames"] == 3
    # MaxCLL and MaxFALL may come from different frames
    cl2 = LL.ContentLightLevel()
    cl2.update(_record(65535, {4095: 1, 0: 999}))                 # one 10000-nit pixel in black
    cl2.update(_record(33297, {2081: 1000}))                      # flat 100 nits
    assert cl2.max_cll == 10000.0 and 99.0 < cl2.max_fall < 101.0
    assert cl2.x265_params() == "max-cll=10000,100"
    assert LL.round_half_up(0.5) == 1 and LL.round_half_up(0.49) == 0 and LL.round_half_up(399.5) == 400


def test_accumulator_percentile_ignores_outliers():
    rec = _record(65535, {4095: 1, 2081: 9999})
    full, p999 = LL.ContentLightLevel(), LL.ContentLightLevel(cll_percentile=99.9)
    full.update(rec)
    p999.update(rec)
    assert full.max_cll == 10000.0
    assert p999.max_cll == LL.pq_nits(16 * 2081 + 15) and p999.max_fall == full.max_fall
    with pytest.raises(ValueError):
        LL.ContentLightLevel(cll_percentile=0)


def test_ref_equals_a_per_pixel_loop_on_5x7():
    rng = np.random.default_rng(57)
    a = rng.integers(0, 65536, (5, 7, 3), dtype=np.uint16)
    a[0, 0] = (0, 0, 0)
    a[4, 6] = (65535, 1, 2)
    for rect in (None, (0, 0, 7, 5), (1, 2, 3, 2), (6, 4, 1, 1), (3, 0, 4, 5)):
        got, want = R.record(a, rect), R.record_loop(a.tolist(), rect)
        assert got.dtype == np.uint32 and got.shape == (R.WORDS,) and np.array_equal(got, want), rect
        assert int(got[:R.BINS].sum()) == got[4102] and got[4103] == 0
    one = R.record(a, (6, 4, 1, 1))
    assert tuple(one[4096:4100]) == (65535, 1, 2, 65535) and one[4095] == 1 and one[4100] == 65535


@pytest.mark.parametrize("seed,kind", [(0, "uniform"), (1, "dark"), (2, "bright"), (3, "two-level")])
def test_histogram_fall_within_the_bound_the_table_gives(seed, kind):
    """FALL from the histogram vs the exact per-pixel mean of nits(m).  Every pixel's error is at most the widest deviation inside
    its own bin, dev[b] = max over the bin's 16 codes of |nits(c) - nits(16 b + 8)|; so the frame's error is at most
    sum(hist * dev) / pixels, and never more than max(dev).  Both bounds come from the EOTF table, none from a measured frame."""
    table = LL.pq_nits(np.arange(65536))
    mid = LL.bin_nits()
    assert np.array_equal(mid, table[8::16])
    dev = np.abs(table.reshape(4096, 16) - mid[:, None]).max(axis=1)
    worst = float(dev.max())
    assert worst == float(np.abs(table - mid[np.arange(65536) >> 4]).max()) and 5.0 < worst < 20.0     # the top bin: about 11.6 nits
    rng = np.random.default_rng(seed)
    h, w = 48, 64
    if kind == "uniform":
        a = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
    elif kind == "dark":
        a = rng.integers(0, 20000, (h, w, 3), dtype=np.uint16)
    elif kind == "bright":
        a = rng.integers(60000, 65536, (h, w, 3), dtype=np.uint16)
    else:
        a = np.where(rng.random((h, w, 1)) < 0.1, 65535, 33297).astype(np.uint16).repeat(3, axis=2)
    f = LL.FrameLight.from_record(R.record(a))
    m = a.max(axis=2).astype(np.int64)
    exact = float(table[m].mean())
    frame_bound = float((f.hist * dev).sum() / f.pixels)
    err = abs(f.fall - exact)
    assert err <= frame_bound * (1 + 1e-9) + 1e-9 <= worst * (1 + 1e-9) + 1e-9, (err, frame_bound, worst)
    assert f.cll == table[m.max()] and f.mean_code == m.mean()
