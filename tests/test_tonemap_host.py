"""The tone map without a GPU: the rule's ``lin`` table (hdrtv_pq_eotf_table), the three host curves of hdrtv_mi355x/tonemap.py and
their gain tables, the pixel rule (tests/tonemap_ref.py) on grey pixels, and every place that validates the options -- lib, worker,
dispatcher, command line, and the library's argument checks that need no device."""
import ctypes
import pickle

import numpy as np
import pytest

import tonemap_ref as R

F = np.float32
KINDS = ("spline", "bt.2390", "clip")
TARGETS = (600.0, 203.0)
E = np.arange(65536, dtype=np.float64) / 65535.0


@pytest.fixture(scope="module")
def lin():
    return R.lin_table()


@pytest.fixture(scope="module")
def curves():
    from hdrtv_mi355x import tonemap as T
    return {(k, t): T.tone_curve(k, t) for k in KINDS for t in TARGETS}


def test_lin_round_trips_every_code_and_is_monotone(lin):
    assert lin.dtype == F and lin.shape == (65536,)
    assert np.array_equal(R.code(lin), np.arange(65536))
    assert (np.diff(lin) >= 0).all()
    assert lin[0] == 0 and lin[65535] == 1
    # and it IS the EOTF, to float32: the repair moves an entry by a few steps of the grid at most
    from hdrtv_mi355x import tonemap as T
    want = T.pq_eotf(E[1:]) / 10000.0
    assert np.abs(lin[1:].astype(np.float64) / want - 1.0).max() < 1e-6


def test_all_ones_is_the_identity_on_every_code(lin):
    c = np.arange(65536, dtype=np.uint16).reshape(256, 256, 1).repeat(3, 2)
    c[:, :, 1], c[:, :, 2] = c[::-1, :, 1].copy(), c[:, ::-1, 2].copy()
    assert np.array_equal(R.apply(c, np.ones(65536, F), lin), c)


def test_every_curve_is_monotone_and_maps_peak_to_peak(curves):
    for key, c in curves.items():
        t = c.T(E)
        assert (np.diff(t) >= 0).all(), key
        assert abs(float(c.T(c.smax)) - c.dmax) <= 1e-9, key
        assert abs(float(c.T(1.0)) - c.dmax) <= 1e-9, key                 # above the source peak: clamped
        assert t.min() >= c.dmin and t.max() <= c.dmax, key
        g = c.gain_table()
        assert g.dtype == F and g.shape == (65536,) and np.isfinite(g).all() and g[0] == 1 and (g > 0).all() and (g <= 1).all(), key
        assert (g[1:][t[1:] == E[1:]] == 1).all(), key                      # exactly 1.0f wherever T(e) == e
        assert (g[1:][t[1:] < E[1:] - 1e-6] < 1).all(), key                 # and below it where the curve rolls off
    assert (curves["clip", 600.0].gain_table() == 1).sum() > 40000 and (curves["bt.2390", 600.0].gain_table() == 1).sum() > 40000


def test_a_target_at_or_above_the_source_is_off():
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import tonemap as T
    for k in KINDS:
        for target, source in ((1000.0, 1000.0), (4000.0, 1000.0), (600.0, 600.0), (601.0, 600.0)):
            c = T.tone_curve(k, target, source)
            assert c.off and np.array_equal(c.T(E), E) and (c.gain_table() == 1).all(), (k, target, source)
            assert L.tone_mapping(k, target, source) is None
        assert not T.tone_curve(k, 999.0).off and L.tone_mapping(k, 999.0) is not None
    assert L.tone_mapping(None) is None and L.tone_mapping("none", "anything") is None and L.tone_mapping("NONE") is None


def test_bt2390_follows_the_report():
    """Report ITU-R BT.2390, EETF: with signals normalised by the source range, KS = 1.5 maxLum - 0.5; below KS the identity, at
    E1 = 1 the Hermite spline gives maxLum.  1000 -> 600 nits: 100 nits lies below the knee and stays, 1000 nits lands on 600."""
    from hdrtv_mi355x import tonemap as T
    c = T.tone_curve("bt.2390", 600.0)
    smin, smax, dmax = float(T.pq_oetf(0.0)), float(T.pq_oetf(1000.0)), float(T.pq_oetf(600.0))
    ks = 1.5 * (dmax - smin) / (smax - smin) - 0.5
    e100 = float(T.pq_oetf(100.0))
    assert (e100 - smin) / (smax - smin) < ks
    assert float(c.T(e100)) == e100 and abs(float(T.pq_eotf(c.T(e100))) - 100.0) < 1e-9
    assert abs(float(T.pq_eotf(c.T(smax))) - 600.0) < 1e-6
    # just above the knee the curve bends below the identity, and it is continuous there
    knee = smin + ks * (smax - smin)
    assert float(c.T(knee + 1e-3)) < knee + 1e-3 and abs(float(c.T(knee + 1e-9)) - float(c.T(knee - 1e-9))) < 1e-8
    # the black lift: E3 = E2 + minLum (1 - E2)^4 puts the source's black on the target's
    lifted = T.tone_curve("bt.2390", 600.0, target_min=0.05)
    assert abs(float(lifted.T(lifted.smin)) - lifted.dmin) < 1e-9 and abs(float(lifted.T(lifted.smax)) - lifted.dmax) < 1e-9
    assert (np.diff(lifted.T(E)) >= 0).all()


def test_spline_matches_the_prototype_digits_and_meets_with_one_slope():
    from hdrtv_mi355x import tonemap as T
    c = T.tone_curve("spline", 600.0)
    assert c.param == 0.45 == T.SPLINE_PARAM
    assert round(c.sk, 4) == 0.3007 and round(c.dk, 4) == 0.2918 and round(c.slope, 4) == 0.9836
    nits = lambda n: float(T.pq_eotf(c.T(T.pq_oetf(n))))               # noqa: E731
    assert round(nits(100.0), 2) == 79.52 and round(nits(18.0), 2) == 15.94 and round(nits(1000.0), 3) == 600.0
    d = T.tone_curve("spline", 203.0)
    assert round(d.dk, 4) == 0.2733 and round(d.slope, 4) == 0.9389
    for cv in (c, d, T.tone_curve("spline", 400.0, param=0.0), T.tone_curve("spline", 400.0, param=1.0),
               T.tone_curve("spline", 600.0, source_avg=40.0)):
        h = 1e-6
        at, lo, hi = float(cv.T(cv.sk)), float(cv.T(cv.sk - h)), float(cv.T(cv.sk + h))
        assert abs(at - cv.dk) < 1e-12                                      # the knee maps to the knee
        assert abs(hi - at) < 2e-6 and abs(at - lo) < 2e-6                  # continuous
        assert abs((at - lo) / h - cv.slope) < 1e-4 and abs((hi - at) / h - cv.slope) < 1e-4, (cv.target_peak, cv.param)
        assert abs(float(cv.T(cv.smin)) - cv.dmin) < 1e-9 and abs(float(cv.T(cv.smax)) - cv.dmax) < 1e-9
        assert (np.diff(cv.T(E)) >= 0).all()
    # source_avg places the knee (within its limits), param = 1 leaves the slope at 1
    assert abs(T.tone_curve("spline", 600.0, source_avg=40.0).sk - float(T.pq_oetf(40.0))) < 1e-12
    assert T.tone_curve("spline", 400.0, param=1.0).slope == 1.0


def test_the_rule_on_grey_pixels_follows_the_curve(lin, curves):
    """For every curve and every m >= 1 the rule on (m, m, m) gives a code within 1 of round(65535 T(m / 65535))."""
    m = np.arange(1, 65536)
    grey = m.astype(np.uint16).reshape(-1, 1, 1).repeat(3, 2)
    for key, c in curves.items():
        got = R.apply(grey, c.gain_table(), lin)
        assert (got[:, :, 0] == got[:, :, 1]).all() and (got[:, :, 0] == got[:, :, 2]).all()
        want = np.floor(65535.0 * c.T(E[1:]) + 0.5).astype(np.int64)
        err = np.abs(got[:, 0, 0].astype(np.int64) - want)
        print(key, "largest distance in codes:", int(err.max()), "codes off by one:", int((err == 1).sum()))
        assert err.max() <= 1, key
        assert got.max() <= np.floor(65535.0 * c.dmax + 0.5) + 1, key


def test_clip_above_the_frame_changes_nothing(lin):
    from hdrtv_mi355x import tonemap as T
    rng = np.random.default_rng(5)
    top = int(np.floor(65535.0 * float(T.pq_oetf(600.0))))                  # every code at or below 600 nits
    frame = rng.integers(0, top + 1, (33, 47, 3)).astype(np.uint16)
    frame[0, 0] = top
    gain = T.tone_curve("clip", 600.0).gain_table()
    assert np.array_equal(R.apply(frame, gain, lin), frame)
    frame[1, 1] = (65535, 100, 7)                                           # one pixel above: only that pixel moves
    out = R.apply(frame, gain, lin)
    assert (out != frame).any(axis=2).sum() == 1 and out[1, 1, 0] in (top, top + 1) and out[1, 1, 1] < 100


BAD = [dict(kind="hable", target_peak=600), dict(kind=None, target_peak=600), dict(kind="spline", target_peak=float("nan")),
       dict(kind="spline", target_peak=float("inf")), dict(kind="spline", target_peak=600, source_peak=float("inf")),
       dict(kind="spline", target_peak=600, source_peak=float("nan")), dict(kind="spline", target_peak=0), dict(kind="spline", target_peak=-5),
       dict(kind="spline", target_peak="600"), dict(kind="spline", target_peak=True), dict(kind="spline", target_peak=None),
       dict(kind="spline", target_peak=600, source_peak=10001), dict(kind="spline", target_peak=20000, source_peak=30000),
       dict(kind="spline", target_peak=600, target_min=600), dict(kind="spline", target_peak=600, target_min=-0.1),
       dict(kind="spline", target_peak=600, source_min=1000), dict(kind="spline", target_peak=600, source_min=-1),
       dict(kind="spline", target_peak=600, param=-0.1), dict(kind="spline", target_peak=600, param=1.01),
       dict(kind="spline", target_peak=600, param=float("nan")), dict(kind="spline", target_peak=600, param="0.45"),
       dict(kind="clip", target_peak=600, param=0.45), dict(kind="bt.2390", target_peak=600, param=0.45),
       dict(kind="spline", target_peak=600, source_avg=2000), dict(kind="spline", target_peak=600, source_avg=float("nan"))]


def test_every_value_error():
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import tonemap as T
    for kw in BAD:
        with pytest.raises(ValueError):
            T.tone_curve(**kw)
        if kw["kind"] is not None:
            with pytest.raises(ValueError):
                L.tone_mapping(**kw)
    with pytest.raises(ValueError, match="target_peak"):
        L.tone_mapping("spline")
    t = L.tone_mapping("Spline", 600)
    assert t == L.ToneMapping("spline", 600.0, 1000.0, 0.0, 0.0, None, 0.45) and hash(t) == hash(L.tone_mapping("spline", 600.0))
    assert pickle.loads(pickle.dumps(t)) == t and L.tone_mapping(*tuple(t)) == t      # a plain tuple: it crosses a process boundary
    assert L.tone_mapping("clip", 203).param is None
    assert np.array_equal(t.gain_table(), T.tone_curve("spline", 600).gain_table())


def test_worker_validates(tmp_path):
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, **kw)      # noqa: E731
    assert mk()._tone is None and mk(tone_mapping="none", target_peak=600)._tone is None
    assert mk(tone_mapping="spline", target_peak=1000)._tone is None                            # nothing to roll off
    assert mk(tone_mapping="spline", target_peak=600)._tone == L.tone_mapping("spline", 600)
    assert mk(tone_mapping="spline", target_peak=600, tone_param=0.3, source_peak=4000)._tone == L.tone_mapping("spline", 600, 4000, param=0.3)
    assert mk(tone_mapping="bt.2390", target_peak=203, out_pix_fmt="p010le", deband=True, light_stats=True)._tone.kind == "bt.2390"
    for kw in (dict(tone_mapping="spline"), dict(tone_mapping="hable", target_peak=600), dict(tone_mapping="spline", target_peak=-1),
               dict(tone_mapping="spline", target_peak=600, tone_param=2), dict(tone_mapping="clip", target_peak=600, tone_param=0.5),
               dict(tone_mapping="spline", target_peak=600, source_peak=float("nan"))):
        with pytest.raises(ValueError):
            mk(**kw)


def _echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    tone = [init_args.get(k, "absent") for k in ("tone_mapping", "target_peak", "source_peak", "tone_param")]

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = 9999 if tone[0] == "absent" else ("spline", "bt.2390", "clip").index(tone[0])
        out.flat[2] = 9999 if tone[1] == "absent" else int(tone[1])
        out.flat[3] = 9999 if tone[2] == "absent" else int(tone[2])
        out.flat[4] = 9999 if tone[3] in ("absent", None) else int(round(tone[3] * 100))
    return process


def test_dispatcher_validates_and_hands_the_curve_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    from hdrtv_mi355x import lib as L
    h, w = 6, 10
    run = dict(make_worker=_echo_worker, slots=2, numa=False)
    for kw in (dict(tone_mapping="spline"), dict(tone_mapping="reinhard", target_peak=600), dict(tone_mapping="spline", target_peak=0),
               dict(tone_mapping="spline", target_peak=600, tone_param=-1)):
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, **run, **kw)
    off = [1, 9999, 9999, 9999, 9999]                                       # off: init_args keep their keys
    for kw, want in (({}, off), ({"tone_mapping": "none", "target_peak": 600}, off), ({"tone_mapping": "spline", "target_peak": 1000}, off),
                     ({"tone_mapping": "spline", "target_peak": 600}, [5, 0, 600, 1000, 45]),
                     ({"tone_mapping": "clip", "target_peak": 203, "source_peak": 4000}, [5, 2, 203, 4000, 9999])):
        got = {}
        with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **kw, **run) as d:
            assert d.tone == L.tone_mapping(kw.get("tone_mapping"), kw.get("target_peak"), kw.get("source_peak", 1000.0))
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:5].tolist() == want, kw


def test_playback_command_line():
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    assert P.parse_args(base).tone is None and P.parse_args(base + ["--tone-mapping", "none"]).tone is None
    assert P.parse_args(base + ["--tone-mapping", "spline", "--target-peak", "600"]).tone == L.tone_mapping("spline", 600)
    assert P.parse_args(base + ["--tone-mapping", "spline", "--target-peak", "1000"]).tone is None
    a = P.parse_args(base + ["--tone-mapping", "spline", "--target-peak", "400", "--source-peak", "4000", "--tone-mapping-param", "0.3"])
    assert a.tone == L.tone_mapping("spline", 400, 4000, param=0.3)
    a = P.parse_args(base + ["--out-size", "192x128", "--tone-mapping", "bt.2390", "--target-peak", "203", "--out-pix-fmt", "p010le",
                             "--film-grain", "1", "--light-level"])
    assert a.tone.kind == "bt.2390" and a.tone.target_peak == 203.0
    assert P.parse_args(base + ["--tone-mapping", "clip", "--target-peak", "600", "--deband"]).tone.kind == "clip"
    bad = [base + ["--tone-mapping", "spline"], base + ["--target-peak", "600"], base + ["--tone-mapping-param", "0.3"],
           base + ["--tone-mapping", "none", "--target-peak", "600"], base + ["--tone-mapping", "hable", "--target-peak", "600"],
           base + ["--tone-mapping", "spline", "--target-peak", "0"], base + ["--tone-mapping", "spline", "--target-peak", "nan"],
           base + ["--tone-mapping", "spline", "--target-peak", "600", "--tone-mapping-param", "1.5"],
           base + ["--tone-mapping", "clip", "--target-peak", "600", "--tone-mapping-param", "0.3"],
           base + ["--tone-mapping", "spline", "--target-peak", "600", "--source-peak", "20000"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(argv)
        assert e.value.code == 2, argv


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    assert so.hdrtv_pq_eotf_table(None) == lib.EINVAL
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    assert so.hdrtv_rgb48_tonemap(None, None, a, 1, 1, a, a) == lib.EINVAL          # a NULL context is refused whatever else is given
    assert so.hdrtv_post_rgb48_tonemap(None, None, a, lib.F32, 1, 1, 0, 0.0, a, a) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)
