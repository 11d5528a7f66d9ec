"""hdrtv_post_rgb48_scaled, the parts that need no GPU: the facts the resampling rule (include/hdrtv_mi355x.h, restated in
tests/rgb48_scale_ref.py) rests on, the exported symbol, and the host layers that carry the output size."""
import ctypes
import math

import numpy as np
import pytest

import rgb48_scale_ref as R

RATIOS = [(52, 104), (52, 131), (7, 200), (36, 97), (150, 333), (1080, 2160), (1920, 3840), (1280, 3840), (1920, 2560)]


def test_known_coefficients_of_exact_2x_and_3x():
    start, q = R.tab(52, 104)
    assert start[0] == -3 and q[0].tolist() == [121, -1114, 4440, 14628, -2184, 493]
    assert start[1] == -2 and q[1].tolist() == [493, -2184, 14628, 4440, -1114, 121]
    for d in range(104):                                   # two phases, nothing else
        assert q[d].tolist() == q[d % 2].tolist() and start[d] == d // 2 - 3 + (d % 2)
    start, q = R.tab(50, 150)
    assert q[0].tolist() == [208, -1536, 6265, 13336, -2400, 511]
    assert q[1].tolist() == [0, 0, 16384, 0, 0, 0]
    assert q[2].tolist() == [511, -2400, 13336, 6265, -1536, 208]
    for d in range(150):
        assert q[d].tolist() == q[d % 3].tolist()
    assert start[:3].tolist() == [-3, -2, -2]


@pytest.mark.parametrize("n,m", RATIOS)
def test_coefficients_sum_to_one_and_the_horizontal_pass_fits_int32(n, m):
    start, q = R.tab(n, m)
    assert (q.sum(axis=1) == R.ONE).all()
    assert int(np.abs(q).sum(axis=1).max()) * 65535 < 2 ** 31          # |hor| <= 65535 * sum |q|
    assert (np.diff(start) >= 0).all() and (np.diff(start) <= 1).all()   # one output step moves the taps by at most one sample
    assert start[0] >= -3 and start[-1] + 5 <= n + 2
    assert np.abs(q).max() < 32768                                      # the device tables hold them as int16


def test_sum_of_magnitudes_over_a_phase_sweep():
    worst = 0
    for i in range(100000):
        t = i / 100000.0
        w = [R.lanczos3(t - k) for k in range(-2, 4)]
        s = 0.0
        for v in w:
            s += v
        q = [int(math.floor(v / s * R.ONE + 0.5)) for v in w]
        big = max(range(6), key=lambda k: (q[k], -k))
        q[big] += R.ONE - sum(q)
        assert sum(q) == R.ONE
        worst = max(worst, sum(abs(v) for v in q))
    assert worst <= 25290 and worst * 65535 < 2 ** 31


@pytest.mark.parametrize("n", [1, 5, 7, 61, 103])
def test_identity_when_the_sizes_agree(n):
    start, q = R.tab(n, n)
    assert (q == np.array([0, 0, R.ONE, 0, 0, 0])).all() and (start == np.arange(n) - 2).all()
    src = np.random.default_rng(n).integers(0, 65536, (n, n + 3, 3), dtype=np.uint16)
    assert np.array_equal(R.scale(src, n, n + 3), src)


@pytest.mark.parametrize("v", [0, 1, 39977, 65535])
def test_flat_in_flat_out(v):
    src = np.full((5, 7, 3), v, np.uint16)
    assert (R.scale(src, 64, 200) == v).all() and (R.scale(src, 13, 7) == v).all()


def test_step_at_2x_pins_both_clamps():
    src = np.zeros((6, 16, 3), np.uint16)
    src[:, 8:] = 65535                                     # a vertical edge: every row is the same 0 / 65535 step
    out = R.scale(src, 12, 32)
    assert sorted(set(out[0].ravel().tolist())) == [0, 484, 1972, 13788, 51747, 63563, 65051, 65535]
    assert (out == out[0]).all()
    # the ringing lobes overshoot on both sides before the clamp: the unclamped sums leave [0, 65535]
    hor = R.hor_pass(src, 32)
    assert hor.min() < 0 and hor.max() > 65535 * R.ONE


def test_enlarging_only():
    with pytest.raises(ValueError):
        R.tab(8, 7)


def test_library_exports_the_entry_point_and_refuses_a_null_context():
    from hdrtv_mi355x import lib
    for ab in (False, True):
        so = lib.load(ab=ab)
        buf = (ctypes.c_uint16 * 8)()
        assert so.hdrtv_post_rgb48_scaled(None, None, ctypes.addressof(buf), lib.F32, 1, 1, 0, 0.0, ctypes.addressof(buf), 1, 1) == lib.EINVAL
    assert any(n == "hdrtv_post_rgb48_scaled" for n, _, _ in lib.SYMBOLS)


def test_playback_cli_refuses_an_output_size_below_the_processing_size(capsys):
    from hdrtv_mi355x import playback
    for bad in ("32x48", "64x47", "63x48"):
        with pytest.raises(SystemExit) as e:
            playback.main(["--weights-dir", "/nonexistent", "--size", "64x48", "--out-size", bad])
        assert e.value.code == 2
        assert "--out-size" in capsys.readouterr().err


def test_rgb48le_sink_speaks_of_the_size_it_is_given(tmp_path):
    from hdrtv_mi355x.playback import Rgb48leSink
    s = Rgb48leSink(str(tmp_path / "o.raw"), 3840, 2160, 60.0)
    assert "--demuxer-rawvideo-w=3840" in s.mpv_args() and "--demuxer-rawvideo-h=2160" in s.mpv_args()
    assert "3840x2160" in s.ffmpeg_input_args()
    s.close()


def test_sim_dispatcher_delivers_views_at_the_output_size_in_order():
    from hdrtv_mi355x.dispatch import FrameDispatcher, host_sim_worker
    h, w, oh, ow, n = 16, 24, 40, 50, 7
    got = []
    with FrameDispatcher(2, h, w, lambda i, v: got.append((i, v.shape, int(v[0, 0, 0]), int(v[oh - 1, ow - 1, 2]))),
                         make_worker=host_sim_worker, init_args={"device_ms": 0.1}, slots=2, start_timeout=120.0, numa=None,
                         out_height=oh, out_width=ow) as d:
        for i in range(n):
            d.submit(np.full((h, w, 3), i + 1, np.uint8))
        d.flush(timeout=60)
    assert [g[0] for g in got] == list(range(n))
    for i, shape, tag, last in got:
        assert shape == (oh, ow, 3) and tag == (i + 1) * 257 and last == 257 * (i % 2 + 1)       # the stand-in filled the whole slot
    with pytest.raises(ValueError):
        FrameDispatcher(1, h, w, lambda i, v: None, make_worker=host_sim_worker, out_height=h - 1, out_width=w)
