"""Output cleanup (deband + ordered dither), the parts that need no GPU: the facts the two rules (include/hdrtv_mi355x.h, restated in
tests/cleanup_ref.py) state about themselves, and the argument checks of every layer that carries the cleanup -- lib.output_cleanup,
the worker, the dispatcher, the playback command line and the C entry points' refusals that return before any device call."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import cleanup_ref as K
import ycbcr10_ref as R

COMBOS = [(f, s) for f in R.FORMATS for s in R.SITINGS if not (f == "yuv422p10le" and s == "topleft")]
CORNERS = [(r, g, b) for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)]


# ---------------------------------------------------------------------------------------------------------------- Bayer index
def test_bayer_formula_is_the_recursive_matrix_and_a_permutation():
    y, x = np.mgrid[0:16, 0:16]
    m = K.bayer_index(x, y)
    assert np.array_equal(m, K.bayer_recursive(16))
    assert sorted(m.reshape(-1).tolist()) == list(range(256))
    assert m[0, 0] == 0 and m[0, 1] == 128 and m[1, 0] == 192 and m[1, 1] == 64          # [[0, 2], [3, 1]] * 64
    yy, xx = np.mgrid[0:48, 0:80]                                                          # period 16 in both axes
    assert np.array_equal(K.bayer_index(xx, yy), np.tile(m, (3, 5)))
    assert ((2 * m + 1) << 11).sum() == 256 << 19                                          # the mean of t is exactly 2^19


# ---------------------------------------------------------------------------------------------------------------- dither
def test_block_mean_of_dithered_luma_is_within_1_512_code_of_the_unrounded_value():
    rng = np.random.default_rng(0)
    worst = 0.0
    for k in range(200):
        c = rng.integers(0, 65536, 3).astype(np.uint16)
        frame = np.tile(c, (32, 48, 1))
        y = K.luma(frame, 1).astype(np.float64)
        want = 64.0 + K.luma_sum(c) / 2.0 ** 20
        for by in range(2):
            for bx in range(3):
                worst = max(worst, abs(y[16 * by:16 * by + 16, 16 * bx:16 * bx + 16].mean() - want))
        # the integer sum is the exact formula apart from the coefficients' own rounding: at most 1.5 * 65535 / 2^20 code
        assert abs(want - R.exact(c)[0]) <= 1.5 * 65535 / 2.0 ** 20
    print("worst |block mean of dithered Y - (64 + sum / 2^20)| = %.6f code" % worst)
    assert worst <= 1.0 / 512


@pytest.mark.parametrize("fmt,siting", COMBOS)
def test_dithered_outputs_stay_in_range_for_the_cube_corners(fmt, siting):
    shift = 6 if fmt == "p010le" else 0
    for c in CORNERS:
        frame = np.tile(np.array(c, np.uint16), (32, 32, 1))
        y, cb, cr = K.planes(frame, fmt, siting, 1)
        assert not any((p & ((1 << shift) - 1)).any() for p in (y, cb, cr))
        y, cb, cr = y >> shift, cb >> shift, cr >> shift
        assert y.min() >= 64 and y.max() <= 940, (c, int(y.min()), int(y.max()))
        assert min(cb.min(), cr.min()) >= 64 and max(cb.max(), cr.max()) <= 960, c
        if c[0] == c[1] == c[2]:                                  # grey: the chroma sums are zero, the threshold never reaches a code
            assert (cb == 512).all() and (cr == 512).all()
    # a sharp pattern of the corners, odd rows and columns differing: the taps mix them, the bounds hold
    rng = np.random.default_rng(3)
    frame = np.array(CORNERS, np.uint16)[rng.integers(0, 8, (32, 48))]
    y, cb, cr = (p >> shift for p in K.planes(frame, fmt, siting, 1))
    assert y.min() >= 64 and y.max() <= 940 and min(cb.min(), cr.min()) >= 64 and max(cb.max(), cr.max()) <= 960


@pytest.mark.parametrize("fmt,siting", COMBOS)
def test_dither_0_is_the_undithered_rule(fmt, siting):
    rgb = np.random.default_rng(11).integers(0, 65536, (18, 34, 3)).astype(np.uint16)
    assert np.array_equal(K.pack(rgb, fmt, siting, 0), R.pack(rgb, fmt, siting))
    d = K.pack(rgb, fmt, siting, 1)
    assert d.shape == R.pack(rgb, fmt, siting).shape and not np.array_equal(d, R.pack(rgb, fmt, siting))
    # dithering moves a sample by at most one code
    sh = 6 if fmt == "p010le" else 0
    assert np.abs((d >> sh).astype(int) - (R.pack(rgb, fmt, siting) >> sh).astype(int)).max() == 1


# ---------------------------------------------------------------------------------------------------------------- deband
def test_deband_staircase_smooths_the_steps_and_keeps_the_line():
    f, line = K.staircase()
    out = K.deband(f)
    assert out.dtype == np.uint16 and out.shape == f.shape
    assert np.array_equal(out[line], f[line])                    # the line's pixels
    touched = np.zeros(line.shape, bool)                         # every pixel with a reference on the line
    for ys, xs in K.deband_refs(*line.shape):
        touched |= line[ys, xs]
    assert touched.sum() > line.sum()
    assert np.array_equal(out[touched], f[touched])
    changed = (out != f).any(axis=2)
    print("staircase: %.1f %% of the pixels change, distinct codes %d -> %d" % (100 * changed.mean(), len(np.unique(f[..., 0])),
                                                                             len(np.unique(out[..., 0]))))
    assert changed.mean() > 0.40
    assert len(np.unique(f[..., 0])) == 17 and len(np.unique(out[..., 0])) > 17
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()      # grey stays grey


def test_deband_offsets_stay_in_reach_and_follow_the_seed():
    for rng in (1, 5, 16):
        dx, dy = K.deband_offsets(40, 60, rng, 0)
        assert dx.min() == -rng and dx.max() == rng and dy.min() == -rng and dy.max() == rng
    a, b = K.deband_offsets(40, 60, 16, 0), K.deband_offsets(40, 60, 16, 7)
    assert not np.array_equal(a[0], b[0])
    assert np.array_equal(a[0], K.deband_offsets(40, 60, 16, 0)[0])                       # fixed: the same in every frame
    # x = 0, y = 0, S = 0 hashes 0 to 0: dx = dy = -R
    assert K.deband_offsets(1, 1, 16, 0)[0][0, 0] == -16 and K.deband_offsets(1, 1, 16, 0)[1][0, 0] == -16


def test_deband_leaves_noise_a_single_pixel_and_hue_alone():
    r = np.random.default_rng(1).integers(0, 65536, (64, 96, 3)).astype(np.uint16)       # P(a pixel passes) < 1e-15 at T = 1311
    assert np.array_equal(K.deband(r), r)
    one = np.array([[[123, 45678, 65535]]], np.uint16)
    assert np.array_equal(K.deband(one), one) and np.array_equal(K.deband(one, 1, 65535, 9), one)
    # all or nothing across the channels: a step in ONE channel beyond the threshold keeps all three
    f = np.full((40, 40, 3), 30000, np.uint16)
    f[:, 20:, 2] = 40000
    out = K.deband(f)
    assert np.array_equal(out, f)
    f[:, 20:, 2] = 30600                                           # within the threshold: blue is smoothed, red and green have nothing to do
    out = K.deband(f)
    assert (out[..., :2] == 30000).all() and (out[..., 2] != f[..., 2]).any()
    with pytest.raises(ValueError):
        K.deband(f, 17)
    with pytest.raises(ValueError):
        K.deband(f, 16, 0)


def test_header_states_both_rules():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdrtv_mi355x.h")).read()
    for v in ("0x9E3779B9", "0x7feb352d", "0x846ca68b", "1311", "hdrtv_rgb48_deband", "hdrtv_post_ycbcr10_ex", "hdrtv_rgb48_to_ycbcr10_ex",
              "HDRTV_DITHER_ORDERED", "7 - 2i", "6 - 2i", "tests/cleanup_ref.py"):
        assert v in text, v
    assert re.search(r"#define HDRTV_DITHER_NONE 0\b", text) and re.search(r"#define HDRTV_DITHER_ORDERED 1\b", text)


# ---------------------------------------------------------------------------------------------------------------- validation
BAD_CLEANUP = [dict(deband_range=0), dict(deband_range=17), dict(deband_range=-1), dict(deband_range=2.5), dict(deband_range="8"),
               dict(deband_threshold=0), dict(deband_threshold=65536), dict(deband_threshold=-5), dict(deband_threshold=None),
               dict(dither="bayer"), dict(dither="error_diffusion"), dict(dither=1), dict(dither=None), dict(deband="yes"), dict(deband=2)]


def test_output_cleanup_constructor_and_pickle():
    from hdrtv_mi355x import lib as L
    c = L.output_cleanup()
    assert tuple(c) == (False, 16, 1311, "none") and not c.active and c.dither_code == L.DITHER_NONE
    assert c._fields == ("deband", "deband_range", "deband_threshold", "dither")
    c = L.output_cleanup(True, 1, 65535, "Ordered", pix_fmt="p010le")
    assert tuple(c) == (True, 1, 65535, "ordered") and c.active and c.dither_code == L.DITHER_ORDERED
    assert L.output_cleanup(deband=True).active and L.output_cleanup(dither="ordered").active
    assert L.output_cleanup(True, pix_fmt="rgb48le") == (True, 16, 1311, "none")          # deband alone goes with rgb48le
    back = pickle.loads(pickle.dumps(c))
    assert back == c and isinstance(back, L.OutputCleanup) and back.active and back.dither_code == 1
    assert L.OutputCleanup(*tuple(c)) == c                                                # what the dispatcher's worker rebuilds
    for bad in BAD_CLEANUP:
        with pytest.raises(ValueError):
            L.output_cleanup(**bad)
    with pytest.raises(ValueError):
        L.output_cleanup(dither="ordered", pix_fmt="rgb48le")
    # OutputFormat keeps its four fields: the cleanup travels beside it
    assert L.OutputFormat._fields == ("pix_fmt", "siting", "h", "w")
    names = {n for n, _, _ in L.SYMBOLS}
    assert {"hdrtv_rgb48_deband", "hdrtv_post_ycbcr10_ex", "hdrtv_rgb48_to_ycbcr10_ex"} <= names


def test_worker_refuses_every_bad_value(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, **kw)      # noqa: E731
    w = mk(out_pix_fmt="p010le", deband=True, deband_range=8, deband_threshold=500, dither="ordered")
    assert tuple(w._cleanup) == (True, 8, 500, "ordered")
    assert not mk()._cleanup.active and tuple(mk()._cleanup) == (False, 16, 1311, "none")
    assert mk(deband=True)._cleanup.active                                                   # rgb48le with deband alone
    for bad in BAD_CLEANUP:
        with pytest.raises(ValueError):
            mk(out_pix_fmt="p010le", **bad)
    with pytest.raises(ValueError):
        mk(dither="ordered")                                                                 # rgb48le is not dithered
    with pytest.raises(ValueError):
        mk(out_pix_fmt="rgb48le", deband=True, dither="ordered")


def _cleanup_echo_worker(rank, device_index, init_args):
    c = init_args.get("cleanup")

    def process(frame, out):
        out[...] = 0
        if c is not None:
            out.flat[0], out.flat[1], out.flat[2], out.flat[3] = int(c[0]), c[1], c[2], 1 if c[3] == "ordered" else 0
            out.flat[4] = 1 if type(c) is tuple else 2
        else:
            out.flat[4] = 7
    return process


def test_dispatcher_validates_and_hands_the_tuple_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    h, w = 6, 10
    for bad in BAD_CLEANUP:
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, make_worker=_cleanup_echo_worker, numa=False, out_pix_fmt="p010le", **bad)
    with pytest.raises(ValueError):
        D.FrameDispatcher(1, h, w, lambda i, v: None, make_worker=_cleanup_echo_worker, numa=False, dither="ordered")
    got = {}
    with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=_cleanup_echo_worker, slots=2, numa=False,
                           out_pix_fmt="yuv420p10le", deband=True, deband_range=4, deband_threshold=900, dither="ordered") as d:
        assert d._out_b == h * w * 3 and tuple(d.cleanup) == (True, 4, 900, "ordered")      # the slot size does not change
        d.submit(np.zeros((h, w, 3), np.uint8))
        d.flush(timeout=60)
    assert d.exit_codes == [0] and got[0][:5].tolist() == [1, 4, 900, 1, 1]
    got.clear()
    with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=_cleanup_echo_worker, slots=2,
                           numa=False) as d:                                                # off: init_args stay as they were
        assert d._out_b == h * w * 6 and not d.cleanup.active
        d.submit(np.zeros((h, w, 3), np.uint8))
        d.flush(timeout=60)
    assert d.exit_codes == [0] and got[0].reshape(-1)[4] == 7


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    a = P.parse_args(base)
    assert tuple(a.cleanup) == (False, 16, 1311, "none") and a.proc_wh == (96, 64) and a.out_wh == (96, 64)
    a = P.parse_args(base + ["--out-pix-fmt", "p010le", "--deband", "--deband-range", "7", "--deband-threshold", "2000", "--dither", "ordered"])
    assert tuple(a.cleanup) == (True, 7, 2000, "ordered")
    assert tuple(P.parse_args(base + ["--deband"]).cleanup) == (True, 16, 1311, "none")      # rgb48le, deband alone
    bad = [["--dither", "ordered"], ["--out-pix-fmt", "rgb48le", "--dither", "ordered"], ["--out-pix-fmt", "p010le", "--dither", "bayer"],
           ["--deband-range", "0"], ["--deband-range", "17"], ["--deband-range", "x"], ["--deband-threshold", "0"],
           ["--deband-threshold", "65536"], ["--deband-threshold", "1.5"], ["--deband", "--deband-range", "-3"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(base + extra)
        assert e.value.code == 2, extra


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    P, P420 = lib.YCC_P010, lib.YCC_YUV420P10
    # a NULL context is refused whatever else is given
    assert so.hdrtv_rgb48_deband(None, None, a, 2, 4, 16, 1311, 0, a + 96) == lib.EINVAL
    for dither in (0, 1, 2, -1):
        assert so.hdrtv_post_ycbcr10_ex(None, None, a, lib.F32, 2, 4, 0, 0.0, P, 0, a, 8, a + 32, None, 8, dither) == lib.EINVAL
        assert so.hdrtv_rgb48_to_ycbcr10_ex(None, None, a, 2, 4, P420, 0, a, 8, a + 32, a + 48, 4, dither) == lib.EINVAL
    assert all(x == 0xA5A5 for x in buf)
