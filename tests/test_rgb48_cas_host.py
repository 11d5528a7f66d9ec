"""Contrast-adaptive sharpening in front of the fused Lanczos upscale (hdrtv_post_rgb48_scaled_cas), the parts that need no GPU:
the facts the integer rule (include/hdrtv_mi355x.h step 1s, restated in tests/rgb48_cas_ref.py) states about itself, the CAS code
and the reference's schedule (lib.cas_code, lib.scale_cas), and the argument checks of every layer that carries the strength --
the worker, the dispatcher, the playback command line, the C entry point's refusals that return before any device call."""
import ctypes
import os

import numpy as np
import pytest

import rgb48_antiring_ref as A
import rgb48_cas_ref as C
import rgb48_scale_ref as S

CODES = (1032, 3426, 3486, 3605, 4084, 4096)


def _checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((yy + xx) & 1) * 65535).astype(np.uint16)[..., None], (h, w, 3)).copy()


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_flat_and_single_pixel_frames_are_returned_unchanged():
    for K in CODES:
        for v in (0, 1, 777, 39977, 65534, 65535):
            for shape in ((1, 1, 3), (1, 9, 3), (7, 1, 3), (6, 11, 3)):
                x = np.full(shape, v, np.uint16)
                assert np.array_equal(C.sharpen(x, K), x), (K, v, shape)
        x = np.array([[[0, 31000, 65535]]], np.uint16)                  # 1 x 1: every neighbour is the pixel itself, per channel
        assert np.array_equal(C.sharpen(x, K), x)


def test_the_hand_derived_step():
    """A 16384 / 49152 vertical edge at K = 3426 (the reference's 0.22).  At the dark pixel beside the edge: mn = 32768,
    mx = 98304, q = min(32768, 32766) = 32766, r = (32766 << 15) // 98304 = 10922, A = isqrt(5592064) = 2364,
    den = 54816 - 9456 = 45360, t = -32768, floor((-77463552 + 22680) / 45360) = -1708."""
    x = np.full((5, 8, 3), 16384, np.uint16)
    x[:, 4:] = 49152
    out = C.sharpen(x, 3426)
    for y in range(5):
        for ch in range(3):
            assert out[y, :, ch].tolist() == [16384, 16384, 16384, 14676, 50860, 49152, 49152, 49152]
    p = C.parts(x, 3426)
    at = lambda k: int(p[k][2, 3, 0])       # noqa: E731
    assert (at("mn"), at("mx"), at("q"), at("r"), at("A"), at("den"), at("t")) == (32768, 98304, 32766, 10922, 2364, 45360, -32768)
    assert np.array_equal(C.sharpen(x.transpose(1, 0, 2).copy(), 3426), out.transpose(1, 0, 2))       # the rule has no preferred axis


def test_mx_zero_and_the_bounds_of_the_intermediates_at_the_extreme_inputs():
    one = np.zeros((9, 9, 3), np.uint16)
    one[4, 4] = 65535
    rng = np.random.default_rng(11)
    frames = {"zeros": np.zeros((6, 7, 3), np.uint16), "ones": np.full((6, 7, 3), 65535, np.uint16), "checker": _checker(8, 9),
              "one bright pixel": one, "one dark pixel": 65535 - one, "noise": rng.integers(0, 65536, (40, 50, 3)).astype(np.uint16),
              "near white": rng.integers(65000, 65536, (20, 20, 3)).astype(np.uint16)}
    for K in CODES:
        for name, x in frames.items():
            p = C.parts(x, K)
            assert 0 <= p["q"].min() and (p["q"] <= p["mx"]).all() and (p["q"] << 15).max() < 2 ** 32, (name, K)
            assert 0 <= p["r"].min() and p["r"].max() <= 32768, (name, K)
            assert 0 <= p["A"].min() and p["A"].max() <= 4096, (name, K)
            assert p["den"].min() > 0 and p["den"].max() <= 65536, (name, K)
            assert np.abs(p["A"] * p["t"]).max() < 2 ** 30 and np.abs(p["num"]).max() < 2 ** 31, (name, K)
            assert 0 <= p["out"].min() and p["out"].max() <= 65535
    z = C.parts(frames["zeros"], 1032)
    assert not z["mx"].any() and not z["r"].any() and not z["out"].any()                 # mx = 0 -> r = 0, the pixel stays 0
    assert (C.parts(frames["ones"], 1032)["q"] == 0).all()                               # 131070 - mx is the minimum: A = 0
    assert np.array_equal(C.sharpen(frames["checker"], 1032), frames["checker"])         # q = 0 on a full-range checkerboard
    assert C.parts(frames["near white"], 4084)["A"].max() > 0                            # ... and not on a near-white one


def _from_view(view, H, W, dH, dW):
    """The two plain passes over ``view`` [H + 8][W + 8][3], the value the scaler reads at every tap POSITION -4 .. n + 3 of each
    axis: no clamping here, what a tap outside the frame sees is the view's business."""
    xs, qx = S.tab(W, dW)
    ys, qy = S.tab(H, dH)
    v = view.astype(np.int64)
    hor = sum(v[:, xs + 4 + k] * qx[:, k].reshape(1, dW, 1) for k in range(S.TAPS))
    acc = sum(hor[ys + 4 + k] * qy[:, k].reshape(dH, 1, 1) for k in range(S.TAPS))
    return np.clip((acc + (1 << 27)) >> 28, 0, 65535).astype(np.uint16)


def test_a_tap_outside_the_frame_reads_the_sharpened_edge_pixel():
    """Scaled 2x, the first output rows read tap positions -3 .. -1.  The rule: they see sharpen(frame)[0], the edge pixel
    sharpened from frame rows 0, 0, 1.  A halo staged by position -- the raw frame extended first, every position sharpened from
    its neighbours by position -- would sharpen position -2 from rows 0, 0, 0; on a frame whose rows 0 and 1 differ that shows."""
    rng = np.random.default_rng(3)
    K, (H, W) = 3426, (12, 14)
    x = rng.integers(20000, 45000, (H, W, 3)).astype(np.uint16)
    x[0], x[1], x[-2], x[-1] = 9000, 52000, 52000, 9000                    # rows 0 / 1 and the last two differ
    x[:, 0], x[:, 1] = 9000, 52000
    pad = lambda v, n: np.pad(v, ((n, n), (n, n), (0, 0)), mode="edge")      # noqa: E731
    rule_view = pad(C.sharpen(x, K), 4)
    naive_view = C.sharpen(pad(x, 5), K)[1:-1, 1:-1]
    assert np.array_equal(rule_view[4:-4, 4:-4], naive_view[4:-4, 4:-4])     # inside the frame both are the same
    assert np.array_equal(rule_view[2], rule_view[4]) and not np.array_equal(naive_view[2], rule_view[2])
    want = C.scale(x, 2 * H, 2 * W, K)
    assert np.array_equal(_from_view(rule_view, H, W, 2 * H, 2 * W), want)
    naive = _from_view(naive_view, H, W, 2 * H, 2 * W)
    assert not np.array_equal(naive[:3], want[:3]) and not np.array_equal(naive[:, :3], want[:, :3])
    assert np.array_equal(naive[8:-8, 8:-8], want[8:-8, 8:-8])               # away from the border nothing depends on it
    # a frame whose first and last two rows and columns agree cannot tell the two apart
    y = x.copy()
    y[0], y[-1] = y[1], y[-2]
    y[:, 0], y[:, -1] = y[:, 1], y[:, -2]
    assert np.array_equal(_from_view(C.sharpen(pad(y, 5), K)[1:-1, 1:-1], H, W, 2 * H, 2 * W), C.scale(y, 2 * H, 2 * W, K))


def test_the_composition_sharpens_first_and_code_0_is_the_scaler_alone():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 65536, (9, 13, 3)).astype(np.uint16)
    for a in (0, 77, 256):
        assert np.array_equal(C.scale(x, 20, 31, 0, a), A.scale(x, 20, 31, a))
        assert np.array_equal(C.scale(x, 20, 31, 3426, a), A.scale(C.sharpen(x, 3426), 20, 31, a))
    assert np.array_equal(C.scale(x, 20, 31, 0), S.scale(x, 20, 31))
    assert not np.array_equal(C.scale(x, 20, 31, 3426), S.scale(x, 20, 31))
    assert np.array_equal(C.scale(x, 9, 26, 3426), S.scale(C.sharpen(x, 3426), 9, 26))       # one axis at identity: still sharpened


def test_header_states_the_rule():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdrtv_mi355x.h")).read()
    for v in ("hdrtv_post_rgb48_scaled_cas", "int antiring, int cas", "131070 - mx", "(q << 15) / mx", "sqrt(r << 9)", "16 * K - 4 * A",
              "(den >> 1)", "1032..4096", "4096 - ((c * 3064 + 128) >> 8)", "tests/rgb48_cas_ref.py", "gui_scaling.py:114-138", "UNPINNED"):
        assert v in text, v


# ---------------------------------------------------------------------------------------------------------------- the strength
BAD_CAS = [True, False, "0.2", "on", "", None, float("nan"), -0.01, 1.01, 2, -1, float("inf"), [0.2], b"auto"]


def test_cas_code_known_answers_and_refusals():
    from hdrtv_mi355x import lib as L
    assert [L.cas_code(v) for v in (0.22, 0.20, 0.16, 1.0, 1, 0, 0.0, 0.5)] == [3426, 3486, 3605, 1032, 1032, 0, 0, 2564]
    assert L.cas_code(1 / 512) == 4084 and L.cas_code(0.0019) == 0 and L.cas_code(np.float32(0.22)) == 3426
    codes = [L.cas_code(c / 256) for c in range(1, 257)]
    assert codes == sorted(codes, reverse=True) and codes[0] == 4084 and codes[-1] == 1032
    assert all(L.CAS_CODE_MIN <= k <= L.CAS_CODE_MAX for k in codes) and (L.CAS_CODE_MIN, L.CAS_CODE_MAX) == (1032, 4096)
    assert all(L.cas_code(s) == C.code(s) for s in (0, 0.001, 0.0019, 0.002, 0.16, 0.2, 0.22, 0.5, 0.999, 1))
    # K / 256 is the filter's lerp(16, 4.03, s) to within the rounding of the code
    for s in (0.16, 0.20, 0.22, 1.0):
        assert abs(L.cas_code(s) / 256 - (16 + (4.03 - 16) * s)) < 0.03
    for bad in BAD_CAS + ["auto"]:
        with pytest.raises(ValueError):
            L.cas_code(bad)
    assert L.check_cas("auto") == "auto" and L.check_cas("AUTO") == "auto" and L.check_cas(0.25) == 0.25 and L.check_cas(1) == 1.0
    for bad in BAD_CAS:
        with pytest.raises(ValueError):
            L.check_cas(bad)
        with pytest.raises(ValueError):
            L.resolve_cas(bad, 96, 64, 250, 150)
    ex = dict((n, a) for n, _, a in L.SYMBOLS)
    assert ex["hdrtv_post_rgb48_scaled_cas"] == ex["hdrtv_post_rgb48_scaled_ex"] + [ctypes.c_int]
    # the descriptors keep their fields: the code travels beside them as a plain number
    assert L.OutputFormat._fields == ("pix_fmt", "siting", "h", "w")
    assert L.OutputCleanup._fields == ("deband", "deband_range", "deband_threshold", "dither")


def test_scale_cas_is_the_reference_schedule():
    from hdrtv_mi355x import lib as L
    assert L.scale_cas(960, 540, 3840, 2160) == 0.22
    assert L.scale_cas(1280, 720, 3840, 2160) == 0.20
    assert L.scale_cas(1920, 1080, 3840, 2160) == 0.16
    assert L.scale_cas(1920, 1080, 1920, 1080) == 0.0                                            # nothing is enlarged
    assert L.scale_cas(1920, 1080, 3840, 1080) == 0.0 and L.scale_cas(1920, 1080, 1920, 2160) == 0.0      # one axis equal
    assert L.scale_cas(960, 1080, 3840, 2160) == 0.22 and L.scale_cas(2000, 540, 3840, 2160) == 0.22      # either extent
    assert L.scale_cas(961, 541, 3840, 2160) == 0.20 and L.scale_cas(961, 540, 3840, 2160) == 0.22 and L.scale_cas(960, 541, 3840, 2160) == 0.22
    assert L.scale_cas(1280, 1080, 3840, 2160) == 0.20 and L.scale_cas(1281, 720, 3840, 2160) == 0.20
    assert L.scale_cas(1281, 721, 3840, 2160) == 0.16
    assert L.scale_cas(96, 64, 250, 150) == 0.22
    assert L.resolve_cas("auto", 960, 540, 3840, 2160) == 0.22 and L.resolve_cas("auto", 960, 540, 960, 540) == 0.0
    assert L.resolve_cas(0.5, 960, 540, 3840, 2160) == 0.5
    assert [L.cas_code(L.scale_cas(w, h, 3840, 2160)) for w, h in ((960, 540), (1280, 720), (1920, 1080))] == [3426, 3486, 3605]


# ---------------------------------------------------------------------------------------------------------------- validation
def test_worker_validates(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, out_w=250, out_h=150, **kw)      # noqa: E731
    assert mk()._cas == 0.0 and mk(cas=0.2)._cas == 0.2 and mk(cas="auto")._cas == "auto" and mk(cas=1)._cas == 1.0
    assert mk(cas=0.2, antiring="auto")._antiring == "auto"
    for bad in BAD_CAS:
        with pytest.raises(ValueError):
            mk(cas=bad)


def _cas_echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    v = init_args.get("cas")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = 7 if v is None else 1 if v == "auto" else 2
        out.flat[2] = 0 if v is None or v == "auto" else int(round(float(v) * 1000))
        out.flat[3] = 1 if "cas" in keys else 0
        out.flat[4] = 1 if "antiring" in keys else 0
    return process


def test_dispatcher_validates_and_hands_the_value_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    h, w = 6, 10
    run = dict(make_worker=_cas_echo_worker, slots=2, numa=False, out_height=12, out_width=20)
    for bad in BAD_CAS:
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, cas=bad, **run)
    for kw, want in (({"cas": 0.2}, [2, 2, 200, 1, 0]), ({"cas": "auto"}, [2, 1, 0, 1, 0]), ({"cas": 0.16, "antiring": 0.1}, [3, 2, 160, 1, 1]),
                     ({}, [1, 7, 0, 0, 0]), ({"cas": 0.0}, [1, 7, 0, 0, 0])):        # off: init_args keep their keys
        got = {}
        with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **kw, **run) as d:
            assert d.cas == kw.get("cas", 0.0) and d._out_b == 12 * 20 * 6
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:5].tolist() == want, kw


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    big = base + ["--out-size", "250x150"]
    assert P.parse_args(base).cas == 0.0 and P.parse_args(big).cas == 0.0                       # off by default
    assert P.parse_args(big + ["--cas", "auto"]).cas == "auto" and P.parse_args(big + ["--cas", "AUTO"]).cas == "auto"
    assert P.parse_args(big + ["--cas", "0.2"]).cas == 0.2 and P.parse_args(big + ["--cas", "1"]).cas == 1.0
    assert P.parse_args(big + ["--cas", "0"]).cas == 0.0
    both = P.parse_args(big + ["--cas", "auto", "--antiring", "0.3"])
    assert both.cas == "auto" and both.antiring == 0.3
    bad = [base + ["--cas", "auto"], base + ["--cas", "0.2"], base + ["--out-size", "96x64", "--cas", "0.2"],
           big + ["--cas", "1.5"], big + ["--cas", "-0.1"], big + ["--cas", "nan"], big + ["--cas", "on"],
           big + ["--cas", "true"], big + ["--cas", ""]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(argv)
        assert e.value.code == 2, argv


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    for cas in (0, 1032, 3426, 4096, -1, 1, 1031, 4097, 65536):            # a NULL context is refused whatever else is given
        for ar in (0, 77, 257):
            assert so.hdrtv_post_rgb48_scaled_cas(None, None, a, lib.F32, 1, 1, 0, 0.0, a, 2, 2, ar, cas) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)          # bad codes with a live context: tests/test_gpu_rgb48_cas.py
