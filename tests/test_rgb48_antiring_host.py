"""Anti-ringing of the fused Lanczos upscale (hdrtv_post_rgb48_scaled_ex), the parts that need no GPU: the facts the integer rule
(include/hdrtv_mi355x.h steps 3a / 3b, restated in tests/rgb48_antiring_ref.py) states about itself, the strength code and the
reference's schedule (lib.antiring_code, lib.scale_antiring), and the argument checks of every layer that carries the strength --
the worker, the dispatcher, the playback command line, the C entry point's refusals that return before any device call."""
import ctypes
import os

import numpy as np
import pytest

import rgb48_antiring_ref as A
import rgb48_scale_ref as S

SHAPES = [((36, 52), (72, 104)), ((36, 52), (97, 131)), ((5, 7), (64, 200)), ((100, 150), (257, 333)), ((61, 103), (61, 206)),
          ((61, 103), (122, 103)), ((61, 103), (61, 103))]
LO, HI = 16384, 49151          # the codes of 0.25 and 0.75


def step(h, w):
    """The 0.25 / 0.75 step on both axes: red and blue step along x, green along y."""
    src = np.full((h, w, 3), LO, np.uint16)
    src[:, w // 2:, 0] = HI
    src[h // 2:, :, 1] = HI
    src[:, w // 2:, 2] = HI
    return src


def contents(h, w):
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    return {
        "uniform": rng.integers(0, 65536, (h, w, 3)).astype(np.uint16),
        "checker": np.broadcast_to((((yy + xx) & 1) * 65535).astype(np.uint16)[..., None], (h, w, 3)).copy(),
        "step": step(h, w),
        "flat": np.full((h, w, 3), 39977, np.uint16),
    }


def outside(out, lo, hi):
    """(number of values outside [lo, hi], the largest excess)."""
    o = out.astype(np.int64)
    e = np.maximum(o - hi, 0) + np.maximum(lo.astype(np.int64) - o, 0)
    return int((e > 0).sum()), int(e.max())


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_strength_0_is_the_plain_rule_and_full_strength_stays_in_the_envelope(src, dst):
    (h, w), (dh, dw) = src, dst
    for name, x in contents(h, w).items():
        assert np.array_equal(A.scale(x, dh, dw, 0), S.scale(x, dh, dw)), name
        lo, hi = A.envelope(x, dh, dw)
        assert lo.shape == (dh, dw, 3) and (lo <= hi).all()
        assert outside(A.scale(x, dh, dw, A.FULL), lo, hi) == (0, 0), name
        if name == "flat":
            for a in (1, 77, 256):
                assert (A.scale(x, dh, dw, a) == 39977).all()


def test_an_axis_at_identity_is_untouched():
    x = contents(61, 103)["uniform"]
    for a in (26, 77, 256):
        assert np.array_equal(A.scale(x, 61, 103, a), x)
        p = A.passes(x, 61, 206, a)
        assert not p["d_v"].any() and np.array_equal(p["v"], p["hor"] << 14)       # the vertical pass is the identity
        assert not A.passes(x, 122, 103, a)["d_h"].any()


def test_the_step_overshoot_shrinks_with_the_strength_and_is_gone_at_full():
    x = step(36, 52)
    lo, hi = A.envelope(x, 72, 104)
    assert lo.min() == LO and hi.max() == HI
    n0, e0 = outside(A.scale(x, 72, 104, 0), lo, hi)
    n77, e77 = outside(A.scale(x, 72, 104, 77), lo, hi)
    n256, e256 = outside(A.scale(x, 72, 104, 256), lo, hi)
    print(f"0.25 / 0.75 step 36x52 -> 72x104: a = 0: {n0} values outside, largest excess {e0}; a = 77: {n77}, {e77}; a = 256: {n256}, {e256}")
    assert (n0, e0) == (1984, 3382) and e77 == 2365              # the figures of the plain rule and of the reference's 0.30
    assert e0 > e77 > e256 == 0 and n256 == 0
    # monotone in between as well
    worst = [outside(A.scale(x, 72, 104, a), lo, hi)[1] for a in (0, 1, 26, 56, 77, 128, 255, 256)]
    assert all(p > q for p, q in zip(worst, worst[1:])), worst


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_intermediate_values_fit_the_device_types(src, dst):
    (h, w), (dh, dw) = src, dst
    for name, x in contents(h, w).items():
        for a in (0, 77, 256):
            p = A.passes(x, dh, dw, a)
            assert np.abs(p["hor"]).max() < 2 ** 31 and np.abs(p["d_h"]).max() < 2 ** 31, (name, a)      # int32 in the horizontal pass
            # the device splits d of the vertical pass at bit 16: the high part is an int32 factor
            assert np.abs(p["d_v"]).max() < 2 ** 46 and np.abs(p["v"]).max() < 2 ** 46, (name, a)


def test_split_products_equal_the_64_bit_form():
    """The device keeps d * a off the 64-bit multiplier: d = dh * 2^s + dl, and (d * a + 128) >> 8 = dh * a * 2^(s-8) + ((dl * a + 128) >> 8)
    for s = 8 (horizontal) and s = 16 (vertical).  Python integers, flooring shifts."""
    rng = np.random.default_rng(5)
    ds = [0, 1, -1, 255, 256, -256, -257, 2 ** 28 - 1, -2 ** 28, 2 ** 31 - 1, -2 ** 31] + [int(v) for v in rng.integers(-2 ** 31, 2 ** 31, 500)]
    for d in ds:
        for a in (1, 26, 77, 255, 256):
            assert (d * a + 128) >> 8 == (d >> 8) * a + ((((d & 255) * a) + 128) >> 8)
    dv = [0, -1, 65535, 65536, -65537, 2 ** 46 - 1, -2 ** 46] + [int(v) for v in rng.integers(-2 ** 46, 2 ** 46, 500)]
    for d in dv:
        for a in (1, 26, 77, 255, 256):
            assert (d * a + 128) >> 8 == (d >> 16) * (a << 8) + ((((d & 65535) * a) + 128) >> 8)
            assert -2 ** 31 <= d >> 16 < 2 ** 31


def test_header_states_the_rule():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdrtv_mi355x.h")).read()
    for v in ("hdrtv_post_rgb48_scaled_ex", "int antiring", "(d * a + 128) >> 8", "<< 14", "0..256", "floor(s * 256 + 0.5)",
              "tests/rgb48_antiring_ref.py", "gui_scaling.py:82-111", "UNPINNED"):
        assert v in text, v
    assert "No anti-ringing" not in text


# ---------------------------------------------------------------------------------------------------------------- the strength
BAD_ANTIRING = [True, False, "0.3", "on", "", None, float("nan"), -0.01, 1.01, 2, -1, float("inf"), [0.3], b"auto"]


def test_antiring_code_known_answers_and_refusals():
    from hdrtv_mi355x import lib as L
    assert [L.antiring_code(v) for v in (0.30, 0.22, 0.10, 1.0, 0, 0.0, 1, 0.5)] == [77, 56, 26, 256, 0, 0, 256, 128]
    assert L.antiring_code(np.float32(0.3)) == 77 and L.antiring_code(1 / 512) == 1 and L.antiring_code(0.0019) == 0
    for bad in BAD_ANTIRING + ["auto"]:
        with pytest.raises(ValueError):
            L.antiring_code(bad)
    assert L.check_antiring("auto") == "auto" and L.check_antiring("AUTO") == "auto" and L.check_antiring(0.25) == 0.25
    for bad in BAD_ANTIRING:
        with pytest.raises(ValueError):
            L.check_antiring(bad)
    names = [n for n, _, _ in L.SYMBOLS]
    assert "hdrtv_post_rgb48_scaled_ex" in names
    ex = dict((n, a) for n, _, a in L.SYMBOLS)
    assert ex["hdrtv_post_rgb48_scaled_ex"] == ex["hdrtv_post_rgb48_scaled"] + [ctypes.c_int]
    # the descriptors keep their fields: the strength travels beside them as a plain number
    assert L.OutputFormat._fields == ("pix_fmt", "siting", "h", "w")
    assert L.OutputCleanup._fields == ("deband", "deband_range", "deband_threshold", "dither")


def test_scale_antiring_is_the_reference_schedule():
    from hdrtv_mi355x import lib as L
    assert L.scale_antiring(960, 540, 3840, 2160) == 0.30
    assert L.scale_antiring(1280, 720, 3840, 2160) == 0.22
    assert L.scale_antiring(1920, 1080, 3840, 2160) == 0.10
    assert L.scale_antiring(1920, 1080, 1920, 1080) == 0.0                # nothing is enlarged
    assert L.scale_antiring(1920, 1080, 3840, 1080) == 0.0 and L.scale_antiring(1920, 1080, 1920, 2160) == 0.0      # one axis equal
    assert L.scale_antiring(1280, 1080, 3840, 2160) == 0.22 and L.scale_antiring(2000, 540, 3840, 2160) == 0.30      # either extent
    assert L.scale_antiring(961, 541, 3840, 2160) == 0.22 and L.scale_antiring(1281, 721, 3840, 2160) == 0.10
    assert L.scale_antiring(96, 64, 250, 150) == 0.30
    assert L.resolve_antiring("auto", 960, 540, 3840, 2160) == 0.30 and L.resolve_antiring("auto", 960, 540, 960, 540) == 0.0
    assert L.resolve_antiring(0.5, 960, 540, 3840, 2160) == 0.5
    assert [L.antiring_code(L.scale_antiring(w, h, 3840, 2160)) for w, h in ((960, 540), (1280, 720), (1920, 1080))] == [77, 56, 26]


# ---------------------------------------------------------------------------------------------------------------- validation
def test_worker_validates(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, out_w=250, out_h=150, **kw)      # noqa: E731
    assert mk()._antiring == 0.0 and mk(antiring=0.3)._antiring == 0.3 and mk(antiring="auto")._antiring == "auto"
    assert mk(antiring=1)._antiring == 1.0
    for bad in BAD_ANTIRING:
        with pytest.raises(ValueError):
            mk(antiring=bad)


def _antiring_echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    v = init_args.get("antiring")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = 7 if v is None else 1 if v == "auto" else 2
        out.flat[2] = 0 if v is None or v == "auto" else int(round(float(v) * 1000))
        out.flat[3] = 1 if "antiring" in keys else 0
    return process


def test_dispatcher_validates_and_hands_the_value_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    h, w = 6, 10
    run = dict(make_worker=_antiring_echo_worker, slots=2, numa=False, out_height=12, out_width=20)
    for bad in BAD_ANTIRING:
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, antiring=bad, **run)
    for value, want in ((0.22, [2, 2, 220, 1]), ("auto", [2, 1, 0, 1])):
        got = {}
        with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, antiring=value, **run) as d:
            assert d.antiring == value and d._out_b == 12 * 20 * 6
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:4].tolist() == want, value
    got = {}
    with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **run) as d:      # off
        assert d.antiring == 0.0
        d.submit(np.zeros((h, w, 3), np.uint8))
        d.flush(timeout=60)
    assert d.exit_codes == [0] and got[0].reshape(-1)[:4].tolist() == [1, 7, 0, 0]           # init_args keep their keys


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    big = base + ["--out-size", "250x150"]
    assert P.parse_args(base).antiring == 0.0 and P.parse_args(big).antiring == 0.0            # off by default
    assert P.parse_args(big + ["--antiring", "auto"]).antiring == "auto"
    assert P.parse_args(big + ["--antiring", "0.3"]).antiring == 0.3 and P.parse_args(big + ["--antiring", "1"]).antiring == 1.0
    assert P.parse_args(big + ["--antiring", "0"]).antiring == 0.0
    bad = [base + ["--antiring", "auto"], base + ["--antiring", "0.3"], base + ["--out-size", "96x64", "--antiring", "0.3"],
           big + ["--antiring", "1.5"], big + ["--antiring", "-0.1"], big + ["--antiring", "nan"], big + ["--antiring", "on"],
           big + ["--antiring", "true"], big + ["--antiring", ""]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(argv)
        assert e.value.code == 2, argv


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    for ar in (0, 77, 256, -1, 257):
        assert so.hdrtv_post_rgb48_scaled_ex(None, None, a, lib.F32, 1, 1, 0, 0.0, a, 1, 1, ar) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)
