"""The 10-bit letterbox without a GPU: the numpy rule (tests/letterbox10_ref.py) against what it must reduce to -- constant frames,
the u8 oracle on codes both rules can hold -- its geometry cases, the C ABI's declarations and NULL-context answers, the worker's
opt-in and the playback command line."""
import ctypes

import numpy as np
import pytest

import letterbox10_ref as LB
import ycbcr10_in_ref as R
from oracle import letterbox_oracle as O

# (sw, sh, dw, dh, mode): the cases of tests/test_gpu_letterbox10.py
CASES = [(192, 128, 96, 64, "area_int"), (288, 192, 96, 64, "area_int"), (384, 256, 96, 64, "area_int"), (140, 76, 70, 38, "area_int"),
         (144, 96, 96, 64, "area_frac"), (200, 116, 96, 64, "area_frac"), (64, 96, 96, 64, "area_frac"), (96, 40, 96, 64, "copy"),
         (48, 32, 96, 64, "cubic"), (50, 30, 96, 64, "cubic")]
RECTS = {(200, 116): (96, 56, 0, 4), (64, 96): (43, 64, 26, 0), (96, 40): (96, 40, 0, 12), (50, 30): (96, 58, 0, 3)}


@pytest.mark.parametrize("sw,sh,dw,dh,mode", CASES)
def test_geometry_cases_resolve_to_their_modes(sw, sh, dw, dh, mode):
    assert LB.mode_of(sw, sh, dw, dh) == mode
    new_w, new_h, x0, y0, _ = O.geometry(sw, sh, dw, dh)
    assert (new_w, new_h, x0, y0) == RECTS.get((sw, sh), (dw, dh, 0, 0))
    assert sw <= LB.MAX_SHRINK * new_w and sh <= LB.MAX_SHRINK * new_h          # inside the cap
    nw, nh, _, _, _ = O.geometry(480, 40, 96, 8)
    assert 480 > LB.MAX_SHRINK * nw                                             # the 5x case is outside it


@pytest.mark.parametrize("fmt", R.PIX_FMTS)
@pytest.mark.parametrize("sw,sh,dw,dh,mode", CASES)
def test_a_constant_frame_stays_constant_inside_the_rectangle_and_zero_outside(sw, sh, dw, dh, mode, fmt):
    """Exactly constant in the copy and area modes.  The cubic mode's 11-bit coefficients are rounded one by one, as OpenCV's are, and
    the four of a destination index sum to 2047 or 2049 for some fractions (50 -> 96: all three; 48 -> 96: 2048 throughout): a
    constant c comes out as (c * sum_x * sum_y + 2^21) >> 22, which is c wherever both sums are 2048 and within one code of it
    elsewhere (255 is kept at eight bits, 600 of 1023 is not).  That is the rule, so that is what is asserted."""
    for luma in (64, 600, 940):
        frame = R.grey_frame(np.full((sh, sw), luma, np.uint16), fmt)
        code = R.to_rgb10(frame, fmt)[0, 0]
        got = LB.letterbox10(frame, dw, dh, fmt)
        new_w, new_h, x0, y0, _ = O.geometry(sw, sh, dw, dh)
        inside = np.zeros((dh, dw), bool)
        inside[y0:y0 + new_h, x0:x0 + new_w] = True
        assert got.dtype == np.uint16 and got.shape == (dh, dw, 3)
        assert (got[~inside] == 0).all(), mode
        rect = got[y0:y0 + new_h, x0:x0 + new_w].astype(np.int64)
        if mode != "cubic":
            assert (rect == code).all(), (mode, luma)
            continue
        sx, sy = O.cubic_tab(sw, new_w)[1].sum(axis=1), O.cubic_tab(sh, new_h)[1].sum(axis=1)
        assert set(np.unique(sx)) | set(np.unique(sy)) <= {2047, 2048, 2049}
        want = (code.astype(np.int64)[None, None, :] * (sy[:, None] * sx[None, :])[..., None] + (1 << 21)) >> 22
        assert np.array_equal(rect, np.clip(want, 0, 1023)), (mode, luma)
        exact = (sy[:, None] == 2048) & (sx[None, :] == 2048)
        assert exact.any() and (rect[exact] == code).all() and np.abs(rect - code).max() <= 1, (mode, luma)


@pytest.mark.parametrize("sw,sh,dw,dh,mode", CASES)
def test_resize_stage_equals_the_u8_oracle_on_codes_both_can_hold(sw, sh, dw, dh, mode):
    """Codes in [0, 255] (area: the result is a mean, never above 255) and in [64, 192] (cubic: the negative taps of an axis sum to
    about -0.19, so the result leaves the codes' range of 128 by about (1.19^2 - 1) / 2 = 0.21 of it, 27 codes, and stays inside
    [0, 255]): the two rules differ only in the clamp, which then never acts."""
    lo, hi = (64, 193) if mode == "cubic" else (0, 256)
    codes = np.random.default_rng(sw * sh).integers(lo, hi, (sh, sw, 3), dtype=np.uint16)
    want = O.letterbox_bgr(codes.astype(np.uint8), dw, dh)
    got = LB.letterbox_codes(codes, dw, dh)
    assert got.dtype == np.uint16 and np.array_equal(got, want.astype(np.uint16))
    # and the clamp does act at ten bits where it must: full-range noise through the cubic overshoots 1023 before it
    if mode == "cubic":
        wild = np.random.default_rng(1).integers(0, 2, (sh, sw, 3), dtype=np.uint16) * 1023
        out = LB.letterbox_codes(wild, dw, dh)
        assert out.max() == 1023 and out.min() == 0
        assert LB.letterbox_codes(wild, dw, dh, top=4095).max() > 1023


def test_lib_declares_both_entry_points_and_a_null_context_is_einval():
    from hdrtv_mi355x import lib
    names = {s[0]: s for s in lib.SYMBOLS}
    assert len(names["hdrtv_letterbox_ycbcr10"][2]) == 15 and len(names["hdrtv_preprocess_ycbcr10_letterboxed"][2]) == 16
    so = lib.load()
    buf = (ctypes.c_uint16 * 4096)()
    p = ctypes.addressof(buf)
    assert so.hdrtv_letterbox_ycbcr10(None, None, p, 32, p, p, 16, lib.YCC_YUV420P10, 709, 0, 8, 16, p, 4, 8) == lib.EINVAL
    assert so.hdrtv_last_error(None) == b"null context"
    assert so.hdrtv_preprocess_ycbcr10_letterboxed(None, None, p, 32, p, p, 16, lib.YCC_YUV420P10, 709, 0, 8, 16, 4, 8, p, p) == lib.EINVAL
    assert not any(buf)


class _Called(Exception):
    pass


class _StubProcessor:
    def __init__(self):
        self.calls = []

    def preprocess_ycbcr10(self, frame, **kw):
        self.calls.append(("preprocess_ycbcr10", frame.shape, kw))
        raise _Called

    def preprocess_ycbcr10_letterboxed(self, frame, out_w, out_h, **kw):
        self.calls.append(("preprocess_ycbcr10_letterboxed", frame.shape, out_w, out_h, kw))
        raise _Called


def _stub_worker(monkeypatch):
    import torch
    from hdrtv_mi355x.worker import HeadlessPipelineWorker

    class Ev:
        def record(self, *a):
            pass

    w = HeadlessPipelineWorker("unused", proc_w=96, proc_h=64)
    w._processor = _StubProcessor()
    monkeypatch.setattr(w, "_cuda_timing_events", lambda: (Ev(), Ev()))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: None)
    return w


@pytest.mark.parametrize("fmt", R.PIX_FMTS)
def test_worker_refuses_by_default_and_letterboxes_on_request(monkeypatch, fmt):
    w = _stub_worker(monkeypatch)
    fmt_dict = {"pix_fmt": fmt, "matrix": 2020, "full_range": True}
    big, fit = R.random_frame(128, 192, 1, fmt), R.random_frame(64, 96, 2, fmt)
    w.set_input_format(fmt, 2020, True)
    assert w._yuv_format == fmt_dict
    with pytest.raises(ValueError, match="letterbox"):
        w._process_frame(frame=big, frame_idx=0, mpv_w=False)
    assert w._processor.calls == []
    w.set_input_format(fmt, 2020, True, letterbox=True)
    assert w._yuv_format == fmt_dict                                 # the flag lives beside the dict, not in it
    with pytest.raises(_Called):
        w._process_frame(frame=big, frame_idx=0, mpv_w=False)
    assert w._processor.calls == [("preprocess_ycbcr10_letterboxed", big.shape, 96, 64, fmt_dict)]
    with pytest.raises(_Called):                                     # a frame of the processing size takes the call it took before
        w._process_frame(frame=fit, frame_idx=1, mpv_w=False)
    assert w._processor.calls[-1] == ("preprocess_ycbcr10", fit.shape, fmt_dict)
    w.set_input_format(fmt, 2020, True)                              # and the opt-in does not outlive the call that gave it
    with pytest.raises(ValueError, match="letterbox"):
        w._process_frame(frame=big, frame_idx=2, mpv_w=False)


def test_playback_src_size_is_parsed_and_handed_on(monkeypatch, tmp_path):
    from hdrtv_mi355x import playback as P
    import hdrtv_mi355x.worker as WK
    seen = {}

    class Stop(Exception):
        pass

    class FakeWorker:
        def __init__(self, *a, **k):
            seen["proc"] = (k["proc_w"], k["proc_h"])

        def _load_model(self, key):
            return True

        def set_input_format(self, pix_fmt, yuv_matrix=709, yuv_full_range=False, **kw):
            seen["fmt"] = (pix_fmt, yuv_matrix, yuv_full_range, kw)
            raise Stop

    def fake_source(path, w, h, fps, **kw):
        seen["src"] = (w, h)
        src = P.SyntheticSource(w, h, fps, 2)
        src.pix_fmt, src.yuv_matrix, src.yuv_full_range = kw["pix_fmt"], kw["yuv_matrix"], kw["yuv_full_range"]
        return src

    fake_source.PIX_FMTS = P.RawVideoSource.PIX_FMTS
    monkeypatch.setattr(WK, "HeadlessPipelineWorker", FakeWorker)
    monkeypatch.setattr(P, "RawVideoSource", fake_source)
    base = ["--weights-dir", str(tmp_path), "--input", "x.yuv", "--no-prefetch", "--size", "96x64"]
    a = P.parse_args(base)
    assert a.src_wh == a.proc_wh == (96, 64)
    a = P.parse_args(base + ["--src-size", "192x128"])
    assert a.src_wh == (192, 128) and a.proc_wh == (96, 64) and a.out_wh == (96, 64)
    for bad in ("192", "0x128", "ax b"):
        with pytest.raises(SystemExit):
            P.parse_args(base + ["--src-size", bad])
    for fmt in R.PIX_FMTS:                                           # a 10-bit format with a differing --src-size sets the opt-in
        with pytest.raises(Stop):
            P.main(base + ["--pix-fmt", fmt, "--src-size", "192x128", "--yuv-matrix", "601"])
        assert seen == {"proc": (96, 64), "src": (192, 128), "fmt": (fmt, 601, False, {"letterbox": True})}
        with pytest.raises(Stop):                                    # ... an equal one does not
            P.main(base + ["--pix-fmt", fmt, "--src-size", "96x64"])
        assert seen == {"proc": (96, 64), "src": (96, 64), "fmt": (fmt, 709, False, {})}
    with pytest.raises(Stop):                                        # the 8-bit formats are letterboxed by the worker without it
        P.main(base + ["--pix-fmt", "nv12", "--src-size", "192x128"])
    assert seen == {"proc": (96, 64), "src": (192, 128), "fmt": ("nv12", 709, False, {})}
