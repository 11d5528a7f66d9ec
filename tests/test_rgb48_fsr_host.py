"""The FSR upscale of the RGB48 output (hdrtv_post_rgb48_fsr), the parts that need no GPU: known answers of the NumPy restatement of
the rule (tests/rgb48_fsr_ref.py), the reference over every frame of the device test, the division-free sample conversion of the
kernel, and the host surface that carries the scaler (lib, the worker, the dispatcher, the playback command line)."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import rgb48_fsr_ref as F
from test_gpu_rgb48_fsr import MODES, SHAPES, contents

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------- the rule
def test_position_tables():
    fp, pp = F.positions(4, 8)                                     # exact 2x
    assert fp.dtype == np.int32 and pp.dtype == np.float32
    assert fp.tolist() == [-1, 0, 0, 1, 1, 2, 2, 3] and pp.tolist() == [0.75, 0.25] * 4
    fp, pp = F.positions(1080, 2160)
    assert fp[0] == -1 and fp[-1] == 1079 and set(pp.tolist()) == {0.25, 0.75} and np.array_equal(fp[1::2], np.arange(1080))
    fp, pp = F.positions(7, 7)                                     # identity
    assert fp.tolist() == list(range(7)) and not pp.any()
    fp, pp = F.positions(37, 64)                                   # ragged: p = (d + 0.5) * 37 / 64 - 0.5
    assert fp[:6].tolist() == [-1, 0, 0, 1, 2, 2] and fp[-1] == 36 and (np.diff(fp) >= 0).all() and np.diff(fp).max() == 1
    assert pp[0] == f32(0.7890625) and pp[1] == f32(0.3671875) and pp[63] == f32((63.5 * 37 / 64 - 0.5) - 36)
    assert (pp >= 0).all() and (pp < 1).all()
    for n, m in ((37, 64), (33, 34), (1, 2), (17, 33)):            # a step of one output pixel moves fp by at most one source pixel
        fp, _ = F.positions(n, m)
        assert fp[0] >= -1 and fp[-1] <= n - 1 and np.diff(fp).min() >= 0 and np.diff(fp).max() <= 1


def test_bit_pattern_approximations():
    bits = lambda v: int(np.asarray(v, f32).view(np.uint32))      # noqa: E731
    for a, pat in ((1.0, 0x3F800000), (0.5, 0x3F000000), (0.0, 0)):
        assert bits(a) == pat
        assert bits(F.aprx_rcp(f32(a))) == 0x7EF07EBB - pat
        assert bits(F.aprx_rsq(f32(a))) == 0x5F347D74 - (pat >> 1)
    # 0x3f707ebb, 0x3ff07ebb and 0x3f747d74 as numbers: crude values of 1 / 1, 1 / 0.5 and 1 / sqrt(1), as the rule wants them
    assert F.aprx_rcp(f32(1.0)) == f32(0.93943375) and F.aprx_rcp(f32(0.5)) == f32(1.8788675) and F.aprx_rsq(f32(1.0)) == f32(0.95503926)
    assert np.isfinite(F.aprx_rcp(f32(0.0))) and np.isfinite(F.aprx_rsq(f32(0.0)))
    a = np.array([1.0, 0.5, 0.0], f32)
    assert F.aprx_rcp(a).dtype == np.float32 and F.aprx_rcp(a).shape == (3,)


def test_constants_are_the_float32_values_the_header_names():
    assert F.LOB_K == f32(-0.29) and F.W_B == f32(0.4) and F.RCAS_LIMIT == f32(0.1875) and F.EPS == f32(1e-6)
    assert F.sharp_factor(0.0) == 1.0 and F.sharp_factor(2.0) == 0.25 and F.sharp_factor(1) == 0.5
    assert F.sharp_factor(0.2) == f32(2.0 ** -float(f32(0.2)))     # from the float32 the C entry point receives


def test_a_flat_frame_returns_its_code():
    for v in sorted(set([0, 1, 2, 3, 32768, 33297, 65534, 65535] + list(range(0, 65536, 257)))):
        x = np.full((6, 7, 3), v, np.uint16)
        for mode in MODES:
            for dh, dw in ((12, 14), (9, 13)):
                assert (F.scale(x, dh, dw, mode) == v).all(), (v, mode, dh, dw)


def test_a_single_pixel_is_repeated():
    x = np.array([[[7, 30000, 65535]]], np.uint16)
    for dh, dw in ((2, 2), (1, 2), (2, 1)):
        for mode in MODES:
            assert np.array_equal(F.scale(x, dh, dw, mode), np.broadcast_to(x[0, 0], (dh, dw, 3))), (dh, dw, mode)
    assert np.array_equal(F.scale(x, 1, 1, 0.2), x)                # equal sizes: the codes


def test_easu_alone_stays_inside_its_four_inner_codes():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 65536, (19, 23, 3)).astype(np.uint16)
    for dh, dw in ((38, 46), (30, 41), (19, 46)):
        out = F.scale(x, dh, dw).astype(int)
        fy, _ = F.positions(19, dh)
        fx, _ = F.positions(23, dw)
        y0, y1 = np.clip(fy, 0, 18)[:, None], np.clip(fy + 1, 0, 18)[:, None]
        x0, x1 = np.clip(fx, 0, 22)[None, :], np.clip(fx + 1, 0, 22)[None, :]
        four = np.stack([x[y0, x0], x[y0, x1], x[y1, x0], x[y1, x1]]).astype(int)
        assert (out >= four.min(0)).all() and (out <= four.max(0)).all()
        assert (out != four[0]).any()                               # and it does interpolate
    # RCAS may leave that interval: it sharpens
    out = F.scale(x, 38, 46, 0.0).astype(int)
    assert not np.array_equal(out, F.scale(x, 38, 46).astype(int))


def test_sharpness_2_changes_less_than_sharpness_0():
    rng = np.random.default_rng(6)
    x = rng.integers(0, 65536, (24, 31, 3)).astype(np.uint16)
    base = F.scale(x, 48, 62).astype(int)
    d0, d2 = F.scale(x, 48, 62, 0.0).astype(int) - base, F.scale(x, 48, 62, 2.0).astype(int) - base
    assert 0 < (d2 != 0).sum() < (d0 != 0).sum()
    assert np.abs(d2).sum() < np.abs(d0).sum()


def test_refused_sizes():
    x = np.zeros((4, 6, 3), np.uint16)
    for dh, dw in ((9, 6), (4, 13), (3, 6), (4, 5)):
        with pytest.raises(ValueError):
            F.scale(x, dh, dw)
    assert F.scale(x, 8, 12, 0.2).shape == (8, 12, 3) and F.scale(x, 8, 12).dtype == np.uint16


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_the_reference_is_finite_on_every_frame_of_the_device_test(src, dst):
    """No NaN anywhere and the EASU weight sum aW stays positive (the division aC / aW is then harmless).  The float tensors of the
    device test are quantised here by the plain rule; the PQ codes of the same tensors are other integers of the same kind."""
    (h, w), (dh, dw) = src, dst
    low = np.inf
    for name, t in contents(h, w).items():
        codes = F.quant(np.clip(t, 0, 1).transpose(1, 2, 0))
        img, aw = F.easu(codes, dh, dw, with_weight=True)
        assert np.isfinite(img).all() and np.isfinite(aw).all(), name
        assert (aw > 0).all(), (name, float(aw.min()))
        low = min(low, float(aw.min()))
        for mode in MODES[1:]:
            out = F.rcas(img, mode)
            assert np.isfinite(out).all() and (out >= 0).all() and (out <= 1).all(), (name, mode)
    print("%dx%d -> %dx%d: smallest aW %.4f" % (h, w, dh, dw, low))


def _round_f32(x):
    """A Fraction -> the nearest float32 (ties to even), without going through a double rounding."""
    a = f32(float(x))
    best = None
    for c in (np.nextafter(a, f32(-np.inf)), a, np.nextafter(a, f32(np.inf))):
        err = abs(Fraction(float(c)) - x)
        even = (int(np.asarray(c, f32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, c)
    return best[1]


def test_the_kernel_gets_a_sample_without_a_division():
    """csrc/post_fsr.hip: q = c * r, e = fma(-q, 65535, c), s = fma(e, r, q) with r = float32(1 / 65535) is the correctly rounded
    c / 65535 for every code -- in exact arithmetic, each of the three operations rounded once."""
    r = Fraction(float(f32(1.0 / 65535.0)))
    want = np.arange(65536, dtype=f32) / f32(65535)
    plain = 0
    for c in range(65536):
        q = Fraction(float(_round_f32(c * r)))
        e = Fraction(float(_round_f32(c - q * 65535)))
        s = _round_f32(e * r + q)
        assert s == want[c], c
        plain += float(_round_f32(c * r)) != float(want[c])
    assert plain > 0                    # the product alone is not enough: the correction step is needed
    text = open(os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc", "post_fsr.hip")).read()
    assert "__fmaf_rn(__fmaf_rn(-q, 65535.f, x), r, q)" in text and "(float)(1.0 / 65535.0)" in text


def test_header_makefile_and_kernel_state_the_rule():
    text = open(os.path.join(REPO, "include", "hdrtv_mi355x.h")).read()
    for v in ("hdrtv_post_rgb48_fsr", "int rcas, float sharpness", "0x7ef07ebb", "0x5f347d74", "1 / 32768", "b c i j f e k l h g o n",
              "(0.2126 r + 0.7152 g)", "float32(c) / float32(65535)", "(d + 0.5) * n / m - 0.5", "tests/rgb48_fsr_ref.py", "0.25 - 1/16",
              "2^-sharpness", "H <= dH <= 2H", "gui_scaling.py:42-43", "UNPINNED"):
        assert v in text, v
    mk = open(os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc", "Makefile")).read()
    assert " post_fsr.hip " in mk and "$(BUILD)/post_fsr.o: CXXFLAGS += -ffp-contract=off" in mk
    assert any("post_fsr.o" in ln and ln.rstrip().endswith(": post_quant.h") for ln in mk.splitlines())
    src = open(os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc", "post_fsr.hip")).read()
    for banned in ("__fdividef", "__frcp_rn", "rsqrtf", "__builtin_amdgcn_rcp", "__builtin_amdgcn_rsq", "__builtin_amdgcn_sqrt", "sqrtf"):
        assert banned not in src, banned


# ------------------------------------------------------------------------------------------------------------------- the options
BAD_SHARP = [True, False, "0.2", "none", "", float("nan"), -0.01, 2.01, 3, -1, float("inf"), [0.2], b"0.2"]
BAD_SCALER = [None, True, 0, 1, "", "bicubic", "fsr2", "ewa", b"fsr", ["fsr"]]


def test_check_scaler_and_check_fsr_sharpness():
    from hdrtv_mi355x import lib as L
    assert L.SCALERS == ("lanczos", "fsr") and L.FSR_MAX_RATIO == 2 and L.FSR_SHARPNESS == 0.2
    assert L.check_scaler() == "lanczos" and L.check_scaler("lanczos") == "lanczos" and L.check_scaler("fsr") == "fsr"
    assert L.check_scaler("FSR") == "fsr" and L.check_scaler("Lanczos") == "lanczos"
    for bad in BAD_SCALER:
        with pytest.raises(ValueError):
            L.check_scaler(bad)
    assert L.check_fsr_sharpness(None) is None
    assert [L.check_fsr_sharpness(v) for v in (0, 0.0, 0.2, 1, 2, 2.0, np.float32(0.5))] == [0.0, 0.0, 0.2, 1.0, 2.0, 2.0, 0.5]
    assert all(type(L.check_fsr_sharpness(v)) is float for v in (0, 1, np.float32(0.5)))
    for bad in BAD_SHARP:
        with pytest.raises(ValueError):
            L.check_fsr_sharpness(bad)
    ex = dict((n, a) for n, _, a in L.SYMBOLS)
    assert ex["hdrtv_post_rgb48_fsr"] == ex["hdrtv_post_rgb48_scaled"] + [ctypes.c_int, ctypes.c_float]


def test_check_fsr_size_names_the_limit():
    from hdrtv_mi355x import lib as L
    for ok in ((1920, 1080, 3840, 2160), (96, 64, 96, 64), (96, 64, 192, 64), (96, 64, 97, 128), (1, 1, 2, 2)):
        L.check_fsr_size(*ok)
    for bad in ((96, 64, 193, 128), (96, 64, 192, 129), (1920, 1080, 3840, 2161), (960, 540, 3840, 2160), (1, 1, 3, 1)):
        with pytest.raises(ValueError, match="2x"):
            L.check_fsr_size(*bad)
    with pytest.raises(ValueError, match="192x128"):
        L.check_fsr_size(96, 64, 250, 150)
    with pytest.raises(ValueError, match="below"):
        L.check_fsr_size(96, 64, 95, 128)


def test_cas_and_antiring_under_the_scaler():
    from hdrtv_mi355x import lib as L
    # lanczos: both pass through, checked
    assert L.scaler_options("lanczos") == (0.0, 0.0)
    assert L.scaler_options("lanczos", "auto", 0.2) == ("auto", 0.2) and L.scaler_options("Lanczos", 0.3, "AUTO") == (0.3, "auto")
    # fsr: the reference's schedules give 0 for both, so "auto" is 0; an explicit nonzero value is refused
    assert L.scaler_options("fsr") == (0.0, 0.0) and L.scaler_options("fsr", "auto", "auto") == (0.0, 0.0)
    assert L.scaler_options("fsr", 0, 0.0) == (0.0, 0.0) and L.scaler_options("FSR", "AUTO", 0) == (0.0, 0.0)
    for kw in (dict(antiring=0.3), dict(cas=0.2), dict(antiring=1, cas="auto"), dict(antiring="auto", cas=1e-3)):
        with pytest.raises(ValueError, match="lanczos"):
            L.scaler_options("fsr", **kw)
    for s in ("lanczos", "fsr"):
        for kw in (dict(antiring=True), dict(cas="on"), dict(antiring=1.5), dict(cas=float("nan"))):
            with pytest.raises(ValueError):
                L.scaler_options(s, **kw)
    with pytest.raises(ValueError):
        L.scaler_options("ewa")


def test_worker_validates(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, **{"out_w": 192, "out_h": 128, **kw})      # noqa: E731
    wk = mk()
    assert (wk._scaler, wk._fsr_sharpness, wk._cas, wk._antiring) == ("lanczos", 0.2, 0.0, 0.0)
    wk = mk(scaler="fsr", cas="auto", antiring="auto")
    assert (wk._scaler, wk._fsr_sharpness, wk._cas, wk._antiring) == ("fsr", 0.2, 0.0, 0.0)
    assert mk(scaler="FSR", fsr_sharpness=None)._fsr_sharpness is None and mk(scaler="fsr", fsr_sharpness=2)._fsr_sharpness == 2.0
    assert mk(scaler="lanczos", cas="auto", antiring=0.3)._cas == "auto"
    assert mk(scaler="fsr", out_w=96, out_h=64)._scaler == "fsr"                   # nothing enlarged: nothing to refuse
    for kw in ([dict(scaler=s) for s in BAD_SCALER] + [dict(scaler="fsr", fsr_sharpness=s) for s in BAD_SHARP] +
               [dict(fsr_sharpness="sharp"), dict(scaler="fsr", cas=0.2), dict(scaler="fsr", antiring=0.3),
                dict(scaler="fsr", out_w=193), dict(scaler="fsr", out_h=129), dict(scaler="fsr", out_w=250, out_h=150)]):
        with pytest.raises(ValueError):
            mk(**kw)
    mk(out_w=250, out_h=150)                                                       # the Lanczos scaler has no such limit


def _echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    s, v = init_args.get("scaler"), init_args.get("fsr_sharpness", "absent")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = 7 if s is None else 1 if s == "fsr" else 2
        out.flat[2] = 9999 if v == "absent" else 5555 if v is None else int(round(float(v) * 1000))
        out.flat[3] = 1 if "cas" in keys else 0
        out.flat[4] = 1 if "antiring" in keys else 0
    return process


def test_dispatcher_validates_and_hands_the_scaler_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    h, w = 6, 10
    run = dict(make_worker=_echo_worker, slots=2, numa=False, out_height=12, out_width=20)
    for kw in ([dict(scaler=s) for s in BAD_SCALER[:6]] + [dict(scaler="fsr", fsr_sharpness=s) for s in BAD_SHARP[:8]] +
               [dict(scaler="fsr", cas=0.2), dict(scaler="fsr", antiring=0.3), dict(scaler="fsr", out_width=21),
                dict(scaler="fsr", out_height=13)]):
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, **{**run, **kw})
    for kw, want in (({"scaler": "fsr"}, [3, 1, 200, 0, 0]), ({"scaler": "FSR", "fsr_sharpness": None}, [3, 1, 5555, 0, 0]),
                     ({"scaler": "fsr", "fsr_sharpness": 1.5, "cas": "auto", "antiring": "auto"}, [3, 1, 1500, 0, 0]),
                     ({}, [1, 7, 9999, 0, 0]), ({"scaler": "lanczos", "fsr_sharpness": 1.0}, [1, 7, 9999, 0, 0]),       # off: init_args keep their keys
                     ({"scaler": "lanczos", "cas": 0.2}, [2, 7, 9999, 1, 0])):
        got = {}
        with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **kw, **run) as d:
            assert d.scaler == kw.get("scaler", "lanczos").lower() and d._out_b == 12 * 20 * 6
            if d.scaler == "fsr":
                assert d.cas == 0.0 and d.antiring == 0.0
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:5].tolist() == want, kw


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    big = base + ["--out-size", "192x128"]
    a = P.parse_args(big)
    assert (a.scaler, a.fsr_sharpness, a.cas, a.antiring) == ("lanczos", 0.2, 0.0, 0.0)         # off by default
    a = P.parse_args(big + ["--scaler", "fsr"])
    assert (a.scaler, a.fsr_sharpness, a.cas, a.antiring) == ("fsr", 0.2, 0.0, 0.0)
    assert P.parse_args(big + ["--scaler", "fsr", "--fsr-sharpness", "0"]).fsr_sharpness == 0.0
    assert P.parse_args(big + ["--scaler", "fsr", "--fsr-sharpness", "2"]).fsr_sharpness == 2.0
    assert P.parse_args(big + ["--scaler", "fsr", "--fsr-sharpness", "none"]).fsr_sharpness is None
    a = P.parse_args(big + ["--scaler", "fsr", "--cas", "auto", "--antiring", "auto"])           # the schedules give 0 for FSR
    assert a.cas == 0.0 and a.antiring == 0.0
    assert P.parse_args(big + ["--scaler", "fsr", "--cas", "0", "--antiring", "0"]).cas == 0.0
    assert P.parse_args(base + ["--out-size", "100x128", "--scaler", "fsr"]).out_wh == (100, 128)
    assert P.parse_args(base + ["--out-size", "96x128", "--scaler", "fsr"]).scaler == "fsr"     # one axis at identity still enlarges
    a = P.parse_args(base + ["--out-size", "250x150", "--scaler", "lanczos", "--cas", "auto", "--antiring", "0.3"])
    assert (a.scaler, a.cas, a.antiring) == ("lanczos", "auto", 0.3)
    bad = [base + ["--scaler", "fsr"], base + ["--out-size", "96x64", "--scaler", "fsr"],         # nothing is enlarged
           base + ["--out-size", "193x128", "--scaler", "fsr"], base + ["--out-size", "192x129", "--scaler", "fsr"],
           base + ["--out-size", "250x150", "--scaler", "fsr"],                                   # more than 2x
           big + ["--scaler", "fsr", "--cas", "0.2"], big + ["--scaler", "fsr", "--antiring", "0.3"],
           big + ["--scaler", "fsr", "--fsr-sharpness", "2.5"], big + ["--scaler", "fsr", "--fsr-sharpness", "-0.1"],
           big + ["--scaler", "fsr", "--fsr-sharpness", "nan"], big + ["--scaler", "fsr", "--fsr-sharpness", "sharp"],
           big + ["--scaler", "fsr", "--fsr-sharpness", ""], big + ["--fsr-sharpness", "0.2"],    # belongs to --scaler fsr
           big + ["--scaler", "lanczos", "--fsr-sharpness", "0.2"], big + ["--scaler", "bicubic"], big + ["--scaler", "FSR"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(argv)
        assert e.value.code == 2, argv


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    for rcas in (0, 1, 2, -1):            # a NULL context is refused whatever else is given
        for sharp in (0.2, -0.1, 2.5, float("nan")):
            assert so.hdrtv_post_rgb48_fsr(None, None, a, lib.F32, 1, 1, 0, 0.0, a, 2, 2, rcas, sharp) == lib.EINVAL
    assert so.hdrtv_post_rgb48_fsr(None, None, a, lib.F32, 1, 1, 0, 0.0, a, 3, 2, 0, 0.2) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)          # bad arguments with a live context: tests/test_gpu_rgb48_fsr.py
