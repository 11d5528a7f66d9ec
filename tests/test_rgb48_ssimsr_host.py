"""The spline36 / SSimSuperRes upscale of the RGB48 output (hdrtv_post_rgb48_ssimsr), the parts that need no GPU: known answers of
the NumPy restatement of the rule (tests/rgb48_ssimsr_ref.py), its tables, the reference over every frame of the device test, and
the host surface that carries the two scaler names (lib, the worker, the dispatcher, the playback command line)."""
import ctypes
import os

import numpy as np
import pytest

import rgb48_down_ref as D
import rgb48_ssimsr_ref as R
from test_gpu_rgb48_fsr import contents
from test_gpu_rgb48_ssimsr import SHAPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
f32 = np.float32
NAMES = ("spline36", "ssim_superres")


# ------------------------------------------------------------------------------------------------------------------- the rule
def test_spline36_phases_at_exactly_2x():
    start, q = R.stab(4, 8)
    a = [173, -1036, 4401, 14408, -1874, 312]
    assert q[0].tolist() == a and q[1].tolist() == a[::-1] and q[2].tolist() == a and q[7].tolist() == a[::-1]
    assert start.tolist() == [-3, -2, -2, -1, -1, 0, 0, 1]
    start, q = R.stab(1080, 2160)
    assert start[0] == -3 and start[-1] == 1077 and {tuple(r) for r in q.tolist()} == {tuple(a), tuple(a[::-1])}
    for n, m in ((37, 64), (33, 34), (1, 2), (24, 36)):
        start, q = R.stab(n, m)
        assert (q.sum(axis=1) == R.ONE).all() and np.diff(start).min() >= 0 and np.diff(start).max() <= 1
    assert R.spline36_w(0.0) == 1.0 and R.spline36_w(3.0) == 0.0 and R.spline36_w(-3.5) == 0.0
    for x in (1.0, 2.0):                                            # the pieces meet at zero, up to the rounding of the coefficients
        assert abs(R.spline36_w(x)) < 1e-15 and abs(R.spline36_w(-x)) < 1e-15


def test_a_flat_frame_returns_its_code():
    for v in sorted(set([0, 1, 2, 3, 32768, 33297, 65534, 65535] + list(range(0, 65536, 257)))):
        x = np.full((6, 7, 3), v, np.uint16)
        for dh, dw in ((12, 14), (9, 13), (7, 8)):
            for ssim in (False, True):
                assert (R.scale(x, dh, dw, ssim=ssim) == v).all(), (v, dh, dw, ssim)


def test_a_single_pixel_is_repeated_and_equal_sizes_return_the_codes():
    x = np.array([[[7, 30000, 65535]]], np.uint16)
    for ssim in (False, True):
        assert np.array_equal(R.scale(x, 2, 2, ssim=ssim), np.broadcast_to(x[0, 0], (2, 2, 3)))
        assert np.array_equal(R.scale(x, 1, 1, ssim=ssim), x)
    y = np.random.default_rng(2).integers(0, 65536, (5, 7, 3)).astype(np.uint16)
    assert np.array_equal(R.scale(y, 5, 7, ssim=True), y)


def test_stage_b_changes_almost_every_code_of_full_range_noise():
    x = np.random.default_rng(0).integers(0, 65536, (36, 52, 3)).astype(np.uint16)
    a, b = R.scale(x, 72, 104), R.scale(x, 72, 104, ssim=True)
    assert a.dtype == b.dtype == np.uint16 and a.shape == b.shape == (72, 104, 3)
    assert 0.95 < float((a != b).mean()) < 0.99


def test_low_resolution_tables():
    t = R.lowtab(4, 8)                                              # exact 2x: eight taps at +-0.25 .. +-1.75
    assert t["cnt"].tolist() == [8] * 4 and t["lo"].tolist() == [-3, -1, 1, 3] and t["w"].shape == (4, 8) and t["w"].dtype == np.float32
    assert all(xs == [-1.75, -1.25, -0.75, -0.25, 0.25, 0.75, 1.25, 1.75] for xs in t["x"])
    assert t["b0"].tolist() == [0, 2, 4, 6] and t["f"].tolist() == [0.5] * 4
    assert np.array_equal(t["w"][0], t["w"][0][::-1]) and abs(float(t["w"][0].astype(np.float64).sum()) - 1) < 1e-6
    worst = 0
    for n, m in ((1080, 2160), (37, 64), (53, 101), (33, 34), (70, 71), (24, 36), (17, 33), (33, 65), (1, 2), (2, 3), (3, 4), (5, 9), (100, 199)):
        t = R.lowtab(n, m)
        assert 1 <= t["cnt"].min() and t["cnt"].max() <= R.MAX_LOW_TAPS, (n, m)
        assert (np.diff(t["lo"]) >= 0).all() and (t["f"] >= 0).all() and (t["f"] < 1).all()
        for j in range(n):
            lo, hi, _, xs = D.footprint(m, n, j)                    # the shrinking rule's footprint, from the high extent to the low one
            assert (lo, hi - lo + 1) == (t["lo"][j], t["cnt"][j]) and max(abs(x) for x in xs) <= 2.0
            assert not t["w"][j, t["cnt"][j]:].any()
        worst = max(worst, int(t["cnt"].max()))
    assert worst == 8             # the bound is 9 = 4 r + 1 integers in a span of 4 r <= 8; nine would need both ends on integers at r = 2
    assert R.mn_w(0.0) == 1.0 - 0.334 / 3.0 and abs(R.mn_w(2.0)) < 1e-15


def test_final_tables():
    t = R.fintab(24, 36)                                            # 1.5x: p = (d + 0.5) / 1.5 - 0.5 hits .5 at d = 1, 4, 7, ...
    assert t["ip"][:6].tolist() == [0, 1, 1, 2, 3, 3] and t["off"][1] == -0.5 and t["off"][4] == -0.5      # the tie goes up
    for n, m in ((24, 36), (37, 64), (33, 34), (1, 2), (1080, 2160), (17, 33)):
        t = R.fintab(n, m)
        assert (t["off"] >= -0.5).all() and (t["off"] < 0.5).all() and t["ip"].min() >= 0 and t["ip"].max() <= n - 1
        assert np.diff(t["ip"]).min() >= 0 and np.diff(t["ip"]).max() <= 1 and t["kern"].dtype == np.float32
        assert (t["kern"][:, 1] >= f32(np.cos(np.pi / 6))).all() and (t["kern"] >= 0).all()
    t = R.fintab(4, 8)
    assert t["ip"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and t["off"].tolist() == [-0.25, 0.25] * 4
    assert t["kern"][0].tolist() == [f32(np.cos(np.pi * -0.75 / 3)), f32(np.cos(np.pi * 0.25 / 3)), f32(np.cos(np.pi * 1.25 / 3))]


def test_refused_sizes():
    x = np.zeros((4, 6, 3), np.uint16)
    for dh, dw in ((9, 12), (8, 13), (3, 12), (8, 5), (4, 12), (8, 6), (4, 5), (0, 0)):
        for ssim in (False, True):
            with pytest.raises(ValueError):
                R.scale(x, dh, dw, ssim=ssim)
    assert R.scale(x, 8, 12, ssim=True).shape == (8, 12, 3) and R.scale(x, 5, 7).dtype == np.uint16


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_the_reference_is_finite_on_every_frame_of_the_device_test(src, dst):
    """No NaN anywhere, every denominator positive: Lr.a >= 1e-6 up to the two roundings of the linear fetch (both of its terms are
    floored at 5e-7), both variances >= 1e-6, the weight sum Ws > 0.  The float tensors
    of the device test are quantised here by the plain rule; the PQ codes of the same tensors are other integers of the same kind."""
    (h, w), (dh, dw) = src, dst
    low = np.inf
    for name, t in contents(h, w).items():
        codes = R.quant(np.clip(t, 0, 1).transpose(1, 2, 0))
        p = R.spline36(codes, dh, dw)
        lr = R.lowres(p, h, w)
        vl, vh = R.var(codes, lr)
        pix, ws = R.final_parts(codes, p, lr, vl, vh)
        for a in (lr, vl, vh, pix, ws):
            assert a.dtype == np.float32 and np.isfinite(a).all(), name
        assert (lr[..., 3] >= f32(1e-6) * (1 - f32(2.0 ** -22))).all() and (vl >= f32(1e-6)).all() and (vh >= f32(1e-6)).all() and (ws > 0).all(), name
        assert (pix >= 0).all() and (pix <= 1).all()
        low = min(low, float(ws.min()))
    print("%dx%d -> %dx%d: smallest Ws %.4f" % (h, w, dh, dw, low))


def test_header_makefile_and_kernel_state_the_rule():
    text = open(os.path.join(REPO, "include", "hdrtv_mi355x.h")).read()
    for v in ("hdrtv_post_rgb48_ssimsr", "uint16_t *dst, int dH, int dW, int ssim);", "13/11 x - 453/209", "-6/11 y + 270/209", "1/11 y - 45/209",
              "(0.2126 (r r) + 0.7152 (g g)) + 0.0722 (b b)", "B = 0.334, C = 0.333", "float32(5e-7)", "float32(1e-6)", "floor(p + 0.5)",
              "cos(pi (t - off) / 3)", "-1.5 * sqrt(vL[g] / (vH[g] + mV))", "(-1 - R) * c0", "H < dH <= 2 H and W < dW <= 2 W",
              "tests/rgb48_ssimsr_ref.py", "gui_scaling.py:42-43", "UNPINNED", "_is_upscale_required"):
        assert v in text, v
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " post_ssimsr.hip " in mk and "$(BUILD)/post_ssimsr.o: CXXFLAGS += -ffp-contract=off" in mk
    assert any("post_ssimsr.o" in ln and ln.rstrip().endswith(": post_quant.h") for ln in mk.splitlines())
    src = open(os.path.join(CSRC, "post_ssimsr.hip")).read()
    for banned in ("__fdividef", "__frcp_rn", "rsqrtf", "__builtin_amdgcn_rcp", "__builtin_amdgcn_rsq", "__builtin_amdgcn_sqrt", "cosf", "__cosf"):
        assert banned not in src, banned
    for v in ("__fmul_rn", "__fadd_rn", "__fsub_rn", "__fdiv_rn", "post_quant.h"):
        assert v in src, v


# ------------------------------------------------------------------------------------------------------------------- the options
def test_lib_names_sizes_and_symbol():
    from hdrtv_mi355x import lib as L
    assert L.UPSCALERS == ("lanczos", "fsr", "spline36", "ssim_superres") and L.SCALERS == ("lanczos", "fsr") and L.SSIMSR_MAX_RATIO == 2
    assert [L.check_scaler(s) for s in ("spline36", "SSIM_SuperRes", "Spline36", "fsr", "lanczos")] == ["spline36", "ssim_superres", "spline36", "fsr", "lanczos"]
    for bad in (None, True, 0, "", "ssim", "ssimsuperres", "spline64", "ewa", b"spline36", ["spline36"]):
        with pytest.raises(ValueError):
            L.check_scaler(bad)
    ex = dict((n, a) for n, _, a in L.SYMBOLS)
    assert ex["hdrtv_post_rgb48_ssimsr"] == ex["hdrtv_post_rgb48_scaled"] + [ctypes.c_int]
    for ok in ((1920, 1080, 3840, 2160), (96, 64, 96, 64), (96, 64, 97, 65), (1, 1, 2, 2), (70, 33, 71, 34)):
        L.check_ssimsr_size(*ok)
    for bad in ((96, 64, 193, 128), (96, 64, 192, 129), (960, 540, 3840, 2160), (1, 1, 3, 2)):
        with pytest.raises(ValueError, match="2x"):
            L.check_ssimsr_size(*bad)
    with pytest.raises(ValueError, match="192x128"):
        L.check_ssimsr_size(96, 64, 250, 150)
    for bad in ((96, 64, 96, 128), (96, 64, 192, 64)):
        with pytest.raises(ValueError, match="both axes"):
            L.check_ssimsr_size(*bad)
        with pytest.raises(ValueError, match="2x"):                 # the message names the limit too
            L.check_ssimsr_size(*bad)
    with pytest.raises(ValueError, match="below"):
        L.check_ssimsr_size(96, 64, 95, 128)


def test_cas_antiring_and_downscalers_under_the_new_names():
    from hdrtv_mi355x import lib as L
    for s in NAMES:
        assert L.scaler_options(s) == (0.0, 0.0) and L.scaler_options(s.upper(), "auto", "AUTO") == (0.0, 0.0) and L.scaler_options(s, 0, 0.0) == (0.0, 0.0)
        for kw in (dict(antiring=0.3), dict(cas=0.2), dict(antiring=1, cas="auto"), dict(antiring="auto", cas=1e-3)):
            with pytest.raises(ValueError, match="lanczos"):
                L.scaler_options(s, **kw)
        for kw in (dict(antiring=True), dict(cas="on"), dict(antiring=1.5)):
            with pytest.raises(ValueError):
                L.scaler_options(s, **kw)
        for down in ("mitchell", "ssim"):
            with pytest.raises(ValueError, match="enlarges"):
                L.down_options(down, 0.0, 96, 64, 48, 32, s)
        assert L.down_options(None, 0.0, 96, 64, 192, 128, s) is None
    assert L.scaler_options("lanczos", "auto", 0.2) == ("auto", 0.2)            # untouched


def test_worker_validates(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, **{"out_w": 192, "out_h": 128, **kw})      # noqa: E731
    for s in NAMES:
        wk = mk(scaler=s.upper(), cas="auto", antiring="auto")
        assert (wk._scaler, wk._cas, wk._antiring) == (s, 0.0, 0.0)
        assert mk(scaler=s, out_w=96, out_h=64)._scaler == s                       # nothing enlarged: nothing to refuse
        assert mk(scaler=s, out_w=97, out_h=65)._scaler == s
        for kw in (dict(cas=0.2), dict(antiring=0.3), dict(out_w=193), dict(out_h=129), dict(out_w=250, out_h=150), dict(out_w=96), dict(out_h=64),
                   dict(downscaler="ssim", out_w=48, out_h=32)):
            with pytest.raises(ValueError):
                mk(scaler=s, **kw)
    with pytest.raises(ValueError):
        mk(scaler="ssim")


def _echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    s = init_args.get("scaler")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = {None: 7, "fsr": 1, "spline36": 3, "ssim_superres": 4}.get(s, 2)
        out.flat[2] = 1 if "fsr_sharpness" in keys else 0
        out.flat[3] = 1 if "cas" in keys or "antiring" in keys else 0
    return process


def test_dispatcher_validates_and_hands_the_scaler_to_its_workers():
    from hdrtv_mi355x import dispatch as Dp
    h, w = 6, 10
    run = dict(make_worker=_echo_worker, slots=2, numa=False, out_height=12, out_width=20)
    for s in NAMES:
        for kw in (dict(cas=0.2), dict(antiring=0.3), dict(out_width=21), dict(out_height=13), dict(out_width=10), dict(out_height=6)):
            with pytest.raises(ValueError):
                Dp.FrameDispatcher(1, h, w, lambda i, v: None, **{**run, "scaler": s, **kw})
    for kw, want in (({"scaler": "spline36"}, [2, 3, 0, 0]), ({"scaler": "SSIM_SUPERRES", "cas": "auto", "antiring": "auto"}, [2, 4, 0, 0]),
                     ({}, [1, 7, 0, 0]), ({"scaler": "lanczos"}, [1, 7, 0, 0])):                   # off: init_args keep their keys
        got = {}
        with Dp.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **kw, **run) as d:
            assert d.scaler == kw.get("scaler", "lanczos").lower() and d._out_b == 12 * 20 * 6
            assert d.cas == 0.0 and d.antiring == 0.0
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:4].tolist() == want, kw


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    big = base + ["--out-size", "192x128"]
    for s in NAMES:
        a = P.parse_args(big + ["--scaler", s])
        assert (a.scaler, a.cas, a.antiring, a.out_wh) == (s, 0.0, 0.0, (192, 128))
        a = P.parse_args(big + ["--scaler", s, "--cas", "auto", "--antiring", "auto"])
        assert a.cas == 0.0 and a.antiring == 0.0
        assert P.parse_args(base + ["--out-size", "100x99", "--scaler", s]).out_wh == (100, 99)
        bad = [base + ["--scaler", s], base + ["--out-size", "96x64", "--scaler", s],            # nothing is enlarged
               base + ["--out-size", "193x128", "--scaler", s], base + ["--out-size", "192x129", "--scaler", s],      # more than 2x
               base + ["--out-size", "96x128", "--scaler", s], base + ["--out-size", "192x64", "--scaler", s],        # one axis at identity
               big + ["--scaler", s, "--cas", "0.2"], big + ["--scaler", s, "--antiring", "0.3"], big + ["--scaler", s, "--fsr-sharpness", "0.2"],
               big + ["--scaler", s.upper()], base + ["--out-size", "48x32", "--scaler", s, "--downscaler", "ssim"]]
        for argv in bad:
            with pytest.raises(SystemExit) as e:
                P.parse_args(argv)
            assert e.value.code == 2, argv
    assert P.parse_args(big).scaler == "lanczos" and P.parse_args(big + ["--scaler", "fsr"]).fsr_sharpness == 0.2


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    for ssim in (0, 1, 2, -1):            # a NULL context is refused whatever else is given
        for dh, dw in ((2, 2), (1, 1), (3, 2), (1, 2)):
            assert so.hdrtv_post_rgb48_ssimsr(None, None, a, lib.F32, 1, 1, 0, 0.0, a, dh, dw, ssim) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)          # bad arguments with a live context: tests/test_gpu_rgb48_ssimsr.py
