"""Film grain, host side (no GPU): the NumPy restatement tests/film_grain_ref.py against the values pinned with exactly its order of
operations -- bits, crc32, range, the identity at I * g = 0 over all 65536 codes, the seed hash's vectors --, the library's
hdrtv_film_grain_seed against it, and the Python surface: lib.check_film_grain, the ``_grain`` plans of lib.ScaleOptions.plan, every
refused combination through the processor's plan, the worker and the dispatcher, and the command line."""
import ctypes
import zlib

import numpy as np
import pytest

import film_grain_ref as R

F = np.float32
SEED_VECTORS = [((0, 0), 0x00000000, 0.0), ((0, 1), 0x229DE055, 0.13522148), ((0, 2), 0x56047BAC, 0.33600587),
                ((1, 0), 0x46E6C454, 0.2769587), ((1234, 59), 0x0EEF4C80, 0.05833888), ((2 ** 32 - 1, 2 ** 32 - 1), 0xDB6474D6, 0.85700154)]


def test_pinned_grain_values():
    g = R.grain(33, 47, F(0.37))
    assert g.dtype == F and g.shape == (33, 47) and np.isfinite(g).all()
    assert g.min() == F(-0.49498796) and g.max() == F(0.49868122)
    bits = g.view(np.uint32)
    assert [int(bits[y, x]) for y, x in ((0, 0), (0, 46), (32, 0), (32, 46), (16, 23))] == \
        [0x3E1B8F7D, 0x3E8F3506, 0xBEE8DE5A, 0xBDE09666, 0xBEC339B5]
    assert zlib.crc32(g.astype("<f4").tobytes()) == 0x6D5781A7


def test_range_at_1080p_and_the_largest_move_of_a_code():
    g = R.grain(1080, 1920, 0.0)
    assert g.min() == F(-0.50000006) and g.max() == F(0.49978954) and abs(float(g.std()) - 0.2246) < 1e-4
    assert np.abs(g).max() <= F(0.50000006)
    # at the reference's intensity a code moves by at most +-328
    codes = np.full((1080, 1920, 3), 32768, np.uint16)
    d = R.apply(codes, 1080, 1920, 0.0, R.INTENSITY).astype(int) - 32768
    assert np.abs(d).max() <= 328 and d.min() < -300 and d.max() > 300
    assert (d[:, :, 0] == d[:, :, 1]).all() and (d[:, :, 0] == d[:, :, 2]).all()          # one g per pixel


def test_zero_intensity_returns_every_code():
    c = np.arange(65536, dtype=np.uint16).reshape(256, 256, 1).repeat(3, 2)
    assert np.array_equal(R.apply(c, 256, 256, F(0.37), 0.0), c)
    assert not np.array_equal(R.apply(c, 256, 256, F(0.37), 0.01), c)
    # the clamp: the ends of the range stay inside it
    for v in (0, 65535):
        out = R.apply(np.full((33, 47, 3), v, np.uint16), 33, 47, 0.0, 0.1)
        assert (out <= v).all() if v else (out >= 0).all()
        assert (out == v).any() and (out != v).any()


def test_no_denormal_and_the_denominator_is_bounded():
    tiny = np.finfo(F).tiny
    for h, w, s in ((33, 47, F(0.37)), (270, 480, 0.0), (64, 128, np.nextafter(F(1), F(0)))):
        px = (np.arange(w, dtype=F) + F(0.5)) / F(w)
        assert (px >= tiny).all()
        g = R.grain(h, w, s)
        assert ((g == 0) | (np.abs(g) >= tiny)).all()
    q = np.linspace(-0.475, 0.475, 100001).astype(F)
    r = q * q
    assert ((r * r + R.B1 * r) + R.B0).min() >= F(0.011)


def test_seed_vectors():
    for args, h, s in SEED_VECTORS:
        assert R.seed_hash(*args) == h, args
        got = R.seed(*args)
        assert got.dtype == F and got == F(s) and 0.0 <= got < 1.0, args
    assert R.seed(0, 2 ** 32 + 1) == R.seed(0, 1)              # the index enters mod 2^32


def test_library_seed_equals_the_restatement():
    from hdrtv_mi355x import lib as L
    for args, _, s in SEED_VECTORS:
        assert F(L.film_grain_seed(*args)) == R.seed(*args) == F(s), args
    rng = np.random.default_rng(5)
    for a, b in rng.integers(0, 2 ** 32, (200, 2)):
        assert F(L.film_grain_seed(int(a), int(b))) == R.seed(int(a), int(b))
    for bad in (-1, 2 ** 32, 1.5, "7", None, True):
        with pytest.raises(ValueError):
            L.film_grain_seed(bad, 0)


def test_the_quantiser_rounds_the_same_fused_or_not():
    """csrc/film_grain.hip and its two sibling files are built without contraction, their twins with it: quant_u16's x * 65535 + 0.5
    must truncate to the same code either way, or a fused grain kernel would start from other codes than its twin writes."""
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.random(1 << 20).astype(F), np.arange(0, 0x3C01, dtype=np.uint16).view(np.float16).astype(F),
                        (np.arange(65536) / 65535.0).astype(F), np.nextafter((np.arange(1, 65536) - 0.5).astype(F) / F(65535), F(0))])
    two = (x * F(65535) + F(0.5)).astype(np.int32)
    one = (x.astype(np.float64) * 65535.0 + 0.5).astype(F).astype(np.int32)      # the product is exact in double: one rounding
    assert np.array_equal(one, two)


def test_the_kernel_header_states_the_rule_once():
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hdr-realtime-video-pipeline_amd", "csrc")
    src = open(os.path.join(csrc, "film_grain.h")).read()
    # s = c / 65535 is post_fsr.hip's sample, shown equal to the correctly rounded quotient by tests/test_rgb48_fsr_host.py
    assert "__fmaf_rn(__fmaf_rn(-q, 65535.f, x), r, q)" in src and "(float)(1.0 / 65535.0)" in src
    for banned in ("__fdividef", "__frcp_rn", "__builtin_amdgcn_rcp", "__fmaf_rn(34", "fmaf("):
        assert banned not in src, banned
    assert sum(ln.split("//")[0].count("__fdiv_rn") for ln in src.splitlines()) == 5      # px, py, permute's / 289, / 41, num / den
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(BUILD)/film_grain.o $(BUILD)/post_scale_grain.o $(BUILD)/post_fsr_grain.o: CXXFLAGS += -ffp-contract=off" in mk
    for name in ("film_grain.hip", "post_scale_grain.hip", "post_fsr_grain.hip"):
        assert " %s " % name in mk, name
        assert "__fdiv_rn" not in open(os.path.join(csrc, name)).read(), name          # the rule lives in film_grain.h alone
    text = open(os.path.join(os.path.dirname(csrc), "..", "include", "hdrtv_mi355x.h")).read()
    for v in ("hdrtv_film_grain_seed", "hdrtv_rgb48_film_grain", "hdrtv_post_rgb48_grain", "hdrtv_post_rgb48_scaled_grain",
              "hdrtv_post_rgb48_fsr_grain", "0.255121822830526", "0x9E3779B1", "0x735A2D97", "tests/film_grain_ref.py", "UNPINNED",
              "fract(t / 289) * 289", "G at the clamped position"):
        assert v in text, v


def test_check_film_grain():
    from hdrtv_mi355x import lib as L
    assert L.FILM_GRAIN_INTENSITY == 0.01 == R.INTENSITY
    assert L.check_film_grain(False) == 0.0 and L.check_film_grain(0) == 0.0 and L.check_film_grain(0.0) == 0.0
    assert L.check_film_grain(True) == 0.01 and L.check_film_grain() == 0.0
    for v in (0.01, 0.1, 0.025, np.float32(0.05), 1e-4):
        assert L.check_film_grain(v) == float(v)
    for bad in ("1", "on", None, float("nan"), float("inf"), -0.01, 0.11, 1, 2, [0.01], b"1"):
        with pytest.raises(ValueError):
            L.check_film_grain(bad)
    for bad in (1.0, -0.1, float("nan"), "x", None, True):
        with pytest.raises(ValueError):
            L.check_grain_seed(bad)
    assert L.check_grain_seed(0) == 0.0 and L.check_grain_seed(np.nextafter(F(1), F(0))) < 1.0


def test_the_plan_gets_the_grain_entries_and_is_unchanged_at_zero():
    from hdrtv_mi355x import lib as L
    lan, fsr = L.scale_options(), L.scale_options(scaler="fsr")
    sizes = (96, 64, 192, 128)
    # off: the plans of before, whatever spelling of "off"
    for off in ((), (0.0, 0.0), (False, 0.5), (0, 0.25)):
        assert lan.plan(*sizes, *off) == L.ScalePlan("hdrtv_post_rgb48_scaled", ())
        assert L.scale_options(antiring=0.3).plan(*sizes, *off) == L.ScalePlan("hdrtv_post_rgb48_scaled_ex", (77,))
        assert L.scale_options(cas=0.22, antiring=0.3).plan(*sizes, *off) == L.ScalePlan("hdrtv_post_rgb48_scaled_cas", (77, 3426))
        assert fsr.plan(*sizes, *off) == L.ScalePlan("hdrtv_post_rgb48_fsr", (1, 0.2))
        assert L.scale_options(scaler="ssim_superres").plan(*sizes, *off) == L.ScalePlan("hdrtv_post_rgb48_ssimsr", (1,))
        assert L.scale_options(downscaler="ssim").plan(96, 64, 48, 32, *off) == L.ScalePlan("hdrtv_post_rgb48_down", (0, 1))
        assert lan.plan(96, 64, 96, 64, *off) is None
    # on: the _grain entry with the two extra arguments
    assert lan.plan(*sizes, True, 0.25) == L.ScalePlan("hdrtv_post_rgb48_scaled_grain", (0, 0, 0.01, 0.25))
    assert L.scale_options(antiring=0.3).plan(*sizes, 0.05, 0.5) == L.ScalePlan("hdrtv_post_rgb48_scaled_grain", (77, 0, 0.05, 0.5))
    assert L.scale_options(cas="auto", antiring="auto").plan(*sizes, 0.1, 0.0) == \
        L.ScalePlan("hdrtv_post_rgb48_scaled_grain", (77, 3426, 0.1, 0.0))
    assert fsr.plan(*sizes, True, 0.75) == L.ScalePlan("hdrtv_post_rgb48_fsr_grain", (1, 0.2, 0.01, 0.75))
    assert L.scale_options(scaler="fsr", fsr_sharpness=None).plan(*sizes, 0.02, 0.0) == \
        L.ScalePlan("hdrtv_post_rgb48_fsr_grain", (0, 0.0, 0.02, 0.0))
    assert lan.plan(96, 64, 96, 64, True, 0.5) is None                             # nothing scaled: hdrtv_post_rgb48_grain, no plan
    with pytest.raises(ValueError):
        fsr.plan(96, 64, 250, 150, True, 0.0)                                      # the scaler's own limits still hold
    for bad_seed in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            lan.plan(*sizes, True, bad_seed)
    with pytest.raises(ValueError):
        lan.plan(*sizes, 0.2, 0.0)


REFUSED = [dict(scaler="spline36"), dict(scaler="ssim_superres"), dict(downscaler="mitchell"), dict(downscaler="ssim")]


def test_every_refused_combination():
    from hdrtv_mi355x import lib as L
    for kw in REFUSED:
        name = "downscaler" if "downscaler" in kw else "scaler"
        with pytest.raises(ValueError, match=f"film_grain does not go with {name}"):
            L.check_grain_chain(True, **kw)
        assert L.check_grain_chain(False, **kw) == 0.0                             # off: nothing to refuse
        opts = L.scale_options(**kw)
        sizes = (96, 64, 48, 32) if "downscaler" in kw else (96, 64, 192, 128)
        with pytest.raises(ValueError, match="film_grain"):
            opts.plan(*sizes, True, 0.0)
        assert opts.plan(*sizes) is not None
    with pytest.raises(ValueError, match="deband"):
        L.check_grain_chain(0.01, deband=True)
    assert L.check_grain_chain(True, "fsr") == 0.01 and L.check_grain_chain(0.05, "lanczos", None, False) == 0.05


def test_worker_validates(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, **{"out_w": 192, "out_h": 128, **kw})      # noqa: E731
    wk = mk()
    assert wk._film_grain == 0.0 and wk._grain_stream_seed == 0
    wk = mk(film_grain=True, grain_stream_seed=1234)
    assert wk._film_grain == 0.01 and wk._grain_stream_seed == 1234
    assert mk(film_grain=0.05, scaler="fsr")._film_grain == 0.05
    assert mk(film_grain=True, out_pix_fmt="p010le", dither="ordered")._film_grain == 0.01          # a dither behind the grain is fine
    for kw in REFUSED:
        sizes = dict(out_w=48, out_h=32) if "downscaler" in kw else {}
        mk(**kw, **sizes)
        with pytest.raises(ValueError, match="film_grain"):
            mk(film_grain=True, **kw, **sizes)
    for kw in (dict(film_grain=True, deband=True), dict(film_grain=0.5), dict(film_grain="1"), dict(film_grain=True, grain_stream_seed=-1),
               dict(film_grain=True, grain_stream_seed=2 ** 32), dict(grain_stream_seed=1.5)):
        with pytest.raises(ValueError):
            mk(**kw)


def _echo_worker(rank, device_index, init_args):
    keys = sorted(init_args)
    g, s = init_args.get("film_grain", "absent"), init_args.get("grain_stream_seed", "absent")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = len(keys)
        out.flat[1] = 9999 if g == "absent" else int(round(float(g) * 10000))
        out.flat[2] = 9999 if s == "absent" else int(s)
    return process


def test_dispatcher_validates_and_hands_the_grain_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    from hdrtv_mi355x import lib as L
    h, w = 6, 10
    run = dict(make_worker=_echo_worker, slots=2, numa=False, out_height=12, out_width=20)
    bad =[dict(film_grain=True, **kw) for kw in REFUSED[:2]] + [dict(film_grain=True, deband=True), dict(film_grain=0.2),
                                                                  dict(film_grain="on"), dict(film_grain=True, grain_stream_seed=-3)]
    for kw in bad:
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, **{**run, **kw})
    with pytest.raises(ValueError, match="film_grain"):
        D.FrameDispatcher(1, h, w, lambda i, v: None, make_worker=_echo_worker, slots=2, numa=False, out_height=3, out_width=5,
                          downscaler="ssim", film_grain=True)
    for kw, want in (({}, [1, 9999, 9999]), ({"film_grain": False, "grain_stream_seed": 77}, [1, 9999, 9999]),      # off: init_args keep their keys
                     ({"film_grain": True}, [3, 100, 0]), ({"film_grain": 0.05, "grain_stream_seed": 4321, "scaler": "fsr"}, [5, 500, 4321])):
        got = {}
        with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args={"marker": 1}, **kw, **run) as d:
            assert d.film_grain == L.check_film_grain(kw.get("film_grain", False)) and d.grain_stream_seed == kw.get("grain_stream_seed", 0)
            d.submit(np.zeros((h, w, 3), np.uint8))
            d.flush(timeout=60)
        assert d.exit_codes == [0] and got[0].reshape(-1)[:3].tolist() == want, kw


def test_playback_command_line():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    big = base + ["--out-size", "192x128"]
    a = P.parse_args(base)
    assert a.film_grain == 0.0 and a.film_grain_seed == 0                                        # off by default
    assert P.parse_args(base + ["--film-grain", "0"]).film_grain == 0.0
    a = P.parse_args(base + ["--film-grain", "1"])
    assert a.film_grain == 0.01 and a.film_grain_seed == 0                                       # the reference's flag and intensity
    a = P.parse_args(big + ["--film-grain", "1", "--film-grain-intensity", "0.05", "--film-grain-seed", "1234"])
    assert a.film_grain == 0.05 and a.film_grain_seed == 1234
    assert P.parse_args(big + ["--film-grain", "1", "--scaler", "fsr"]).film_grain == 0.01
    assert P.parse_args(big + ["--film-grain", "1", "--cas", "auto", "--antiring", "auto"]).film_grain == 0.01
    assert P.parse_args(base + ["--film-grain", "1", "--out-pix-fmt", "p010le", "--dither", "floyd_steinberg", "--light-level"]).film_grain == 0.01
    assert P.parse_args(base + ["--film-grain", "0", "--film-grain-seed", "5"]).film_grain == 0.0
    assert P.parse_args(base + ["--film-grain", "1", "--film-grain-intensity", "0"]).film_grain == 0.0
    bad = [base + ["--film-grain-intensity", "0.05"], base + ["--film-grain", "0", "--film-grain-intensity", "0.05"],      # belongs to --film-grain 1
           base + ["--film-grain", "2"], base + ["--film-grain", "on"], base + ["--film-grain", "1", "--film-grain-intensity", "0.2"],
           base + ["--film-grain", "1", "--film-grain-intensity", "-0.01"], base + ["--film-grain", "1", "--film-grain-intensity", "nan"],
           base + ["--film-grain", "1", "--film-grain-intensity", "x"], base + ["--film-grain", "1", "--film-grain-seed", "-1"],
           base + ["--film-grain", "1", "--film-grain-seed", str(2 ** 32)], base + ["--film-grain", "1", "--film-grain-seed", "1.5"],
           base + ["--film-grain", "1", "--deband"],
           big + ["--film-grain", "1", "--scaler", "spline36"], big + ["--film-grain", "1", "--scaler", "ssim_superres"],
           base + ["--out-size", "48x32", "--film-grain", "1", "--downscaler", "mitchell"],
           base + ["--out-size", "48x32", "--film-grain", "1", "--downscaler", "ssim"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            P.parse_args(argv)
        assert e.value.code == 2, argv


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 96)(*([0xA5A5] * 96))
    a = ctypes.addressof(buf)
    for inten, seed in ((0.01, 0.0), (0.0, 0.0), (0.2, 0.0), (float("nan"), 0.0), (0.01, 1.0), (0.01, float("nan"))):      # a NULL context is refused whatever else is given
        assert so.hdrtv_rgb48_film_grain(None, None, a, 1, 1, inten, seed, a) == lib.EINVAL
        assert so.hdrtv_post_rgb48_grain(None, None, a, lib.F32, 1, 1, 0, 0.0, a, inten, seed) == lib.EINVAL
        assert so.hdrtv_post_rgb48_scaled_grain(None, None, a, lib.F32, 1, 1, 0, 0.0, a, 2, 2, 0, 0, inten, seed) == lib.EINVAL
        assert so.hdrtv_post_rgb48_fsr_grain(None, None, a, lib.F32, 1, 1, 0, 0.0, a, 2, 2, 1, 0.2, inten, seed) == lib.EINVAL
    assert all(v == 0xA5A5 for v in buf)
