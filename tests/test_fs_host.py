"""Floyd-Steinberg error diffusion of the 10-bit Y'CbCr output, the parts that need no GPU: what the rule (include/hdrtv_mi355x.h,
restated twice in tests/fs_ref.py) states about itself, and the argument checks of every layer that carries the new dither name --
lib.output_cleanup, the worker, the dispatcher, the playback command line and the C entry points' refusals that return before any
device call."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import fs_ref as F
import ycbcr10_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(f, s) for f in R.FORMATS for s in R.SITINGS if not (f == "yuv422p10le" and s == "topleft")]
SHAPES = [(1, 1), (2, 1), (5, 3), (70, 33), (33, 70)]
# the flat-plane levels in 1/4096 code: the luma extremes, their neighbours, and a dozen drawn once from default_rng(20261021)
FLAT_LEVELS = [0, 1, 876 * 4096 - 1, 876 * 4096,
               2749086, 771854, 2799349, 92915, 1379463, 585046, 2944577, 462512, 2356421, 186893, 198286, 1023295]


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("h,w", SHAPES)
def test_the_two_forms_agree(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    for lo, hi in ((0, 876), (-448, 448)):
        # beyond the k range on both sides, so that both clamps act
        u = rng.integers((lo - 2) * 4096, (hi + 2) * 4096 + 1, (h, w))
        a, ea = F.diffuse_scalar(u, lo, hi, with_error=True)
        b, eb = F.diffuse(u, lo, hi, with_error=True)
        assert np.array_equal(a, b) and ea == eb
        assert a.min() >= lo and a.max() <= hi


def test_carried_error_is_bounded_on_random_flat_and_saturated_planes():
    rng = np.random.default_rng(7)
    planes = [rng.integers(0, 876 * 4096 + 1, (40, 64)), np.full((40, 64), 2048), np.full((40, 64), 4096 * 300 + 2047),
              np.full((40, 64), -5 * 4096), np.full((40, 64), 900 * 4096), rng.integers(-4096 * 20, 4096 * 900, (40, 64))]
    for u in planes:
        _, emax = F.diffuse(u, 0, 876, with_error=True)
        assert emax <= F.E_BOUND == 2050, emax


def test_flat_luma_planes_keep_their_mean():
    """A condition on the reference: over a flat 48 x 80 plane the mean of k is within 32/4096 code of u (measured: at most
    22/4096, the loss being what falls off the right and bottom edges)."""
    assert len(FLAT_LEVELS) == 16 and all(0 <= v <= 876 * 4096 for v in FLAT_LEVELS)
    worst = 0.0
    for level in FLAT_LEVELS:
        k = F.diffuse(np.full((48, 80), level), 0, 876)
        worst = max(worst, abs(float(k.mean()) * 4096 - level))
    print(f"flat planes: worst |mean k - u| = {worst:.2f} / 4096 code")
    assert worst <= 32.0


@pytest.mark.parametrize("fmt,siting", COMBOS)
def test_sums_are_those_of_the_undithered_rule(fmt, siting):
    rgb = np.random.default_rng(3).integers(0, 65536, (6, 10, 3)).astype(np.uint16)
    (sy, shy), (su, shc), (sv, _) = F.sums(rgb, fmt, siting)
    assert shy == 20 and shc == {"yuv422p10le": 22}.get(fmt, 23 if siting == "left" else 24)
    assert np.array_equal(64 + ((sy + (1 << 19)) >> 20), R.luma(rgb))
    cb, cr = R.chroma(rgb, fmt, siting)
    assert np.array_equal(512 + ((su + (1 << (shc - 1))) >> shc), cb) and np.array_equal(512 + ((sv + (1 << (shc - 1))) >> shc), cr)
    # the samples stay inside the k range times 4096, so base + k needs no clamp on real codes
    assert F.samples(sy, shy).min() >= 0 and F.samples(sy, shy).max() <= 876 * 4096
    assert abs(F.samples(su, shc)).max() <= 448 * 4096 and abs(F.samples(sv, shc)).max() <= 448 * 4096


def test_planes_ranges_layout_and_share_of_changed_samples():
    rgb = np.random.default_rng(5).integers(0, 65536, (32, 48, 3)).astype(np.uint16)
    for fmt, siting in COMBOS:
        y, cb, cr = F.planes(rgb, fmt, siting)
        shl = 6 if fmt == "p010le" else 0
        assert (y >> shl).min() >= 64 and (y >> shl).max() <= 940 and (cb >> shl).min() >= 64 and (cr >> shl).max() <= 960
        assert F.pack(rgb, fmt, siting).size * 2 == R.frame_bytes(fmt, 32, 48)
        assert np.array_equal(F.pack(rgb, fmt, siting)[:32 * 48], y.reshape(-1))
    # saturated corners stay at the ends of the range
    white = np.full((4, 6, 3), 65535, np.uint16)
    y, cb, cr = F.planes(white, "yuv420p10le")
    assert (y == 940).all() and (cb == 512).all() and (cr == 512).all()
    y, cb, cr = F.planes(np.zeros((4, 6, 3), np.uint16), "yuv422p10le")
    assert (y == 64).all() and (cb == 512).all() and (cr == 512).all()
    # a rule of its own: on random input a good share of the samples differs from the plain rounding
    y, _, _ = F.planes(rgb, "yuv420p10le")
    share = float((y != R.luma(rgb)).mean())
    assert 0.05 < share < 0.25, share


# ---------------------------------------------------------------------------------------------------------------- validation
def test_output_cleanup_takes_the_new_name():
    from hdrtv_mi355x import lib as L
    c = L.output_cleanup(dither="Floyd_Steinberg", pix_fmt="yuv422p10le")
    assert tuple(c) == (False, 16, 1311, "floyd_steinberg") and c.active and c.error_diffusion and c.dither_code == L.DITHER_FS == 2
    assert c._fields == ("deband", "deband_range", "deband_threshold", "dither")            # OutputCleanup keeps its four fields
    assert not L.output_cleanup(dither="ordered").error_diffusion and not L.output_cleanup().error_diffusion
    back = pickle.loads(pickle.dumps(c))
    assert back == c and isinstance(back, L.OutputCleanup) and back.error_diffusion
    assert sorted(L.DITHERS) == ["floyd_steinberg", "none", "ordered"]
    for bad in ("error_diffusion", "fs", "floyd-steinberg", 2):
        with pytest.raises(ValueError):
            L.output_cleanup(dither=bad)
    with pytest.raises(ValueError):
        L.output_cleanup(dither="floyd_steinberg", pix_fmt="rgb48le")
    sym = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert sym["hdrtv_ycbcr10_fs_scratch_bytes"][0] is ctypes.c_int64
    assert len(sym["hdrtv_post_ycbcr10_fs"][1]) == 16 and len(sym["hdrtv_rgb48_to_ycbcr10_fs"][1]) == 13
    assert sym["hdrtv_post_ycbcr10_fs"][1][:15] == sym["hdrtv_post_ycbcr10"][1]               # the plain arguments, then the scratch
    assert sym["hdrtv_rgb48_to_ycbcr10_fs"][1][:12] == sym["hdrtv_rgb48_to_ycbcr10"][1]


def test_worker_takes_the_new_name_and_refuses_it_with_rgb48le(tmp_path):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    mk = lambda **kw: HeadlessPipelineWorker(str(tmp_path), proc_w=96, proc_h=64, **kw)      # noqa: E731
    w = mk(out_pix_fmt="yuv422p10le", deband=True, dither="floyd_steinberg")
    assert tuple(w._cleanup) == (True, 16, 1311, "floyd_steinberg") and w._cleanup.error_diffusion
    with pytest.raises(ValueError):
        mk(dither="floyd_steinberg")
    with pytest.raises(ValueError):
        mk(out_pix_fmt="rgb48le", dither="floyd_steinberg")
    with pytest.raises(ValueError):
        mk(out_pix_fmt="p010le", dither="error_diffusion")


def _fs_echo_worker(rank, device_index, init_args):
    c = init_args.get("cleanup")

    def process(frame, out):
        out[...] = 0
        out.flat[0] = 1 if c is not None and type(c) is tuple and c[3] == "floyd_steinberg" else 0
    return process


def test_dispatcher_takes_the_new_name_and_hands_it_to_its_workers():
    from hdrtv_mi355x import dispatch as D
    h, w = 6, 10
    with pytest.raises(ValueError):
        D.FrameDispatcher(1, h, w, lambda i, v: None, make_worker=_fs_echo_worker, numa=False, dither="floyd_steinberg")
    with pytest.raises(ValueError):
        D.FrameDispatcher(1, h, w, lambda i, v: None, make_worker=_fs_echo_worker, numa=False, out_pix_fmt="p010le", dither="error_diffusion")
    got = {}
    with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=_fs_echo_worker, slots=2, numa=False,
                           out_pix_fmt="yuv422p10le", dither="floyd_steinberg") as d:
        assert d._out_b == h * w * 4 and tuple(d.cleanup) == (False, 16, 1311, "floyd_steinberg")
        d.submit(np.zeros((h, w, 3), np.uint8))
        d.flush(timeout=60)
    assert d.exit_codes == [0] and got[0].reshape(-1)[0] == 1


def test_playback_command_line_takes_the_new_name():
    from hdrtv_mi355x import playback as P
    base = ["--weights-dir", "x", "--size", "96x64"]
    a = P.parse_args(base + ["--out-pix-fmt", "yuv422p10le", "--deband", "--dither", "floyd_steinberg"])
    assert tuple(a.cleanup) == (True, 16, 1311, "floyd_steinberg") and a.cleanup.error_diffusion
    for extra in (["--dither", "floyd_steinberg"], ["--out-pix-fmt", "rgb48le", "--dither", "floyd_steinberg"],
                  ["--out-pix-fmt", "p010le", "--dither", "error_diffusion"]):
        with pytest.raises(SystemExit) as e:
            P.parse_args(base + extra)
        assert e.value.code == 2, extra


def test_library_refuses_before_any_device_call():
    from hdrtv_mi355x import lib
    so = lib.load()
    buf = (ctypes.c_uint16 * 160)(*([0xA5A5] * 160))
    a = ctypes.addressof(buf)
    P, P420, P422 = lib.YCC_P010, lib.YCC_YUV420P10, lib.YCC_YUV422P10
    # a NULL context is refused whatever else is given, with a scratch and without one
    for scratch in (a + 128, None):
        assert so.hdrtv_post_ycbcr10_fs(None, None, a, lib.F32, 2, 4, 0, 0.0, P, 0, a, 8, a + 32, None, 8, scratch) == lib.EINVAL
        assert so.hdrtv_rgb48_to_ycbcr10_fs(None, None, a, 2, 4, P420, 0, a, 8, a + 32, a + 48, 4, scratch) == lib.EINVAL
    assert all(x == 0xA5A5 for x in buf)
    # the scratch: 4 (H W + 2 ch cw + W + 2 cw) bytes; negative for what the conversion refuses
    assert so.hdrtv_ycbcr10_fs_scratch_bytes(P, 4, 6) == 4 * (24 + 2 * 2 * 3 + 6 + 6)
    assert so.hdrtv_ycbcr10_fs_scratch_bytes(P420, 4, 6) == so.hdrtv_ycbcr10_fs_scratch_bytes(P, 4, 6)
    assert so.hdrtv_ycbcr10_fs_scratch_bytes(P422, 3, 6) == 4 * (18 + 2 * 3 * 3 + 6 + 6)
    assert so.hdrtv_ycbcr10_fs_scratch_bytes(P422, 2160, 3840) == 4 * (2 * 2160 * 3840 + 2 * 3840)
    for fmt, h, w in ((P, 3, 6), (P420, 3, 6), (P, 4, 5), (P422, 4, 5), (3, 4, 6), (-1, 4, 6), (P, 0, 6), (P, 4, 0), (P422, -2, 6)):
        assert so.hdrtv_ycbcr10_fs_scratch_bytes(fmt, h, w) < 0, (fmt, h, w)


# ---------------------------------------------------------------------------------------------------------------- constants
def test_constants_match_the_source_and_the_header():
    from hdrtv_mi355x import lib as L
    common = open(os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc", "common.h")).read()
    m = re.search(r"constexpr int FS_ROWS = (\d+), FS_CHUNK = (\d+);", common)
    assert m and (int(m.group(1)), int(m.group(2))) == (L.FS_ROWS, L.FS_CHUNK)
    header = open(os.path.join(REPO, "include", "hdrtv_mi355x.h")).read()
    assert re.search(r"#define HDRTV_FS_ROWS %d\b" % L.FS_ROWS, header) and re.search(r"#define HDRTV_FS_CHUNK %d\b" % L.FS_CHUNK, header)
    assert L.FS_ROWS % 64 == 0 and L.FS_ROWS % L.FS_CHUNK == 0


def test_header_states_the_rule_and_no_longer_excludes_it():
    text = open(os.path.join(REPO, "include", "hdrtv_mi355x.h")).read()
    for v in ("hdrtv_ycbcr10_fs_scratch_bytes", "hdrtv_post_ycbcr10_fs", "hdrtv_rgb48_to_ycbcr10_fs", "tests/fs_ref.py", "UNPINNED",
              "(7 r) >> 4", "(3 r) >> 4", "(5 r) >> 4", "r - a - b - c", "(v + 2048) >> 12", "rounds twice", "two scratches"):
        assert v in text, v
    assert "Out of scope: error-diffusion" not in text and "Out of scope: error diffusion" not in text
