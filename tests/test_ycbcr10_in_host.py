"""10-bit Y'CbCr input (P010, yuv420p10le, yuv422p10le) on the host side: the conversion rule of include/hdrtv_mi355x.h
(tests/ycbcr10_in_ref.py) against its stated coefficient table, known answers, the exact double formula and hand-worked upsampling;
10-bit framing in RawVideoSource, the worker and FrameDispatcher; the playback CLI flags; the C entry points' refusal of a NULL
context."""
import ctypes

import numpy as np
import pytest

import ycbcr10_in_ref as R

PAIRS = [(m, full) for m in (709, 601, 2020) for full in (False, True)]


def test_coefficient_table_from_kr_kb():
    table = {(709, False): (76533, 14729, 1752, 4378, 17356), (709, True): (65536, 12901, 1535, 3835, 15201),
             (601, False): (76533, 13113, 3219, 6679, 16574), (601, True): (65536, 11485, 2819, 5850, 14516),
             (2020, False): (76533, 13792, 1539, 5344, 17597), (2020, True): (65536, 12080, 1348, 4681, 15412)}
    for (m, full), want in table.items():
        assert R.coefficients(m, full) == want, (m, full)


def test_known_answers_709_limited_constant_frames():
    known = {(64, 512, 512): (0, 0, 0), (940, 512, 512): (1023, 1023, 1023), (502, 512, 512): (511, 511, 511),
             (64, 64, 960): (805, 0, 0), (250, 240, 640): (447, 207, 0), (0, 512, 512): (0, 0, 0),
             (1023, 512, 512): (1023, 1023, 1023)}
    for (y, u, v), rgb in known.items():
        r, g, b = R.matrix_rgb(np.array([y]), np.array([8 * u]), np.array([8 * v]), 709, False)
        assert (int(r[0]), int(g[0]), int(b[0])) == rgb, (y, u, v)
        for fmt in R.PIX_FMTS:                       # and through the whole-frame path, in every layout
            hc = 4 if fmt == "yuv422p10le" else 2
            f = R.from_values(np.full((4, 6), y), np.full((hc, 3), u), np.full((hc, 3), v), fmt)
            assert f.shape == R.frame_shape(fmt, 4, 6)
            out = R.to_rgb10(f, fmt)
            assert out.shape == (4, 6, 3) and out.dtype == np.uint16 and (out.reshape(-1, 3) == rgb).all(), (fmt, y, u, v)


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_rule_is_within_0p57_code_of_the_double_formula(matrix, full):
    rng = np.random.default_rng(1000 * matrix + int(full))
    n = 200_000
    Y, U, V = rng.integers(0, 1024, n), rng.integers(0, 8 * 1023 + 1, n), rng.integers(0, 8 * 1023 + 1, n)
    got = R.matrix_rgb(Y, U, V, matrix, full)
    want = R.exact_rgb(Y, U, V, matrix, full)
    err = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want))
    print(f"matrix {matrix} full {full}: max |rule - exact| = {err:.4f} code")
    assert err <= 0.57


@pytest.mark.parametrize("fmt", R.PIX_FMTS)
def test_grey_frame_of_black_and_white_luma_is_exactly_0_and_1023(fmt):
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (12, 20))
    out = R.to_rgb10(R.grey_frame(np.where(bits, 940, 64), fmt), fmt)
    assert np.array_equal(out, np.repeat((bits * 1023).astype(np.uint16)[..., None], 3, axis=2))
    t = R.tensor_f16(out)
    assert set(np.unique(t).tolist()) == {0.0, 1.0}              # fp16(1023 * fp32(1/1023)) is 1


def test_all_1024_tensor_values_are_distinct():
    t = R.tensor_f16(np.arange(1024, dtype=np.uint16).reshape(1, 1024, 1).repeat(3, axis=2))
    assert len(np.unique(t[0])) == 1024 and np.all(np.diff(t[0, 0].astype(np.float32)) > 0)


def test_chroma_upsampling_by_hand():
    C = np.array([[10, 50], [90, 130]], np.uint16)               # 4:2:0: the 8-bit rule's integers (tests/test_yuv420_host.py)
    assert R.upsample8(C, 4, 4).tolist() == [[80, 240, 400, 400], [240, 400, 560, 560], [560, 720, 880, 880], [720, 880, 1040, 1040]]
    C = np.array([[10, 50], [90, 130], [7, 1000]], np.uint16)    # 4:2:2: every luma row has its chroma row, C8 = 4 (C[i] + C[i2])
    assert R.upsample8(C, 3, 4).tolist() == [[80, 240, 400, 400], [720, 880, 1040, 1040], [56, 4028, 8000, 8000]]


def test_sample_words_and_layouts():
    rng = np.random.default_rng(5)
    h, w = 6, 8
    Y = rng.integers(0, 1024, (h, w), dtype=np.uint16)
    for fmt in R.PIX_FMTS:
        hc = h if fmt == "yuv422p10le" else h // 2
        U, V = rng.integers(0, 1024, (hc, w // 2), dtype=np.uint16), rng.integers(0, 1024, (hc, w // 2), dtype=np.uint16)
        clean, noisy = R.from_values(Y, U, V, fmt), R.from_values(Y, U, V, fmt, rng)
        assert clean.shape == R.frame_shape(fmt, h, w) and not np.array_equal(clean, noisy)
        for f in (clean, noisy):                                  # the six unused bits of a word do not matter
            assert all(np.array_equal(R.values(p, fmt), v) for p, v in zip(R.split(f, fmt), (Y, U, V))), fmt
        assert np.array_equal(R.to_rgb10(clean, fmt, 601, True), R.to_rgb10(noisy, fmt, 601, True))
    # P010 carries the value in the high bits, CbCr interleaved; the planar layouts in the low bits, Cb plane then Cr plane
    f = R.from_values(np.full((2, 4), 1), np.full((1, 2), 2), np.full((1, 2), 3), "p010le")
    assert f.tolist() == [[64] * 4, [64] * 4, [128, 192, 128, 192]]
    f = R.from_values(np.full((2, 4), 1), np.full((1, 2), 2), np.full((1, 2), 3), "yuv420p10le")
    assert f.tolist() == [[1] * 4, [1] * 4, [2, 2, 3, 3]]
    # flat chroma: 3 C + C = 4 C, the two subsamplings give the same frame
    f420 = R.from_values(Y, np.full((3, 4), 300), np.full((3, 4), 700), "yuv420p10le")
    f422 = R.from_values(Y, np.full((6, 4), 300), np.full((6, 4), 700), "yuv422p10le")
    assert np.array_equal(R.to_rgb10(f420, "yuv420p10le"), R.to_rgb10(f422, "yuv422p10le"))


def test_frame_shape_helpers_and_value_errors():
    from hdrtv_mi355x import lib as L
    assert set(L.YCBCR10_IN_FORMATS) == set(R.PIX_FMTS) and all(L.YCBCR10_IN_FORMATS[k] == R.FMT[k] for k in R.PIX_FMTS)
    assert L.ycbcr10_frame_shape("p010le", 4, 6) == (6, 6) and L.ycbcr10_frame_shape("yuv420p10le", 4, 6) == (6, 6)
    assert L.ycbcr10_frame_shape("yuv422p10le", 3, 6) == (6, 6)                       # an odd height is fine for 4:2:2
    assert L.ycbcr10_frame_hw(np.zeros((6, 6), np.uint16), "yuv422p10le") == (3, 6)
    assert L.ycbcr10_frame_hw(np.zeros((6, 6), np.uint16), "p010le") == (4, 6)
    for bad in (("p010le", 3, 6), ("yuv420p10le", 4, 5), ("yuv422p10le", 4, 5), ("yuv444p10le", 4, 6), ("p010le", 0, 6)):
        with pytest.raises(ValueError):
            L.ycbcr10_frame_shape(*bad)
    for frame, fmt in ((np.zeros((6, 6), np.uint8), "p010le"), (np.zeros((6, 6, 3), np.uint16), "p010le"),
                       (np.zeros((5, 6), np.uint16), "yuv420p10le"), (np.zeros((6, 5), np.uint16), "p010le"),
                       (np.zeros((5, 6), np.uint16), "yuv422p10le"), (np.zeros((6, 6), np.uint16), "nv12")):
        with pytest.raises(ValueError):
            L.ycbcr10_frame_hw(frame, fmt)


@pytest.mark.parametrize("pix_fmt", R.PIX_FMTS)
def test_rawvideo_source_10bit_framing(tmp_path, pix_fmt):
    from hdrtv_mi355x import playback as P
    assert all(f in P.RawVideoSource.PIX_FMTS for f in R.PIX_FMTS) and P.RawVideoSource.PIX_FMTS[:3] == ("bgr24", "yuv420p", "nv12")
    w, h = 8, 6
    frames = [R.random_frame(h, w, seed=i, pix_fmt=pix_fmt) for i in range(3)]
    path = tmp_path / "clip.yuv"
    path.write_bytes(b"".join(f.astype("<u2").tobytes() for f in frames))
    src = P.RawVideoSource(str(path), w, h, 30.0, pix_fmt=pix_fmt, yuv_matrix=2020, yuv_full_range=True)
    assert (src.pix_fmt, src.yuv_matrix, src.yuv_full_range, src.frame_count) == (pix_fmt, 2020, True, 3)
    for f in frames:
        ok, g = src.read()
        assert ok and g.shape == R.frame_shape(pix_fmt, h, w) and g.dtype == np.uint16 and np.array_equal(g, f)
    assert src.read() == (False, None)
    src.release()
    (tmp_path / "odd.yuv").write_bytes(bytes(7 * 6 * 4))
    with pytest.raises(ValueError):
        P.RawVideoSource(str(tmp_path / "odd.yuv"), 7, 6, 30.0, pix_fmt=pix_fmt)     # odd width
    with pytest.raises(ValueError):                              # not a whole number of frames
        P.RawVideoSource(str(path), 10, 6, 30.0, pix_fmt=pix_fmt)
    # the prefetcher hands u16 frames on as they are, with the source's format
    pf = P.PinnedPrefetch(P.RawVideoSource(str(path), w, h, 30.0, pix_fmt=pix_fmt, yuv_matrix=601), upload=False)
    assert (pf.pix_fmt, pf.yuv_matrix, pf.yuv_full_range) == (pix_fmt, 601, False)
    got = []
    while True:
        ok, f = pf.read()
        if not ok:
            break
        got.append(np.array(f))
    pf.release()
    assert len(got) == 3 and all(g.dtype == np.uint16 and np.array_equal(g, f) for g, f in zip(got, frames))


def _standin_worker(rank, device_index, init_args):
    """CPU stand-in for a GPU worker that receives 10-bit slots: the rule on the host, into the RGB48 output slot."""
    fmt = init_args["fmt"]

    def process(frame, out):
        assert frame.dtype == np.uint16 and frame.shape == R.frame_shape(fmt, out.shape[0], out.shape[1])
        np.multiply(R.to_rgb10(frame, fmt), 64, out=out, dtype=np.uint16, casting="unsafe")
        out[0, 0, 1] = rank

    return process


@pytest.mark.parametrize("pix_fmt", ["p010le", "yuv422p10le"])
def test_dispatcher_10bit_slots_with_standin_workers(pix_fmt):
    from hdrtv_mi355x.dispatch import FrameDispatcher
    h, w, n = 8, 12, 5
    frames = [R.random_frame(h, w, seed=40 + i, pix_fmt=pix_fmt) for i in range(n)]
    shape = R.frame_shape(pix_fmt, h, w)
    got = {}
    with FrameDispatcher(2, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=_standin_worker, init_args={"fmt": pix_fmt},
                         slots=2, numa=False, pix_fmt=pix_fmt) as d:
        assert d._in_b == shape[0] * shape[1] * 2 and d._out_b == h * w * 6
        assert all(v.shape == shape and v.dtype == np.uint16 for v in d._ins[0])
        for i, f in enumerate(frames):
            if i % 2:
                d.submit(f)
            else:
                j, view = d.reserve()
                assert j == i and view.shape == shape and view.dtype == np.uint16
                view[...] = f
                d.commit()
        d.flush(timeout=60)
    assert sorted(got) == list(range(n))
    for i, f in enumerate(frames):
        want = R.to_rgb10(f, pix_fmt) * 64
        want[0, 0, 1] = i % 2
        assert np.array_equal(got[i], want), i
    with pytest.raises(ValueError):
        FrameDispatcher(1, 8, 11, lambda i, v: None, make_worker=_standin_worker, pix_fmt=pix_fmt)          # odd width
    with pytest.raises(ValueError):
        FrameDispatcher(1, 7, 12, lambda i, v: None, make_worker=_standin_worker, pix_fmt="yuv420p10le")    # odd height, 4:2:0
    with pytest.raises(ValueError):
        FrameDispatcher(1, 8, 12, lambda i, v: None, make_worker=_standin_worker, pix_fmt="yuv444p10le")


def test_playback_cli_flags(monkeypatch, tmp_path):
    from hdrtv_mi355x import playback as P
    import hdrtv_mi355x.worker as WK
    seen = {}

    class Stop(Exception):
        pass

    class FakeWorker:
        def __init__(self, *a, **k):
            pass

        def _load_model(self, key):
            raise Stop

    def fake_source(path, w, h, fps, **kw):
        seen.update(kw, size=(w, h))
        return P.SyntheticSource(w, h, fps, 2)

    fake_source.PIX_FMTS = P.RawVideoSource.PIX_FMTS             # --pix-fmt follows the real source's list
    monkeypatch.setattr(WK, "HeadlessPipelineWorker", FakeWorker)
    monkeypatch.setattr(P, "RawVideoSource", fake_source)
    for fmt in R.PIX_FMTS:
        with pytest.raises(Stop):
            P.main(["--weights-dir", str(tmp_path), "--size", "64x32", "--input", "x.yuv", "--pix-fmt", fmt, "--yuv-matrix", "2020",
                    "--yuv-range", "full", "--no-prefetch"])
        assert seen == {"pix_fmt": fmt, "yuv_matrix": 2020, "yuv_full_range": True, "size": (64, 32)}
    for bad in (["--pix-fmt", "yuv444p10le"], ["--pix-fmt", "p010be"]):
        with pytest.raises(SystemExit):
            P.main(["--weights-dir", str(tmp_path), "--input", "x.yuv"] + bad)


def test_worker_input_format_and_the_missing_letterbox():
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    w = HeadlessPipelineWorker("unused")
    for fmt in R.PIX_FMTS:
        w.set_input_format(fmt, 2020, True)
        assert w._yuv_format == {"pix_fmt": fmt, "matrix": 2020, "full_range": True}
    w.set_input_format("nv12", 601, True)                                              # the 8-bit form is what it was
    assert w._yuv_format == {"layout": "nv12", "matrix": 601, "full_range": True}
    for bad in ("bgr24", "yuv444p10le", "p010"):
        with pytest.raises(ValueError):
            w.set_input_format(bad)


def test_new_entry_points_refuse_a_null_context():
    from hdrtv_mi355x import lib
    so = lib.load()
    assert (lib.YCC_P010, lib.YCC_YUV420P10, lib.YCC_YUV422P10) == (0, 1, 2)
    buf = (ctypes.c_uint16 * 256)()
    p = ctypes.addressof(buf)
    assert so.hdrtv_ycbcr10_to_rgb10(None, None, p, 16, p, p, 8, lib.YCC_YUV420P10, 709, 0, 4, 8, p) == lib.EINVAL
    assert so.hdrtv_preprocess_ycbcr10(None, None, p, 16, p, p, 8, lib.YCC_YUV420P10, 709, 0, 4, 8, p, p) == lib.EINVAL
    assert so.hdrtv_last_error(None) == b"null context"
    assert not any(buf)
