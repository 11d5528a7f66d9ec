"""8-bit 4:2:0 input (I420, NV12) on the host side: the conversion rule of include/hdrtv_mi355x.h (tests/yuv420_ref.py)
against its stated coefficient table, known answers and a hand-worked upsampling case; 4:2:0 framing in RawVideoSource,
PinnedPrefetch and FrameDispatcher; the playback CLI flags; the new C entry points' argument checks on a NULL context."""
import ctypes

import numpy as np
import pytest

import yuv420_ref as R


def test_coefficient_table_from_kr_kb():
    table = {(601, False): (76309, 13075, 3209, 6660, 16525), (601, True): (65536, 11485, 2819, 5850, 14516),
             (709, False): (76309, 14686, 1747, 4366, 17305), (709, True): (65536, 12901, 1535, 3835, 15201),
             (2020, False): (76309, 13752, 1535, 5328, 17545), (2020, True): (65536, 12080, 1348, 4681, 15412)}
    for (m, full), want in table.items():
        assert R.coefficients(m, full) == want, (m, full)


def _rgb(y, u, v, full=False):
    r, g, b = R.matrix_rgb(np.array([y]), np.array([8 * u]), np.array([8 * v]), 709, full)
    return int(r[0]), int(g[0]), int(b[0])


def test_known_answers_709():
    assert _rgb(16, 128, 128) == (0, 0, 0)
    assert _rgb(235, 128, 128) == (255, 255, 255)
    assert _rgb(255, 128, 128, full=True) == (255, 255, 255)
    bars = {(168, 44, 136): (191, 191, 0), (145, 147, 44): (0, 191, 190), (134, 63, 52): (1, 192, 0),
            (63, 193, 204): (191, 0, 192), (51, 109, 212): (191, 0, 1), (28, 212, 120): (0, 0, 191)}
    for yuv, rgb in bars.items():
        assert _rgb(*yuv) == rgb, yuv
    # and through the whole-frame path: a flat frame of one bar converts to that bar everywhere, in both layouts
    for layout in ("i420", "nv12"):
        Y = np.full((4, 6), 134, np.uint8)
        f = R.pack(Y, np.full((2, 3), 63, np.uint8), np.full((2, 3), 52, np.uint8), layout)
        bgr = R.to_bgr(f, layout)
        assert bgr.shape == (4, 6, 3) and (bgr.reshape(-1, 3) == [0, 192, 1]).all()


def test_chroma_upsampling_4x4_by_hand():
    # chroma plane 2 x 2 of a 4 x 4 frame:  C = [[a, b], [c, d]] = [[10, 50], [90, 130]]
    C = np.array([[10, 50], [90, 130]], np.uint8)
    got = R.upsample8(C, 4, 4)
    # rows: y0 j0 n0 -> 4a | y1 j0 n1 -> 3a + c | y2 j1 n0 -> 3c + a | y3 j1 n1 (clamped) -> 4c   (V4, per chroma column)
    v4 = np.array([[40, 200], [120, 280], [280, 440], [360, 520]])
    # columns: x0 -> 2 V4[0] | x1 -> V4[0] + V4[1] | x2 -> 2 V4[1] | x3 (clamped) -> 2 V4[1]
    want = np.stack([2 * v4[:, 0], v4[:, 0] + v4[:, 1], 2 * v4[:, 1], 2 * v4[:, 1]], axis=1)
    assert want.tolist() == [[80, 240, 400, 400], [240, 400, 560, 560], [560, 720, 880, 880], [720, 880, 1040, 1040]]
    assert np.array_equal(got, want)


def test_layout_pack_split_roundtrip():
    f = R.random_frame(6, 8, seed=5, layout="i420")
    Y, U, V = R.split(f, "i420")
    n = R.pack(Y, U, V, "nv12")
    assert n.shape == (9, 8) and np.array_equal(n[6:, 0::2], U) and np.array_equal(n[6:, 1::2], V)
    assert np.array_equal(R.to_bgr(f, "i420", 601, True), R.to_bgr(n, "nv12", 601, True))


@pytest.mark.parametrize("pix_fmt", ["yuv420p", "nv12"])
def test_rawvideo_source_yuv_framing(tmp_path, pix_fmt):
    from hdrtv_mi355x import playback as P
    w, h = 8, 6
    frames = [R.random_frame(h, w, seed=i, layout="i420" if pix_fmt == "yuv420p" else "nv12") for i in range(3)]
    path = tmp_path / "clip.yuv"
    path.write_bytes(b"".join(f.tobytes() for f in frames))
    src = P.RawVideoSource(str(path), w, h, 30.0, pix_fmt=pix_fmt, yuv_matrix=2020, yuv_full_range=True)
    assert (src.pix_fmt, src.yuv_matrix, src.yuv_full_range, src.frame_count) == (pix_fmt, 2020, True, 3)
    for f in frames:
        ok, g = src.read()
        assert ok and g.shape == (h * 3 // 2, w) and g.dtype == np.uint8 and np.array_equal(g, f)
    assert src.read() == (False, None)
    src.release()
    bgr = P.RawVideoSource(str(path), 4, 3, 30.0)            # the default stays bgr24: 36 bytes a frame, 216 = 6 frames
    assert bgr.pix_fmt == "bgr24" and bgr.frame_count == 6 and bgr.read()[1].shape == (3, 4, 3)
    (tmp_path / "odd.yuv").write_bytes(bytes(7 * 5 * 3))
    with pytest.raises(ValueError):
        P.RawVideoSource(str(tmp_path / "odd.yuv"), 7, 5, 30.0, pix_fmt=pix_fmt)
    with pytest.raises(ValueError):
        P.RawVideoSource(str(path), w, h, 30.0, pix_fmt="yuv422p")
    with pytest.raises(ValueError):                          # not a whole number of frames
        P.RawVideoSource(str(path), 10, 6, 30.0, pix_fmt=pix_fmt)


def test_pinned_prefetch_passes_2d_frames(tmp_path):
    import torch
    from hdrtv_mi355x import playback as P
    w, h = 16, 8
    frames = [R.random_frame(h, w, seed=10 + i) for i in range(5)]
    path = tmp_path / "clip.yuv"
    path.write_bytes(b"".join(f.tobytes() for f in frames))
    pf = P.PinnedPrefetch(P.RawVideoSource(str(path), w, h, 30.0, pix_fmt="yuv420p", yuv_matrix=601))
    assert (pf.pix_fmt, pf.yuv_matrix, pf.yuv_full_range) == ("yuv420p", 601, False)
    got = []
    while True:
        ok, f = pf.read()
        if not ok:
            break
        if torch.cuda.is_available():
            assert isinstance(f, P.PinnedFrame) and tuple(f.pinned_tensor.shape) == (h * 3 // 2, w)
        got.append(np.array(f))
    pf.release()
    assert len(got) == 5 and all(np.array_equal(g, f) for g, f in zip(got, frames))


def _yuv_standin_worker(rank, device_index, init_args):
    """CPU stand-in for a GPU worker that receives 4:2:0 slots: the rule on the host, into the RGB48 output slot."""

    def process(frame, out):
        assert frame.shape == (out.shape[0] * 3 // 2, out.shape[1])
        np.multiply(R.to_bgr(frame, "i420")[..., ::-1], 257, out=out, dtype=np.uint16, casting="unsafe")
        out[0, 0, 1] = rank

    return process


def test_dispatcher_yuv420p_slots_with_standin_workers():
    from hdrtv_mi355x.dispatch import FrameDispatcher
    h, w, n = 8, 12, 7
    frames = [R.random_frame(h, w, seed=40 + i) for i in range(n)]
    got = {}
    with FrameDispatcher(2, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=_yuv_standin_worker, init_args={},
                         slots=2, numa=False, pix_fmt="yuv420p") as d:
        assert d._in_b == h * w * 3 // 2 and d._out_b == h * w * 6
        assert all(v.shape == (h * 3 // 2, w) for v in d._ins[0])
        for i, f in enumerate(frames):
            if i % 2:
                d.submit(f)
            else:
                j, view = d.reserve()
                assert j == i and view.shape == (h * 3 // 2, w)
                view[...] = f
                d.commit()
        d.flush(timeout=60)
    assert sorted(got) == list(range(n))
    for i, f in enumerate(frames):
        want = R.to_bgr(f)[..., ::-1].astype(np.uint16) * 257
        want[0, 0, 1] = i % 2
        assert np.array_equal(got[i], want), i
    with pytest.raises(ValueError):
        FrameDispatcher(1, 7, 12, lambda i, v: None, make_worker=_yuv_standin_worker, pix_fmt="nv12")
    with pytest.raises(ValueError):
        FrameDispatcher(1, 8, 12, lambda i, v: None, make_worker=_yuv_standin_worker, pix_fmt="yuv444p")


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

    monkeypatch.setattr(WK, "HeadlessPipelineWorker", FakeWorker)
    monkeypatch.setattr(P, "RawVideoSource", fake_source)
    fake_source.PIX_FMTS = ("bgr24", "yuv420p", "nv12")
    with pytest.raises(Stop):
        P.main(["--weights-dir", str(tmp_path), "--size", "64x32", "--input", "x.yuv", "--pix-fmt", "nv12", "--yuv-matrix", "2020",
                "--yuv-range", "full", "--no-prefetch"])
    assert seen == {"pix_fmt": "nv12", "yuv_matrix": 2020, "yuv_full_range": True, "size": (64, 32)}
    with pytest.raises(Stop):
        P.main(["--weights-dir", str(tmp_path), "--size", "64x32", "--input", "x.yuv", "--no-prefetch"])
    assert seen["pix_fmt"] == "bgr24" and seen["yuv_matrix"] == 709 and seen["yuv_full_range"] is False
    for bad in (["--pix-fmt", "yuv444p"], ["--yuv-matrix", "2021"], ["--yuv-range", "studio"]):
        with pytest.raises(SystemExit):
            P.main(["--weights-dir", str(tmp_path), "--input", "x.yuv"] + bad)


def test_worker_input_format():
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    w = HeadlessPipelineWorker("unused")
    w.set_input_format("nv12", 601, True)
    assert w._yuv_format == {"layout": "nv12", "matrix": 601, "full_range": True}
    with pytest.raises(ValueError):
        w.set_input_format("bgr24")


def test_new_entry_points_refuse_a_null_context():
    from hdrtv_mi355x import lib
    so = lib.load()
    assert (lib.YUV_I420, lib.YUV_NV12) == (0, 1)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    assert so.hdrtv_yuv420_to_bgr_u8(None, None, p, 8, p, p, 4, lib.YUV_I420, 709, 0, 4, 8, p) == lib.EINVAL
    assert so.hdrtv_preprocess_yuv420(None, None, p, 8, p, p, 4, lib.YUV_I420, 709, 0, 4, 8, p, p) == lib.EINVAL
    assert so.hdrtv_last_error(None) == b"null context"
