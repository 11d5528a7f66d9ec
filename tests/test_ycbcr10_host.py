"""10-bit Y'CbCr output, the parts that need no GPU: the facts the rule (include/hdrtv_mi355x.h, restated in tests/ycbcr10_ref.py)
states about itself, the frame layouts, the sink's ffmpeg arguments, the dispatcher's slot size and the argument checks that
return before any device call."""
import ctypes
import io
import re

import numpy as np
import pytest

import ycbcr10_ref as R

KNOWN = {(0, 0, 0): (64, 512, 512), (65535, 65535, 65535): (940, 512, 512), (32768, 32768, 32768): (502, 512, 512),
         (65535, 0, 0): (294, 387, 960), (0, 65535, 0): (658, 189, 100), (0, 0, 65535): (116, 960, 476)}
COMBOS = [(f, s) for f in R.FORMATS for s in R.SITINGS if not (f == "yuv422p10le" and s == "topleft")]


def test_coefficient_table():
    (yr, yg, yb), (ur, ug, ub), (vr, vg, vb) = R.coefficients()
    assert (yr, yg, yb) == (3682, 9503, 831) and yr + yg + yb == 14016
    assert (ur, ug, ub) == (-2002, -5166, 7168) and (vr, vg, vb) == (7168, -6591, -577)
    assert ur + ug + ub == 0 and vr + vg + vb == 0


def test_header_states_the_same_coefficients():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdrtv_mi355x.h")).read()
    for v in ("14016", "3682", "9503", "831", "7168", "-2002", "-5166", "-577", "-6591", "UNPINNED"):
        assert re.search(r"(?<![\d-])" + re.escape(v) + r"(?!\d)", text), v


@pytest.mark.parametrize("fmt,siting", COMBOS)
def test_known_answers_and_constant_frames(fmt, siting):
    shift = 6 if fmt == "p010le" else 0
    for rgb, (y, cb, cr) in KNOWN.items():
        frame = np.tile(np.array(rgb, np.uint16), (6, 10, 1))
        py, pcb, pcr = R.planes(frame, fmt, siting)
        assert (py == y << shift).all() and (pcb == cb << shift).all() and (pcr == cr << shift).all(), (rgb, fmt, siting)
    rng = np.random.default_rng(5)
    for _ in range(20):                                       # chroma of a constant frame is constant, edges included
        frame = np.tile(rng.integers(0, 65536, 3).astype(np.uint16), (4, 6, 1))
        py, pcb, pcr = R.planes(frame, fmt, siting)
        assert len(np.unique(py)) == len(np.unique(pcb)) == len(np.unique(pcr)) == 1
        g = np.tile(np.uint16(rng.integers(0, 65536)), (4, 6, 3))
        _, gcb, gcr = R.planes(g, fmt, siting)
        assert (gcb == 512 << shift).all() and (gcr == 512 << shift).all()


def test_integer_rule_is_within_0p6_code_of_the_exact_formula():
    t = np.random.default_rng(0).integers(0, 65536, (200000, 1, 3)).astype(np.uint16)
    ey, ecb, ecr = R.exact(t)
    cb, cr = R.chroma(np.repeat(t, 2, axis=1), "yuv422p10le", "left")     # rows of two equal pixels: the per-pixel value
    errs = (np.abs(R.luma(t)[:, 0] - ey[:, 0]).max(), np.abs(cb[:, 0] - ecb[:, 0]).max(), np.abs(cr[:, 0] - ecr[:, 0]).max())
    print("max |integer rule - exact|, codes: Y %.4f Cb %.4f Cr %.4f" % errs)
    assert max(errs) < 0.6
    y = R.luma(t)
    assert y.min() >= 64 and y.max() <= 940 and cb.min() >= 64 and cb.max() <= 960 and cr.min() >= 64 and cr.max() <= 960


def test_taps_and_edge_repeat():
    """One bright pixel: the samples it reaches and their weights, per layout and siting (red: Cr rises by VR * weight)."""
    h, w = 8, 12
    vr = R.coefficients()[2][0]

    def cr_of(y, x, fmt, siting):
        f = np.zeros((h, w, 3), np.uint16)
        f[y, x, 0] = 65535
        return R.chroma(f, fmt, siting)[1].astype(np.int64)

    def val(weight, lg):
        return 512 + ((vr * 65535 * weight + (1 << (19 + lg))) >> (20 + lg))

    c = cr_of(3, 5, "yuv422p10le", "left")                    # odd column: samples 2 and 3 of row 3, weight 1 of 4
    assert c[3, 2] == c[3, 3] == val(1, 2) and (np.delete(c.reshape(-1), [3 * 6 + 2, 3 * 6 + 3]) == 512).all()
    c = cr_of(3, 4, "yuv422p10le", "left")                    # even column: its own sample, weight 2
    assert c[3, 2] == val(2, 2) and (c != 512).sum() == 1
    c = cr_of(3, 4, "yuv420p10le", "left")                    # rows 2j, 2j + 1: row 3 belongs to j = 1
    assert c[1, 2] == val(2, 3) and (c != 512).sum() == 1
    c = cr_of(3, 4, "yuv420p10le", "topleft")                 # odd row: weight 1 in j = 1 (2j + 1) and j = 2 (2j - 1)
    assert c[1, 2] == c[2, 2] == val(2, 4) and (c != 512).sum() == 2
    c = cr_of(2, 4, "yuv420p10le", "topleft")                 # even row: weight 2 in its own j
    assert c[1, 2] == val(4, 4) and (c != 512).sum() == 1
    c = cr_of(0, 0, "yuv420p10le", "topleft")                 # the corner repeats into column -1 and row -1: (2 + 1) * (2 + 1)
    assert c[0, 0] == val(9, 4) and (c != 512).sum() == 1
    c = cr_of(0, 0, "yuv420p10le", "left")
    assert c[0, 0] == val(3, 3)
    c = cr_of(0, 0, "yuv422p10le", "left")
    assert c[0, 0] == val(3, 2)


def test_plane_sizes_and_offsets():
    h, w = 6, 10
    rgb = np.random.default_rng(1).integers(0, 65536, (h, w, 3)).astype(np.uint16)
    for fmt, siting in COMBOS:
        flat = R.pack(rgb, fmt, siting)
        y, cb, cr = R.planes(rgb, fmt, siting)
        assert flat.dtype == np.uint16 and flat.nbytes == R.frame_bytes(fmt, h, w) == h * w * (4 if fmt == "yuv422p10le" else 3)
        (oy, ou, ov), (crows, cwidth) = R.plane_offsets(fmt, h, w)
        assert oy == 0 and ou == h * w and np.array_equal(flat[:ou].reshape(h, w), y)
        if fmt == "p010le":
            assert ov is None and (crows, cwidth) == (h // 2, w) and cb.shape == (h // 2, w // 2)
            c = flat[ou:].reshape(crows, cwidth)
            assert np.array_equal(c[:, 0::2], cb) and np.array_equal(c[:, 1::2], cr)
            assert not (flat & 63).any() and (flat >> 6).max() <= 960 and (flat >> 6).min() >= 64
        else:
            assert (crows, cwidth) == ((h if fmt == "yuv422p10le" else h // 2), w // 2) and cb.shape == (crows, cwidth)
            assert ov == ou + crows * cwidth and ov + crows * cwidth == flat.size
            assert np.array_equal(flat[ou:ov].reshape(crows, cwidth), cb) and np.array_equal(flat[ov:].reshape(crows, cwidth), cr)
            assert flat.max() <= 960


def test_python_side_formats_sizes_and_plane_arguments():
    from hdrtv_mi355x import lib as L
    h, w = 6, 10
    assert L.out_frame_bytes("rgb48le", h, w) == h * w * 6
    for fmt in R.FORMATS:
        assert L.out_frame_bytes(fmt, h, w) == R.frame_bytes(fmt, h, w)
        (oy, ou, ov), (crows, cwidth) = R.plane_offsets(fmt, h, w)
        code, sit, py, ypitch, pu, pv, cpitch = L.ycbcr10_planes(1000, h, w, fmt, "left")
        assert (code, sit, py, ypitch, pu, cpitch) == (L.YCC_FORMATS[fmt], L.SITING_LEFT, 1000, 2 * w, 1000 + 2 * ou, 2 * cwidth)
        assert pv == (None if ov is None else 1000 + 2 * ov)
    for bad in (("p010le", 5, 10), ("yuv420p10le", 6, 9), ("yuv422p10le", 5, 9), ("yuv444p10le", 6, 10)):
        with pytest.raises(ValueError):
            L.out_frame_bytes(*bad)
    assert L.out_frame_bytes("yuv422p10le", 5, 10) == 200
    assert L.check_out_format("P010LE", "TopLeft") == ("p010le", "topleft")
    for bad in (("yuv422p10le", "topleft"), ("p010", "left"), ("p010le", "center")):
        with pytest.raises(ValueError):
            L.check_out_format(*bad)


OUT_SIZES = ((2, 2), (6, 10), (64, 96), (2160, 3840))


@pytest.mark.parametrize("h,w", OUT_SIZES)
def test_output_format_object_states_what_the_public_functions_state(h, w):
    """lib.OutputFormat against hdrtv_ycbcr10_bytes (tests/ycbcr10_ref.frame_bytes when the library is not built), against
    lib.ycbcr10_planes, and through pickle (it crosses into the dispatcher's worker processes)."""
    import pickle
    from hdrtv_mi355x import lib as L
    try:
        so = L.load()
    except RuntimeError:
        so = None
    f = L.output_format("rgb48le", "left", h, w)
    assert f.is_rgb48 and f.nbytes == h * w * 6 and f.shape == (h, w, 3) and int(np.prod(f.shape)) == f.nbytes // 2
    assert pickle.loads(pickle.dumps(f)) == f and isinstance(pickle.loads(pickle.dumps(f)), L.OutputFormat)
    with pytest.raises(ValueError):
        f.planes(4096)
    for fmt, siting in COMBOS:
        f = L.output_format(fmt, siting, h, w)
        assert tuple(f) == (fmt, siting, h, w) and not f.is_rgb48
        want = so.hdrtv_ycbcr10_bytes(L.YCC_FORMATS[fmt], h, w) if so is not None else R.frame_bytes(fmt, h, w)
        assert f.nbytes == want == L.out_frame_bytes(fmt, h, w)
        assert f.shape == (f.nbytes // 2,)
        assert f.planes(4096) == L.ycbcr10_planes(4096, h, w, fmt, siting)
        back = pickle.loads(pickle.dumps(f))
        assert back == f and isinstance(back, L.OutputFormat) and back.nbytes == f.nbytes and back.shape == f.shape


def test_output_format_constructor_rejects_what_the_public_functions_reject():
    from hdrtv_mi355x import lib as L
    odd = [("p010le", "left", 6, 9), ("yuv420p10le", "left", 6, 9), ("yuv422p10le", "left", 6, 9),          # odd W
           ("p010le", "left", 5, 10), ("yuv420p10le", "topleft", 5, 10)]                                    # odd H for 4:2:0
    names = [("yuv422p10le", "topleft", 6, 10),                                                             # 4:2:2 is co-sited
             ("yuv444p10le", "left", 6, 10), ("p010", "left", 6, 10), ("p010le", "center", 6, 10), ("rgb48le", "middle", 6, 10)]
    for fmt, siting, h, w in odd:                            # what out_frame_bytes / ycbcr10_planes reject
        for call in (lambda: L.out_frame_bytes(fmt, h, w), lambda: L.ycbcr10_planes(4096, h, w, fmt, siting),
                     lambda: L.output_format(fmt, siting, h, w)):
            with pytest.raises(ValueError):
                call()
    for fmt, siting, h, w in names:                          # what check_out_format rejects
        for call in (lambda: L.check_out_format(fmt, siting), lambda: L.output_format(fmt, siting, h, w)):
            with pytest.raises(ValueError):
                call()
    assert L.output_format("yuv422p10le", "left", 5, 10).nbytes == 200          # 4:2:2 takes an odd height
    assert L.output_format("RGB48LE", "Left", 5, 9) == ("rgb48le", "left", 5, 9)
    assert L.output_format("p010le", "left", 6, 10).at(6, 10).at(8, 12) == ("p010le", "left", 8, 12)
    with pytest.raises(ValueError):
        L.output_format("p010le", "left", 6, 10).at(7, 12)


def test_library_sizes_and_refusals_without_a_device():
    from hdrtv_mi355x import lib
    so = lib.load()
    P, P420, P422 = lib.YCC_P010, lib.YCC_YUV420P10, lib.YCC_YUV422P10
    for fmt, name in ((P, "p010le"), (P420, "yuv420p10le"), (P422, "yuv422p10le")):
        assert so.hdrtv_ycbcr10_bytes(fmt, 2160, 3840) == lib.out_frame_bytes(name, 2160, 3840)
    assert so.hdrtv_ycbcr10_bytes(P, 2160, 3840) == 24883200 and so.hdrtv_ycbcr10_bytes(P422, 2160, 3840) == 33177600
    assert so.hdrtv_ycbcr10_bytes(P422, 5, 10) == 200
    assert so.hdrtv_ycbcr10_bytes(P, 46342, 46342) == 46342 * 46342 * 3           # past 2^31
    for bad in ((P, 5, 10), (P420, 6, 9), (P422, 6, 9), (3, 6, 10), (-1, 6, 10), (P, 0, 10), (P, 6, 0), (P, -6, 10)):
        assert so.hdrtv_ycbcr10_bytes(*bad) < 0, bad
    # every entry point refuses a NULL context before it touches a device, whatever else it is given
    buf = (ctypes.c_uint16 * 64)(*([0xA5A5] * 64))
    a = ctypes.addressof(buf)
    for fmt, sit, v, cp in ((P, 0, None, 8), (P420, 1, a + 48, 4), (P422, 0, a + 48, 4), (P422, 1, a + 48, 4), (P, 0, a + 48, 8), (7, 0, a, 8),
                            (P420, 5, a + 48, 4), (P420, 0, a + 48, 3)):
        assert so.hdrtv_post_ycbcr10(None, None, a, lib.F32, 2, 4, 0, 0.0, fmt, sit, a, 8, a + 32, v, cp) == lib.EINVAL
        assert so.hdrtv_post_ycbcr10(None, None, a, lib.F32, 2, 4, 1, -1.0, fmt, sit, a, 8, a + 32, v, cp) == lib.EINVAL
        assert so.hdrtv_rgb48_to_ycbcr10(None, None, a, 2, 4, fmt, sit, a, 8, a + 32, v, cp) == lib.EINVAL
    assert so.hdrtv_ring_commit_bytes(None, 0, None, 16) == lib.EINVAL
    assert all(x == 0xA5A5 for x in buf)
    names = {n for n, _, _ in lib.SYMBOLS}
    assert {"hdrtv_post_ycbcr10", "hdrtv_rgb48_to_ycbcr10", "hdrtv_ycbcr10_bytes", "hdrtv_ring_commit_bytes"} <= names


class _Payload:
    def __init__(self, data):
        self._d, self.released = data, False

    def buffer_view(self):
        return memoryview(self._d).cast("B")

    def release(self):
        self.released = True


def test_raw_video_sink_arguments_and_frame_size():
    from hdrtv_mi355x.playback import RawVideoSink, Rgb48leSink
    common = ["-color_range", "tv", "-colorspace", "bt2020nc", "-color_trc", "smpte2084", "-color_primaries", "bt2020"]
    for fmt, siting in COMBOS:
        s = RawVideoSink(io.BytesIO(), 10, 6, 59.94, fmt, siting)
        args = s.ffmpeg_input_args()
        assert args[:8] == ["-f", "rawvideo", "-pix_fmt", fmt, "-s:v", "10x6", "-r", "59.940000"] and args[-2:] == ["-i", "-"]
        assert args[8:16] == common
        assert args[16:-2] == (["-chroma_sample_location", "topleft"] if siting == "topleft" else [])
        assert f"--demuxer-rawvideo-mp-format={fmt[:-2]}" in s.mpv_args()
        good = _Payload(np.zeros(R.frame_bytes(fmt, 6, 10) // 2, np.uint16))
        s(good)
        assert good.released and s.frames == 1 and s.bytes == R.frame_bytes(fmt, 6, 10)
        wrong = _Payload(np.zeros(6 * 10 * 3, np.uint16))                  # an RGB48 frame
        with pytest.raises(ValueError):
            s(wrong)
        assert wrong.released and s.frames == 1
    d = RawVideoSink(io.BytesIO(), 10, 6, 60.0)                            # the default is the RGB48 sink, unchanged
    ref = Rgb48leSink(io.BytesIO(), 10, 6, 60.0)
    assert isinstance(d, Rgb48leSink) and d.ffmpeg_input_args() == ref.ffmpeg_input_args() and d.mpv_args() == ref.mpv_args()
    d(_Payload(np.zeros(6 * 10 * 3, np.uint16)))
    assert d.bytes == 360
    with pytest.raises(ValueError):
        RawVideoSink(io.BytesIO(), 10, 6, 60.0, "yuv422p10le", "topleft")
    with pytest.raises(ValueError):
        RawVideoSink(io.BytesIO(), 10, 5, 60.0, "p010le")


def _fill_worker(rank, device_index, init_args):
    def process(frame, out):
        out[...] = np.arange(out.size, dtype=np.uint32).astype(np.uint16).reshape(out.shape) + np.uint16(frame.flat[0])
    return process


def test_dispatcher_sizes_its_output_slots_for_the_format():
    from hdrtv_mi355x import dispatch as D
    from hdrtv_mi355x import lib as L
    h, w = 6, 10
    for fmt in R.FORMATS + ("rgb48le",):
        nbytes = R.frame_bytes(fmt, h, w) if fmt != "rgb48le" else h * w * 6
        shape = L.output_format(fmt, "left", h, w).shape
        assert 2 * int(np.prod(shape)) == nbytes and (len(shape) == 1) == (fmt != "rgb48le")
    for bad in (dict(out_pix_fmt="yuv444p10le"), dict(out_pix_fmt="yuv422p10le", out_siting="topleft"), dict(out_pix_fmt="p010le", out_height=7)):
        with pytest.raises(ValueError):
            D.FrameDispatcher(1, h, w, lambda i, v: None, make_worker=_fill_worker, numa=False, **bad)
    got = {}
    with D.FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), make_worker=_fill_worker, slots=2, numa=False,
                           out_pix_fmt="yuv420p10le", out_height=8, out_width=12) as d:
        assert d._out_b == 8 * 12 * 3 and d.placement[0]["slot_bytes"] == 2 * (h * w * 3 + 8 * 12 * 3)
        for k in range(3):
            d.submit(np.full((h, w, 3), k, np.uint8))
        d.flush(timeout=60)
    assert d.exit_codes == [0] and sorted(got) == [0, 1, 2]
    for k in range(3):
        assert got[k].shape == (8 * 12 * 3 // 2,) and got[k].dtype == np.uint16
        assert np.array_equal(got[k], np.arange(144, dtype=np.uint16) + k)
