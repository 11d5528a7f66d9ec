"""10-bit Y'CbCr output on a real MI355X: hdrtv_post_ycbcr10 (the model's tensor straight to the planes) and hdrtv_rgb48_to_ycbcr10
(RGB48 codes already on the device), P010 / yuv420p10le / yuv422p10le, both 4:2:0 chroma sitings.

The yardstick is always tests/ycbcr10_ref applied to what the EXISTING entry points write (hdrtv_post_rgb48, or hdrtv_post_pq_rgb48
for pq) -- those are pinned by the other GPU tests, so no quantiser is restated here.  Equality is exact: every u16 of every plane."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import ycbcr10_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
# (H, W).  The kernel's tile is 16 x 128 luma pixels, a lane's group eight pixels: one group, a ragged group, ragged tiles on both
# axes, several tiles down, three tiles across, and the tile plus two on both axes.
SHAPES = [(2, 2), (4, 6), (34, 66), (66, 130), (18, 258), (18, 130)]
COMBOS = [("p010le", "left"), ("p010le", "topleft"), ("yuv420p10le", "left"), ("yuv420p10le", "topleft"), ("yuv422p10le", "left")]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _input(h, w):
    """Seeded values in [-0.25, 1.25] (both clamps of the quantiser act), no NaN, with exact 0 and 1 among them."""
    x = np.random.default_rng(1000 * h + w).uniform(-0.25, 1.25, (3, h, w)).astype(np.float32)
    x[0, 0, 0], x[1, 0, 1], x[2, -1, -1], x[0, -1, 0] = 0.0, 1.0, 1.0, 0.0
    return x


def _codes(p, t, pq):
    """The RGB48 codes of the existing entry points -> (device tensor, numpy)."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.empty((h, w, 3), dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    if pq:
        p._chk(p._lib.hdrtv_post_pq_rgb48(p._ctx, p._stream(), t.data_ptr(), dt, h, w, PEAK, o.data_ptr()), "post_pq_rgb48")
    else:
        p._chk(p._lib.hdrtv_post_rgb48(p._ctx, p._stream(), t.data_ptr(), dt, h, w, o.data_ptr()), "post_rgb48")
    return o, o.cpu().numpy()


def _from_codes(p, codes_dev, fmt, siting):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = codes_dev.shape[:2]
    dst = torch.full((L.out_frame_bytes(fmt, h, w) // 2,), 0xA5A5, dtype=torch.uint16, device=codes_dev.device)
    p._chk(p._lib.hdrtv_rgb48_to_ycbcr10(p._ctx, p._stream(), codes_dev.data_ptr(), h, w, *L.ycbcr10_planes(dst.data_ptr(), h, w, fmt, siting)),
           "rgb48_to_ycbcr10")
    return dst.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "%dx%d" % v)
def test_fused_and_from_codes_equal_the_rule(proc, shape):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = shape
    x = _input(h, w)
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes_dev, codes = _codes(proc, t, pq)
            for fmt, siting in COMBOS:
                want = R.pack(codes, fmt, siting)
                got = proc.postprocess_ycbcr10(t, fmt, siting, pq=bool(pq), peak_nits=PEAK)
                assert got.ndim == 1 and str(got.dtype) == "torch.uint16"
                assert got.numel() * 2 == L.out_frame_bytes(fmt, h, w) == proc._lib.hdrtv_ycbcr10_bytes(L.YCC_FORMATS[fmt], h, w)
                got = got.cpu().numpy()
                tag = (fmt, siting, str(dtype), pq)
                assert np.array_equal(got, want), tag + (int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))
                got2 = _from_codes(proc, codes_dev, fmt, siting)
                assert np.array_equal(got2, want), tag + ("from codes", int((got2 != want).sum()))
                if fmt == "p010le":
                    assert not (got & 63).any()


def _pitched(p, t, codes_dev, fmt, siting, use_codes):
    """The planes in buffers of 0xA5A5 with y_pitch = 2 W + 2, a chroma pitch 6 bytes over its minimum and every plane base 2
    bytes into its buffer -> [(buffer, rows, samples per row, pitch in u16)] for Y, U(V) [, V]."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    ch = h if fmt == "yuv422p10le" else h // 2
    cw = w if fmt == "p010le" else w // 2
    yp, cp = w + 1, cw + 3                                    # in u16
    mk = lambda rows, pitch: torch.full((1 + rows * pitch + 5,), 0xA5A5, dtype=torch.uint16, device="cuda")      # noqa: E731
    by, bu = mk(h, yp), mk(ch, cp)
    bv = None if fmt == "p010le" else mk(ch, cp)
    tail = (L.YCC_FORMATS[fmt], L.YCC_SITINGS[siting], by.data_ptr() + 2, 2 * yp, bu.data_ptr() + 2,
            None if bv is None else bv.data_ptr() + 2, 2 * cp)
    if use_codes:
        p._chk(p._lib.hdrtv_rgb48_to_ycbcr10(p._ctx, p._stream(), codes_dev.data_ptr(), h, w, *tail), "rgb48_to_ycbcr10")
    else:
        p._chk(p._lib.hdrtv_post_ycbcr10(p._ctx, p._stream(), t.data_ptr(), L.F32 if t.dtype == torch.float32 else L.F16, h, w, 0, 0.0,
                                         *tail), "post_ycbcr10")
    out = [(by.cpu().numpy(), h, w, yp), (bu.cpu().numpy(), ch, cw, cp)]
    if bv is not None:
        out.append((bv.cpu().numpy(), ch, cw, cp))
    return out


@pytest.mark.parametrize("shape", [(34, 66), (18, 258)], ids=lambda v: "%dx%d" % v)
def test_pitched_unaligned_planes_match_and_padding_stays(proc, shape):
    import torch
    h, w = shape
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(_input(h, w)).to("cuda", dtype).contiguous()
        codes_dev, codes = _codes(proc, t, 0)
        for fmt, siting in COMBOS:
            y, cb, cr = R.planes(codes, fmt, siting)
            if fmt == "p010le":
                c = np.empty((cb.shape[0], w), np.uint16)
                c[:, 0::2], c[:, 1::2] = cb, cr
                want_planes = [y, c]
            else:
                want_planes = [y, cb, cr]
            for use_codes in (False, True):
                for (buf, rows, n, pitch), want in zip(_pitched(proc, t, codes_dev, fmt, siting, use_codes), want_planes):
                    expect = np.full(buf.shape, 0xA5A5, np.uint16)
                    for r in range(rows):
                        expect[1 + r * pitch: 1 + r * pitch + n] = want[r]
                    assert np.array_equal(buf, expect), (fmt, siting, str(dtype), use_codes, int((buf != expect).sum()))


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 12, 20
    t = torch.rand((3, h, w), device="cuda")
    codes_dev, codes = _codes(proc, t, 0)
    dst = torch.full((h * w * 4,), 0xA5A5, dtype=torch.uint16, device="cuda")
    ctx, st, i, o = proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    u, v = o + 2 * h * w, o + 2 * h * w + h * w // 2               # the planes of a contiguous 4:2:0 frame (bytes)
    P, P420, P422, LEFT, TOP = L.YCC_P010, L.YCC_YUV420P10, L.YCC_YUV422P10, L.SITING_LEFT, L.SITING_TOPLEFT
    ok = (P420, LEFT, o, 2 * w, u, v, w)
    # the arguments both entry points share: (H, W, fmt, siting, dst_y, y_pitch, dst_u, dst_v, c_pitch)
    shared = [
        (h, w, P420, LEFT, None, 2 * w, u, v, w), (h, w, P420, LEFT, o, 2 * w, None, v, w), (h, w, P420, LEFT, o, 2 * w, u, None, w),
        (h, w - 1, P420, LEFT, o, 2 * w, u, v, w), (h - 1, w, P420, LEFT, o, 2 * w, u, v, w), (h - 1, w, P, LEFT, o, 2 * w, u, None, 2 * w),
        (0, w, P420, LEFT, o, 2 * w, u, v, w), (h, 0, P420, LEFT, o, 2 * w, u, v, w), (-h, w, P422, LEFT, o, 2 * w, u, v, w),
        (h, w, P420, LEFT, o, 2 * w - 2, u, v, w), (h, w, P420, LEFT, o, 2 * w + 1, u, v, w),
        (h, w, P420, LEFT, o, 2 * w, u, v, w - 2), (h, w, P420, LEFT, o, 2 * w, u, v, w + 1),
        (h, w, P, LEFT, o, 2 * w, u, None, 2 * w - 2), (h, w, P, LEFT, o, 2 * w, u, None, w),
        (h, w, 3, LEFT, o, 2 * w, u, v, w), (h, w, -1, LEFT, o, 2 * w, u, v, w),
        (h, w, P420, 2, o, 2 * w, u, v, w), (h, w, P420, -1, o, 2 * w, u, v, w),
        (h, w, P, LEFT, o, 2 * w, u, v, 2 * w),                       # P010 with a dst_v
        (h, w, P422, TOP, o, 2 * w, u, v, w),                         # 4:2:2 is co-sited
    ]
    f1, f2 = proc._lib.hdrtv_post_ycbcr10, proc._lib.hdrtv_rgb48_to_ycbcr10
    for k, a in enumerate(shared):
        assert f1(ctx, st, i, L.F32, a[0], a[1], 0, 0.0, *a[2:]) == L.EINVAL, k
        assert f2(ctx, st, codes_dev.data_ptr(), *a) == L.EINVAL, k
    assert f1(None, st, i, L.F32, h, w, 0, 0.0, *ok) == L.EINVAL and f2(None, st, codes_dev.data_ptr(), h, w, *ok) == L.EINVAL
    assert f1(ctx, st, None, L.F32, h, w, 0, 0.0, *ok) == L.EINVAL and f2(ctx, st, None, h, w, *ok) == L.EINVAL
    for dt in (2, -1):
        assert f1(ctx, st, i, dt, h, w, 0, 0.0, *ok) == L.EINVAL
    for peak in (0.0, -100.0):
        assert f1(ctx, st, i, L.F32, h, w, 1, peak, *ok) == L.EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    assert f1(ctx, st, i, L.F32, h, w, 0, -5.0, *ok) == L.OK              # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    n = h * w * 3 // 2
    assert np.array_equal(dst.cpu().numpy()[:n], R.pack(codes, "yuv420p10le", "left")) and (dst.cpu().numpy()[n:] == 0xA5A5).all()
    for bad in (("rgb48le", "left"), ("yuv422p10le", "topleft"), ("nv12", "left"), ("p010le", "centre")):
        with pytest.raises(ValueError):
            proc.postprocess_ycbcr10(t, *bad)


def test_ring_commit_bytes_moves_the_frame_and_nothing_behind_it(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 34, 66
    lib, ctx, st = proc._lib, proc._ctx, proc._stream()
    t = torch.from_numpy(_input(h, w)).cuda()
    _, codes = _codes(proc, t, 0)
    assert lib.hdrtv_ring_create(ctx, 2, h, w) == 0
    try:
        for fmt, siting in (("p010le", "topleft"), ("yuv422p10le", "left")):
            nbytes = L.out_frame_bytes(fmt, h, w)
            host, dev = C.c_void_p(), C.c_void_p()
            slot = lib.hdrtv_ring_acquire(ctx, 100, C.byref(host), C.byref(dev))
            assert slot >= 0
            C.memset(host.value, 0x5A, h * w * 6)
            assert lib.hdrtv_post_ycbcr10(ctx, st, t.data_ptr(), L.F32, h, w, 0, 0.0, *L.ycbcr10_planes(dev.value, h, w, fmt, siting)) == 0
            assert lib.hdrtv_ring_commit_bytes(ctx, slot, st, h * w * 6 + 1) == L.EINVAL
            assert lib.hdrtv_ring_commit_bytes(ctx, slot, st, 0) == L.EINVAL
            assert lib.hdrtv_ring_commit_bytes(ctx, slot, st, nbytes) == 0        # the refused commits left the slot acquired
            assert lib.hdrtv_ring_commit_bytes(ctx, slot, st, nbytes) == L.ESTATE
            assert lib.hdrtv_ring_wait(ctx, slot) == 0
            got = np.ctypeslib.as_array((C.c_uint16 * (h * w * 3)).from_address(host.value)).copy()
            assert lib.hdrtv_ring_release(ctx, slot) == 0
            assert np.array_equal(got[: nbytes // 2], R.pack(codes, fmt, siting)), fmt
            assert (got[nbytes // 2:] == 0x5A5A).all(), fmt
    finally:
        lib.hdrtv_ring_destroy(ctx)


# ------------------------------------------------------------------------------------------ end to end, on a committed golden frame
def _golden_frame(golden_dir):
    return np.load(os.path.join(golden_dir, "hr_64x96_noise_s0.npz"))["frame"]


def test_enqueue_frame_writes_the_rule_of_its_default_output(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    frame = _golden_frame(golden_dir)
    h, w = frame.shape[:2]
    oh, ow = 2 * h, 2 * w
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(frame).cuda()
        st = torch.cuda.current_stream()
        rgb = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
        big = torch.empty((oh, ow, 3), dtype=torch.uint16, device="cuda")
        p.enqueue_frame(0, dev.data_ptr(), h, w, rgb.data_ptr(), stream=st)
        p.enqueue_frame(0, dev.data_ptr(), h, w, big.data_ptr(), stream=st, out_hw=(oh, ow))
        outs = {}
        for fmt, siting in (("p010le", "left"), ("yuv420p10le", "topleft"), ("yuv422p10le", "left")):
            a = torch.full((L.out_frame_bytes(fmt, h, w) // 2,), 0xA5A5, dtype=torch.uint16, device="cuda")
            b = torch.full((L.out_frame_bytes(fmt, oh, ow) // 2,), 0xA5A5, dtype=torch.uint16, device="cuda")
            p.enqueue_frame(0, dev.data_ptr(), h, w, a.data_ptr(), stream=st, out_pix_fmt=fmt, out_siting=siting)
            p.enqueue_frame(0, dev.data_ptr(), h, w, b.data_ptr(), stream=st, out_hw=(oh, ow), out_pix_fmt=fmt, out_siting=siting)
            outs[fmt, siting] = (a, b)
        yuv = torch.full((h * 3 // 2, w), 128, dtype=torch.uint8, device="cuda")
        yrgb, yp010 = torch.empty_like(rgb), torch.empty_like(outs["p010le", "left"][0])
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, yrgb.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, yp010.data_ptr(), stream=st, out_pix_fmt="p010le")
        torch.cuda.synchronize()
        for (fmt, siting), (a, b) in outs.items():
            assert np.array_equal(a.cpu().numpy(), R.pack(rgb.cpu().numpy(), fmt, siting)), fmt
            assert np.array_equal(b.cpu().numpy(), R.pack(big.cpu().numpy(), fmt, siting)), fmt
        assert np.array_equal(yp010.cpu().numpy(), R.pack(yrgb.cpu().numpy(), "p010le", "left"))
        with pytest.raises(ValueError):
            p.enqueue_frame(0, dev.data_ptr(), h, w, rgb.data_ptr(), stream=st, out_pix_fmt="yuv444p10le")
    finally:
        p.close()


def _run_worker(golden_dir, tmp_path, tag, frames, sink_of, **kw):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / tag / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    wk = HeadlessPipelineWorker(str(tmp_path / tag), use_hg=True, proc_w=frames[0].shape[1], proc_h=frames[0].shape[0],
                                hg_weights="seeded:1234", buffer_frames=3, **kw)
    assert wk._load_model("FP16", warmup=False)
    n, done = [0], threading.Event()
    inner = sink_of(wk)

    def sink(payload):
        inner(payload)
        n[0] += 1
        if n[0] == len(frames):
            done.set()

    wk._start_hdr_feeder(sink)
    try:
        for i, f in enumerate(frames):
            wk._process_frame(frame=f, frame_idx=i, mpv_w=True)
        for _ in range(300):                                   # a feeder that died says so at once
            if done.wait(0.1):
                break
            assert wk._hdr_error is None, repr(wk._hdr_error)
        assert done.is_set()
    finally:
        wk._stop_hdr_feeder()
        wk.close()


def test_worker_writes_ycbcr_frames_into_a_file_sink(golden_dir, tmp_path):
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.playback import RawVideoSink
    frames = [_golden_frame(golden_dir), W.synthetic_frame(64, 96, seed=61, kind="noise")]
    h, w = frames[0].shape[:2]
    base, shapes = [], []

    def keep(wk):
        def sink(payload):
            base.append(payload.numpy().copy())
            payload.release()
        return sink

    _run_worker(golden_dir, tmp_path, "rgb", frames, keep)
    path = tmp_path / "out.p010"
    sinks = []

    def to_file(wk):
        s = RawVideoSink(str(path), w, h, 60.0, "p010le", "topleft")
        sinks.append(s)

        def sink(payload):
            shapes.append(payload.numpy().shape)
            s(payload)
        return sink

    _run_worker(golden_dir, tmp_path, "ycc", frames, to_file, out_pix_fmt="p010le", out_siting="topleft")
    sinks[0].close()
    nbytes = L.out_frame_bytes("p010le", h, w)
    assert nbytes == L.load().hdrtv_ycbcr10_bytes(L.YCC_P010, h, w) == h * w * 3
    assert sinks[0].frames == 2 and sinks[0].bytes == 2 * nbytes and shapes == [(nbytes // 2,)] * 2
    data = np.fromfile(str(path), dtype="<u2")
    assert data.size == nbytes
    for i in range(2):
        assert base[i].shape == (h, w, 3)
        assert np.array_equal(data[i * nbytes // 2: (i + 1) * nbytes // 2], R.pack(base[i], "p010le", "topleft")), i


def test_dispatcher_delivers_ycbcr_frames_in_order(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.dispatch import FrameDispatcher
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    frames = [_golden_frame(golden_dir), W.synthetic_frame(64, 96, seed=81, kind="noise")]
    h, w = frames[0].shape[:2]
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    want = []
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    for f in frames:
        dev = torch.from_numpy(f).cuda()
        p.enqueue_frame(0, dev.data_ptr(), h, w, u16.data_ptr(), stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        want.append(R.pack(u16.cpu().numpy(), "yuv420p10le", "left"))
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_pix_fmt="yuv420p10le") as d:
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0]
    assert sorted(got) == [0, 1]
    nbytes = L.out_frame_bytes("yuv420p10le", h, w)
    for i in range(2):
        assert got[i].shape == (nbytes // 2,) and got[i].dtype == np.uint16 and got[i].nbytes == h * w * 3
        assert np.array_equal(got[i], want[i]), i
