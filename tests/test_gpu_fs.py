"""Floyd-Steinberg error diffusion of the 10-bit Y'CbCr output on a real MI355X: hdrtv_post_ycbcr10_fs / hdrtv_rgb48_to_ycbcr10_fs and
the routes through postprocess_ycbcr10, _post_out (what enqueue_frame and the worker deliver through) and the worker that carry
dither="floyd_steinberg".

The yardstick is always tests/fs_ref applied to the RGB48 codes the EXISTING entry points write -- those are pinned by the other GPU
tests, so no quantiser is restated here.  Equality is exact: every u16.

The shapes follow the diffusion kernel (csrc/post_ycbcr_fs.hip): a workgroup keeps R = lib.FS_ROWS rows in flight and stages
C = lib.FS_CHUNK columns at a time.  2 x 2 gives chroma planes one sample wide (every neighbour term dropped), 1 x 2 a 4:2:2 frame
of one row; H = R + 3 (4:2:2) and H = 2 R + 6 (4:2:0) put the carried error row between two row groups into the luma and the chroma
planes; W = C + 2 and W = 2 C + 6 put the staging seam into the luma plane and (the second) into the chroma planes; 70 x 132 is
ragged in every unit (wave, chunk, tile of the samples pass)."""
import os
import threading

import numpy as np
import pytest

import cleanup_ref as K
import fs_ref as F
import ycbcr10_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
COMBOS = [("p010le", "left"), ("p010le", "topleft"), ("yuv420p10le", "left"), ("yuv420p10le", "topleft"), ("yuv422p10le", "left")]
ROWS, CHUNK = 256, 32           # asserted against lib.FS_ROWS / lib.FS_CHUNK below
SMALL_SHAPES = [(2, 2), (6, CHUNK + 2), (6, 2 * CHUNK + 6), (70, 132)]
TALL_SHAPES = [(ROWS + 3, 34), (2 * ROWS + 6, 34)]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    assert (L.FS_ROWS, L.FS_CHUNK) == (ROWS, CHUNK)
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _input(h, w):
    """Seeded values in [-0.25, 1.25] (both clamps of the quantiser act), with exact 0 and 1 among them."""
    x = np.random.default_rng(1000 * h + w).uniform(-0.25, 1.25, (3, h, w)).astype(np.float32)
    x[0, 0, 0], x[1, 0, -1], x[2, -1, -1], x[0, -1, 0] = 0.0, 1.0, 1.0, 0.0
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


def _scratch(p, fmt, h, w, fill=0xFF):
    """A scratch of the size the library asks for, filled: what it holds on entry must not matter."""
    import torch
    from hdrtv_mi355x import lib as L
    n = p._lib.hdrtv_ycbcr10_fs_scratch_bytes(L.YCC_FORMATS[fmt], h, w)
    ch = h if fmt == "yuv422p10le" else h // 2
    assert n == 4 * (h * w + 2 * ch * (w // 2) + 2 * w)
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


def _from_codes(p, codes_dev, fmt, siting, scratch=None):
    """hdrtv_rgb48_to_ycbcr10_fs into a contiguous frame of 0xA5A5."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = codes_dev.shape[:2]
    dst = torch.full((L.out_frame_bytes(fmt, h, w) // 2,), 0xA5A5, dtype=torch.uint16, device="cuda")
    scratch = _scratch(p, fmt, h, w) if scratch is None else scratch
    p._chk(p._lib.hdrtv_rgb48_to_ycbcr10_fs(p._ctx, p._stream(), codes_dev.data_ptr(), h, w,
                                            *L.ycbcr10_planes(dst.data_ptr(), h, w, fmt, siting), scratch.data_ptr()), "rgb48_to_ycbcr10_fs")
    return dst.cpu().numpy()


def _from_tensor(p, t, fmt, siting, pq):
    """hdrtv_post_ycbcr10_fs into a contiguous frame of 0xA5A5."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    dst = torch.full((L.out_frame_bytes(fmt, h, w) // 2,), 0xA5A5, dtype=torch.uint16, device="cuda")
    scratch = _scratch(p, fmt, h, w, 0x5A)
    p._chk(p._lib.hdrtv_post_ycbcr10_fs(p._ctx, p._stream(), t.data_ptr(), L.F32 if t.dtype == torch.float32 else L.F16, h, w, pq, PEAK,
                                        *L.ycbcr10_planes(dst.data_ptr(), h, w, fmt, siting), scratch.data_ptr()), "post_ycbcr10_fs")
    return dst.cpu().numpy()


def _diff(got, want):
    return int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max())


# ------------------------------------------------------------------------------------------------------------ the entry points
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda v: "%dx%d" % v)
def test_both_entry_points_equal_the_rule(proc, shape):
    import torch
    h, w = shape
    x = _input(h, w)
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes_dev, codes = _codes(proc, t, pq)
            for fmt, siting in COMBOS:
                tag = (fmt, siting, str(dtype), pq)
                want = F.pack(codes, fmt, siting)
                got = _from_tensor(proc, t, fmt, siting, pq)
                assert np.array_equal(got, want), tag + _diff(got, want)
                got2 = _from_codes(proc, codes_dev, fmt, siting)
                assert np.array_equal(got2, want), tag + ("from codes",) + _diff(got2, want)
                got3 = proc.postprocess_ycbcr10(t, fmt, siting, pq=bool(pq), peak_nits=PEAK, dither="floyd_steinberg").cpu().numpy()
                assert np.array_equal(got3, want), tag + ("postprocess_ycbcr10",) + _diff(got3, want)
                if fmt == "p010le":                               # the value in the high ten bits, Cb and Cr interleaved
                    assert not (got & 63).any()
                    _, cb, cr = F.planes(codes, fmt, siting)
                    c = got[h * w:].reshape(h // 2, w)
                    assert np.array_equal(c[:, 0::2], cb) and np.array_equal(c[:, 1::2], cr)
                if h * w > 4:                                     # a rule of its own: not the plain rounding, not the ordered dither
                    assert not np.array_equal(want, R.pack(codes, fmt, siting)) and not np.array_equal(want, K.pack(codes, fmt, siting, 1)), tag


@pytest.mark.parametrize("shape", TALL_SHAPES, ids=lambda v: "%dx%d" % v)
def test_the_carried_row_between_row_groups(proc, shape):
    """More rows than a workgroup keeps in flight, in the luma plane and in the chroma planes: H = R + 3 is odd, so it is a 4:2:2
    frame (259 luma and chroma rows); H = 2 R + 6 gives the 4:2:0 layouts 518 luma and 259 chroma rows."""
    import torch
    h, w = shape
    combos = [c for c in COMBOS if (c[0] == "yuv422p10le") == bool(h & 1)]
    x = _input(h, w)
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        codes_dev, codes = _codes(proc, t, 0)
        for fmt, siting in combos:
            want = F.pack(codes, fmt, siting)
            got = _from_tensor(proc, t, fmt, siting, 0)
            assert np.array_equal(got, want), (fmt, siting, str(dtype)) + _diff(got, want)
            got2 = _from_codes(proc, codes_dev, fmt, siting)
            assert np.array_equal(got2, want), (fmt, siting, str(dtype), "from codes") + _diff(got2, want)


def test_one_row_of_422(proc):
    import torch
    t = torch.from_numpy(_input(1, 2)).cuda()
    codes_dev, codes = _codes(proc, t, 0)
    want = F.pack(codes, "yuv422p10le", "left")
    assert want.size == 4
    assert np.array_equal(_from_tensor(proc, t, "yuv422p10le", "left", 0), want)
    assert np.array_equal(_from_codes(proc, codes_dev, "yuv422p10le", "left"), want)


def test_pitched_unaligned_planes_match_and_padding_stays(proc):
    """y_pitch = 2 W + 2, a chroma pitch 6 bytes over its minimum, every plane base 2 bytes into its buffer."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 70, 132
    t = torch.from_numpy(_input(h, w)).cuda()
    codes_dev, codes = _codes(proc, t, 0)
    for fmt, siting in COMBOS:
        y, cb, cr = F.planes(codes, fmt, siting)
        if fmt == "p010le":
            c = np.empty((cb.shape[0], w), np.uint16)
            c[:, 0::2], c[:, 1::2] = cb, cr
            want_planes = [y, c]
        else:
            want_planes = [y, cb, cr]
        ch = h if fmt == "yuv422p10le" else h // 2
        cw = w if fmt == "p010le" else w // 2
        yp, cp = w + 1, cw + 3                                    # in u16
        for use_codes in (False, True):
            mk = lambda rows, pitch: torch.full((1 + rows * pitch + 5,), 0xA5A5, dtype=torch.uint16, device="cuda")      # noqa: E731
            by, bu = mk(h, yp), mk(ch, cp)
            bv = None if fmt == "p010le" else mk(ch, cp)
            tail = (L.YCC_FORMATS[fmt], L.YCC_SITINGS[siting], by.data_ptr() + 2, 2 * yp, bu.data_ptr() + 2,
                    None if bv is None else bv.data_ptr() + 2, 2 * cp, _scratch(proc, fmt, h, w).data_ptr())
            if use_codes:
                proc._chk(proc._lib.hdrtv_rgb48_to_ycbcr10_fs(proc._ctx, proc._stream(), codes_dev.data_ptr(), h, w, *tail), "rgb48_to_ycbcr10_fs")
            else:
                proc._chk(proc._lib.hdrtv_post_ycbcr10_fs(proc._ctx, proc._stream(), t.data_ptr(), L.F32, h, w, 0, 0.0, *tail), "post_ycbcr10_fs")
            bufs = [(by, h, w, yp), (bu, ch, cw, cp)] + ([] if bv is None else [(bv, ch, cw, cp)])
            for (buf, rows, n, pitch), want in zip(bufs, want_planes):
                buf = buf.cpu().numpy()
                expect = np.full(buf.shape, 0xA5A5, np.uint16)
                for r in range(rows):
                    expect[1 + r * pitch: 1 + r * pitch + n] = want[r]
                assert np.array_equal(buf, expect), (fmt, siting, use_codes, int((buf != expect).sum()))


def test_two_runs_and_two_streams_give_the_same_bytes(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 70, 132
    t = torch.from_numpy(_input(h, w)).cuda()
    codes_dev, codes = _codes(proc, t, 0)
    fmt, siting = "p010le", "topleft"
    want = F.pack(codes, fmt, siting)
    a = _from_codes(proc, codes_dev, fmt, siting, _scratch(proc, fmt, h, w, 0x00))
    b = _from_codes(proc, codes_dev, fmt, siting, _scratch(proc, fmt, h, w, 0xFF))
    assert a.tobytes() == b.tobytes() == want.tobytes()
    # two calls in flight on two streams, each with its own scratch
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dsts = [torch.full((want.size,), 0xA5A5, dtype=torch.uint16, device="cuda") for _ in streams]
    scratches = [_scratch(proc, fmt, h, w, 0x11 * (i + 1)) for i in range(2)]
    torch.cuda.synchronize()
    for s, d, sc in zip(streams, dsts, scratches):
        proc._chk(proc._lib.hdrtv_rgb48_to_ycbcr10_fs(proc._ctx, s.cuda_stream, codes_dev.data_ptr(), h, w,
                                                      *L.ycbcr10_planes(d.data_ptr(), h, w, fmt, siting), sc.data_ptr()), "rgb48_to_ycbcr10_fs")
    torch.cuda.synchronize()
    for d in dsts:
        assert np.array_equal(d.cpu().numpy(), want)


def test_refusals_leave_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 12, 20
    t = torch.rand((3, h, w), device="cuda")
    codes_dev, _ = _codes(proc, t, 0)
    dst = torch.full((h * w * 4,), 0xA5A5, dtype=torch.uint16, device="cuda")
    scratch = _scratch(proc, "yuv422p10le", h, w, 0x3C)
    ctx, st, i, o, sc = proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr(), scratch.data_ptr()
    u, v = o + 2 * h * w, o + 2 * h * w + h * w // 2
    ok = (L.YCC_YUV420P10, L.SITING_LEFT, o, 2 * w, u, v, w)
    f1, f2 = proc._lib.hdrtv_post_ycbcr10_fs, proc._lib.hdrtv_rgb48_to_ycbcr10_fs
    for bad_scratch in (None, sc + 2, sc + 1):                    # NULL, and not 4-byte aligned
        assert f1(ctx, st, i, L.F32, h, w, 0, 0.0, *ok, bad_scratch) == L.EINVAL
        assert f2(ctx, st, codes_dev.data_ptr(), h, w, *ok, bad_scratch) == L.EINVAL
    for a in ((h, w - 1) + ok, (h - 1, w) + ok, (h, w, 3) + ok[1:], (h, w, L.YCC_YUV422P10, L.SITING_TOPLEFT) + ok[2:],
              (h, w, L.YCC_P010) + ok[1:], (h, w) + ok[:3] + (2 * w - 2,) + ok[4:], (h, w) + ok[:2] + (None,) + ok[3:]):
        assert f1(ctx, st, i, L.F32, a[0], a[1], 0, 0.0, *a[2:], sc) == L.EINVAL, a
        assert f2(ctx, st, codes_dev.data_ptr(), *a, sc) == L.EINVAL, a
    assert f1(ctx, st, i, 2, h, w, 0, 0.0, *ok, sc) == L.EINVAL and f1(ctx, st, i, L.F32, h, w, 1, 0.0, *ok, sc) == L.EINVAL
    assert f1(ctx, st, None, L.F32, h, w, 0, 0.0, *ok, sc) == L.EINVAL and f2(ctx, st, None, h, w, *ok, sc) == L.EINVAL
    # the _ex entry points still refuse the code of the new name
    assert proc._lib.hdrtv_post_ycbcr10_ex(ctx, st, i, L.F32, h, w, 0, 0.0, *ok, L.DITHER_FS) == L.EINVAL
    assert proc._lib.hdrtv_rgb48_to_ycbcr10_ex(ctx, st, codes_dev.data_ptr(), h, w, *ok, L.DITHER_FS) == L.EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all() and (scratch.cpu().numpy() == 0x3C).all()
    with pytest.raises(ValueError):
        proc.postprocess_ycbcr10(t, "p010le", "left", dither="error_diffusion")


# ------------------------------------------------------------------------------------------------------------ the frame path
def test_post_out_routes_every_dither(proc):
    """_post_out: "none" and "ordered" deliver the bytes they deliver without this dither's name in the library; "floyd_steinberg"
    applies where "ordered" applies -- at the processing size, behind deband, and behind the scaler."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 34, 70
    t = torch.from_numpy(_input(h, w)).cuda()
    codes_dev, codes = _codes(proc, t, 0)
    st = proc._stream()
    for fmt, siting in (("yuv422p10le", "left"), ("p010le", "topleft")):
        out = L.output_format(fmt, siting, h, w)

        def deliver(cleanup, out=out, scale=None):
            dst = torch.full(out.shape, 0xA5A5, dtype=torch.uint16, device="cuda")
            proc._post_out(st, t.data_ptr(), L.F32, h, w, dst.data_ptr(), out, ("test_fs", fmt), cleanup=cleanup, scale=scale)
            return dst.cpu().numpy()

        assert np.array_equal(deliver(None), R.pack(codes, fmt, siting))
        assert np.array_equal(deliver(L.output_cleanup(dither="none")), R.pack(codes, fmt, siting))
        assert np.array_equal(deliver(L.output_cleanup(dither="ordered")), K.pack(codes, fmt, siting, 1))
        assert np.array_equal(deliver(L.output_cleanup(True, 9, 2500, "ordered")), K.cleanup(codes, fmt, siting, True, 9, 2500, 1))
        assert np.array_equal(deliver(L.output_cleanup(dither="floyd_steinberg")), F.pack(codes, fmt, siting))
        assert np.array_equal(deliver(L.output_cleanup(True, 9, 2500, "floyd_steinberg")), F.pack(K.deband(codes, 9, 2500), fmt, siting))
        # behind the scaler: the codes hdrtv_post_rgb48_scaled writes at twice the size
        big = L.output_format("rgb48le", siting, 2 * h, 2 * w)
        plan = L.SCALE_OFF.plan(w, h, 2 * w, 2 * h)
        rgb = torch.empty(big.shape, dtype=torch.uint16, device="cuda")
        proc._post_out(st, t.data_ptr(), L.F32, h, w, rgb.data_ptr(), big, ("test_fs", "big"), scale=plan)
        got = deliver(L.output_cleanup(dither="floyd_steinberg"), out=out.at(2 * h, 2 * w), scale=plan)
        assert np.array_equal(got, F.pack(rgb.cpu().numpy(), fmt, siting))
    with pytest.raises(ValueError):
        proc._post_out(st, t.data_ptr(), L.F32, h, w, codes_dev.data_ptr(), L.output_format("rgb48le", "left", h, w), "test_fs",
                       cleanup=L.OutputCleanup(False, 16, 1311, "floyd_steinberg"))


N = 2
PW, PH = 96, 64


@pytest.fixture(scope="module")
def weights_dir(golden_dir, tmp_path_factory):
    root = tmp_path_factory.mktemp("fs_weights")
    (root / "original").mkdir()
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), root / "original" / "HR.hdrw")
    return str(root)


def _run_worker(weights_dir, frames, **kw):
    """The frames through a worker and a collecting sink -> the delivered frames."""
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wk = HeadlessPipelineWorker(weights_dir, use_hg=False, proc_w=PW, proc_h=PH, **kw)
    assert wk._load_model("FP16") is True
    got, done = [], threading.Event()

    def sink(payload):
        got.append(payload.numpy().copy())
        payload.release()
        if len(got) == len(frames):
            done.set()

    wk._start_hdr_feeder(sink)
    try:
        for i, f in enumerate(frames):
            wk._process_frame(frame=f, frame_idx=i, mpv_w=True)
        assert done.wait(20.0)
    finally:
        wk._stop_hdr_feeder()
        wk.close()
    return got


def test_worker_delivers_deband_then_error_diffusion(weights_dir, golden_dir):
    from hdrtv_mi355x import weights as W
    frames = [np.load(os.path.join(golden_dir, "hr_64x96_noise_s0.npz"))["frame"], W.synthetic_frame(PH, PW, seed=71, kind="gradient")]
    base = _run_worker(weights_dir, frames)
    got = _run_worker(weights_dir, frames, out_pix_fmt="yuv422p10le", deband=True, dither="floyd_steinberg")
    for i in range(N):
        assert base[i].shape == (PH, PW, 3)
        want = F.pack(K.deband(base[i], 16, 1311), "yuv422p10le", "left")
        assert np.array_equal(got[i], want), (i,) + _diff(got[i], want)
