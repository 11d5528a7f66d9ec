"""hdrtv_post_rgb48_fsr on a real MI355X: the FSR upscale (EASU, optionally RCAS) of the RGB48 output, and the routes through
postprocess_rgb48_scaled, enqueue_frame, the worker and the dispatcher that carry the scaler.

The yardstick is always the composition: what the EXISTING unscaled entry point writes at the processing size (hdrtv_post_rgb48, or
hdrtv_post_pq_rgb48 for pq; pinned by the other GPU tests, so no quantiser is restated here), then tests/rgb48_fsr_ref (float32, op
by op).  Equality is exact: every value of every frame."""
import os
import threading

import numpy as np
import pytest

import rgb48_fsr_ref as F
import rgb48_scale_ref as S
import ycbcr10_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
MODES = (None, 0.2, 0.0, 2.0)        # rcas 0, then rcas 1 with the reference's sharpness and both ends of the range
# source (H, W) -> destination (dH, dW).  The kernel's tile is 32 x 64 output pixels.
SHAPES = [
    ((36, 52), (72, 104)),        # exact 2x, several tiles
    ((17, 33), (33, 65)),         # one output row and column past a tile: RCAS reads its ring across tile edges
    ((5, 7), (10, 14)),
    ((37, 53), (64, 101)),        # ragged ratios; odd dW: rows that are not 8-byte aligned, the store code by code
    ((33, 70), (34, 71)),         # a ratio next to 1: the largest footprint
    ((40, 48), (40, 96)),         # one axis at identity: the filter applies in full
    ((40, 48), (80, 48)),
    ((1, 1), (2, 2)),             # everything clamps
    ((1, 1), (1, 2)),
]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def contents(h, w):
    """The frames of the device test (tests/test_rgb48_fsr_host.py runs the reference over the same ones)."""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    step = np.full((3, h, w), 0.25, np.float32)               # the 0.25 / 0.75 step: red and blue along x, green along y
    step[:, :, w // 2:] = 0.75
    step[1] = np.where(yy >= h // 2, 0.75, 0.25)
    return {
        "noise": rng.uniform(-0.02, 1.02, (3, h, w)).astype(np.float32),          # the full range of codes, both clamps a little
        # codes 0 .. 3 only: tiny luma differences, the zero-direction branch, the reciprocal approximation at its largest
        "codes 0..3": (rng.integers(0, 4, (3, h, w)) / 65535.0).astype(np.float32),
        "step": step,
        "checkerboard": np.broadcast_to(((yy + xx) & 1).astype(np.float32), (3, h, w)).copy(),      # 0 / 65535
        "near white": rng.uniform(0.985, 1.0, (3, h, w)).astype(np.float32),
        "flat": np.full((3, h, w), 0.5, np.float32),
    }


def _unscaled(p, t, pq):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.empty((h, w, 3), dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    if pq:
        p._chk(p._lib.hdrtv_post_pq_rgb48(p._ctx, p._stream(), t.data_ptr(), dt, h, w, PEAK, o.data_ptr()), "post_pq_rgb48")
    else:
        p._chk(p._lib.hdrtv_post_rgb48(p._ctx, p._stream(), t.data_ptr(), dt, h, w, o.data_ptr()), "post_rgb48")
    return o.cpu().numpy()


def _fsr(p, t, pq, dh, dw, mode):
    """The C entry point itself; mode None = rcas 0, else rcas 1 with that sharpness."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    rcas, sharp = (0, 7.0) if mode is None else (1, mode)           # rcas 0 ignores the sharpness
    p._chk(p._lib.hdrtv_post_rgb48_fsr(p._ctx, p._stream(), t.data_ptr(), dt, h, w, pq, PEAK, o.data_ptr(), dh, dw, rcas, sharp), "post_rgb48_fsr")
    return o.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_fsr_equals_the_composition(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    total = 0
    for name, x in contents(h, w).items():
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(x).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                img = F.easu(codes, dh, dw)
                for mode in MODES:
                    want = F.quant(img if mode is None else F.rcas(img, mode))
                    got = _fsr(proc, t, pq, dh, dw, mode)
                    bad = got != want
                    print("%s %s pq=%d sharpness=%s: %d of %d values differ, largest |difference| %d" % (
                        name, str(dtype), pq, mode, int(bad.sum()), bad.size, int(np.abs(got.astype(int) - want.astype(int)).max())))
                    assert not bad.any(), (name, str(dtype), pq, mode)
                    total += 1
                if name == "noise" and h > 1 and pq == 0:              # the content gives both stages something to do
                    assert not np.array_equal(F.quant(img), F.quant(F.rcas(img, 0.2)))
                    assert not np.array_equal(F.quant(img), S.scale(codes, dh, dw))
    assert total == 6 * 2 * 2 * len(MODES)


def test_equal_sizes_are_the_unscaled_bytes(proc):
    import torch
    x = contents(36, 52)["noise"]
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes = _unscaled(proc, t, pq)
            for mode in MODES:
                assert np.array_equal(_fsr(proc, t, pq, 36, 52, mode), codes), (str(dtype), pq, mode)


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, dh, dw = 12, 20, 24, 33
    t = torch.rand((3, h, w), device="cuda")
    dst = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device="cuda")
    fn, ctx, st, i, o = proc._lib.hdrtv_post_rgb48_fsr, proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad = [(ctx, st, i, L.F32, h, w, 0, 0.0, o, 2 * h + 1, dw, 0, 0.2), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, 2 * w + 1, 0, 0.2),
           (ctx, st, i, L.F32, h, w, 0, 0.0, o, 2 * h + 1, 2 * w + 1, 1, 0.2)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, r, 0.2) for r in (2, -1, 256)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 1, s) for s in (-0.1, 2.5, nan, inf, -inf)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 1, 2.5), (ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 2, 0.2)]      # equal sizes too
    for r, s in ((0, 0.2), (1, 0.2)):        # the refusals of hdrtv_post_rgb48_scaled, RCAS off and on
        bad += [
            (None, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, r, s), (ctx, st, None, L.F32, h, w, 0, 0.0, o, dh, dw, r, s),
            (ctx, st, i, L.F32, h, w, 0, 0.0, None, dh, dw, r, s), (ctx, st, i, L.F32, 0, w, 0, 0.0, o, dh, dw, r, s),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, h - 1, dw, r, s), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, w - 1, r, s),
            (ctx, st, i, 2, h, w, 0, 0.0, o, dh, dw, r, s), (ctx, st, i, L.F32, h, w, 1, 0.0, o, dh, dw, r, s),
        ]
    for n, a in enumerate(bad):
        assert fn(*a) == L.EINVAL, n
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    assert fn(ctx, st, i, L.F32, h, w, 0, -5.0, o, dh, dw, 1, 0.2) == L.OK      # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), F.scale(_unscaled(proc, t, 0), dh, dw, 0.2))
    assert fn(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 0, nan) == L.OK       # rcas = 0 ignores the sharpness
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), F.scale(_unscaled(proc, t, 0), dh, dw))


def test_python_surface(proc):
    import torch
    t = torch.from_numpy(contents(36, 52)["noise"]).cuda()
    codes = _unscaled(proc, t, 0)
    run = lambda **kw: proc.postprocess_rgb48_scaled(t, 101, 64, **kw).cpu().numpy()      # noqa: E731
    n = len(proc._ycc_scratch)
    assert np.array_equal(run(scaler="fsr"), F.scale(codes, 64, 101, 0.2))                 # the reference's sharpness by default
    assert np.array_equal(run(scaler="FSR", fsr_sharpness=None), F.scale(codes, 64, 101))
    assert np.array_equal(run(scaler="fsr", fsr_sharpness=2, cas="auto", antiring="auto"), F.scale(codes, 64, 101, 2.0))
    assert np.array_equal(run(scaler="fsr", pq=True, peak_nits=PEAK), F.scale(_unscaled(proc, t, 1), 64, 101, 0.2))
    assert np.array_equal(proc.postprocess_rgb48_scaled(t, 52, 36, scaler="fsr").cpu().numpy(), codes)      # equal sizes
    # "lanczos", or leaving it out, gives the bytes of today's calls
    assert np.array_equal(run(), S.scale(codes, 64, 101)) and np.array_equal(run(scaler="lanczos", fsr_sharpness=1.0), run())
    assert len(proc._ycc_scratch) == n
    for kw in (dict(scaler="fsr", cas=0.2), dict(scaler="fsr", antiring=0.3), dict(scaler="bicubic"), dict(scaler=None),
               dict(scaler="fsr", fsr_sharpness=True), dict(scaler="fsr", fsr_sharpness="0.2"), dict(scaler="fsr", fsr_sharpness=float("nan")),
               dict(scaler="fsr", fsr_sharpness=-0.1), dict(scaler="fsr", fsr_sharpness=2.5)):
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError, match="2x"):
        proc.postprocess_rgb48_scaled(t, 105, 72, scaler="fsr")                            # 105 > 2 * 52


def test_enqueue_frame_and_everything_behind_the_scaler_see_the_fsr_codes(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 128, 192
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(W.synthetic_frame(h, w, seed=77, kind="noise")).cuda()
        st = torch.cuda.current_stream()
        new = lambda fmt, hh, ww: torch.full(L.output_format(fmt, "left", hh, ww).shape, 0xA5A5, dtype=torch.uint16, device="cuda")   # noqa: E731
        run = lambda dst, **kw: p.enqueue_frame(0, dev.data_ptr(), h, w, dst.data_ptr(), stream=st, **kw)                           # noqa: E731
        small, lan, lan2, fsr, easu, rag, same = (new("rgb48le", *s) for s in ((h, w), (oh, ow), (oh, ow), (oh, ow), (oh, ow), (100, 192), (h, w)))
        run(small)
        run(lan, out_hw=(oh, ow))
        run(lan2, out_hw=(oh, ow), scaler="lanczos")
        run(fsr, out_hw=(oh, ow), scaler="fsr", cas="auto", antiring="auto")
        run(easu, out_hw=(oh, ow), scaler="fsr", fsr_sharpness=None)
        run(rag, out_hw=(100, 192), scaler="fsr", fsr_sharpness=0.0)
        run(same, scaler="fsr")                                     # nothing is enlarged: the unscaled frame
        torch.cuda.synchronize()
        codes = small.cpu().numpy()
        assert np.array_equal(lan.cpu().numpy(), S.scale(codes, oh, ow)) and np.array_equal(lan2.cpu().numpy(), lan.cpu().numpy())
        assert np.array_equal(fsr.cpu().numpy(), F.scale(codes, oh, ow, 0.2))
        assert np.array_equal(easu.cpu().numpy(), F.scale(codes, oh, ow))
        assert np.array_equal(rag.cpu().numpy(), F.scale(codes, 100, 192, 0.0))
        assert np.array_equal(same.cpu().numpy(), codes)
        assert not np.array_equal(fsr.cpu().numpy(), lan.cpu().numpy()) and not np.array_equal(fsr.cpu().numpy(), easu.cpu().numpy())
        # a scaled yuv420p10le frame = the conversion of the FSR codes; its record = the statistic of those codes
        ycc = new("yuv420p10le", oh, ow)
        rec, want_rec = (torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") for _ in range(2))
        run(ycc, out_hw=(oh, ow), out_pix_fmt="yuv420p10le", scaler="fsr", light_ptr=rec.data_ptr())
        p._chk(p._lib.hdrtv_rgb48_light_stats(p._ctx, p._stream(), fsr.data_ptr(), oh, ow, 0, 0, ow, oh, want_rec.data_ptr()), "rgb48_light_stats")
        torch.cuda.synchronize()
        assert np.array_equal(ycc.cpu().numpy().reshape(-1), R.pack(fsr.cpu().numpy(), "yuv420p10le", "left").reshape(-1))
        assert np.array_equal(rec.cpu().numpy(), want_rec.cpu().numpy())
        # deband sits behind the scaler too
        deb, want_deb = new("rgb48le", oh, ow), None
        run(deb, out_hw=(oh, ow), scaler="fsr", cleanup=L.output_cleanup(True))
        torch.cuda.synchronize()
        want_deb = p.postprocess_deband(fsr).cpu().numpy()
        assert np.array_equal(deb.cpu().numpy(), want_deb)
        # the 4:2:0 input path carries the scaler too
        yuv = torch.from_numpy(np.random.default_rng(3).integers(16, 236, (h * 3 // 2, w)).astype(np.uint8)).cuda()
        ysmall, ybig = new("rgb48le", h, w), new("rgb48le", oh, ow)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ysmall.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ybig.data_ptr(), stream=st, out_hw=(oh, ow), scaler="fsr", fsr_sharpness=2.0)
        torch.cuda.synchronize()
        assert np.array_equal(ybig.cpu().numpy(), F.scale(ysmall.cpu().numpy(), oh, ow, 2.0))
        for kw in (dict(scaler="fsr", cas=0.2), dict(scaler="fsr", antiring=0.1), dict(scaler="nearest"), dict(scaler="fsr", fsr_sharpness=3)):
            with pytest.raises(ValueError):
                run(fsr, out_hw=(oh, ow), **kw)
        with pytest.raises(ValueError, match="2x"):
            run(new("rgb48le", 129, 192), out_hw=(129, 192), scaler="fsr")
    finally:
        p.close()


def _run_worker(golden_dir, tmp_path, tag, frames, **kw):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / tag / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    wk = HeadlessPipelineWorker(str(tmp_path / tag), use_hg=True, proc_w=96, proc_h=64, hg_weights="seeded:1234", buffer_frames=2, **kw)
    assert wk._load_model("FP16", warmup=False)
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
        assert done.wait(30.0)
    finally:
        wk._stop_hdr_feeder()
        wk.close()
    return got


def test_worker_delivers_a_p010_frame_through_fsr(golden_dir, tmp_path):
    from hdrtv_mi355x import weights as W
    oh, ow = 128, 192
    frames = [W.synthetic_frame(64, 96, seed=60 + i, kind="noise") for i in range(2)]
    base = _run_worker(golden_dir, tmp_path, "plain", frames, scaler="fsr")                    # nothing enlarged: the unscaled frames
    fsr = _run_worker(golden_dir, tmp_path, "fsr", frames, out_w=ow, out_h=oh, out_pix_fmt="p010le", scaler="fsr", cas="auto", antiring="auto")
    for i in range(2):
        assert base[i].shape == (64, 96, 3)
        assert np.array_equal(fsr[i].reshape(-1), R.pack(F.scale(base[i], oh, ow, 0.2), "p010le", "left").reshape(-1)), i
        assert not np.array_equal(fsr[i].reshape(-1), R.pack(S.scale(base[i], oh, ow), "p010le", "left").reshape(-1))


def test_dispatcher_workers_apply_the_scaler(golden_dir):
    import torch
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.dispatch import FrameDispatcher
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 100, 192
    frame = W.synthetic_frame(h, w, seed=80, kind="noise")
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    dev = torch.from_numpy(frame).cuda()
    p.enqueue_frame(0, dev.data_ptr(), h, w, u16.data_ptr(), stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    want = F.scale(u16.cpu().numpy(), oh, ow, 0.5)
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_height=oh, out_width=ow, scaler="fsr", fsr_sharpness=0.5, cas="auto") as d:
        assert d.scaler == "fsr" and d.fsr_sharpness == 0.5 and d.cas == 0.0
        d.submit(frame)
        d.flush(timeout=120)
    assert d.exit_codes == [0] and sorted(got) == [0]
    assert got[0].shape == (oh, ow, 3) and np.array_equal(got[0], want)
