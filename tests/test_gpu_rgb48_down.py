"""hdrtv_post_rgb48_down on a real MI355X: the Mitchell / SSimDownscaler shrink of the RGB48 output, and the routes through
postprocess_rgb48_scaled, enqueue_frame, the worker and the dispatcher that carry the downscaler.

The yardstick is always the composition: what the EXISTING unscaled entry point writes at the processing size (hdrtv_post_rgb48, or
hdrtv_post_pq_rgb48 for pq; pinned by the other GPU tests, so no quantiser is restated here), then tests/rgb48_down_ref (stage A in
integers, stage B in float32, op by op).  Equality is exact: every value of every frame."""
import os
import threading

import numpy as np
import pytest

import rgb48_down_ref as D
import ycbcr10_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
MODES = ((0, 0), (51, 0), (256, 0), (0, 1), (51, 1))          # (anti-ringing code, ssim)
# source (H, W) -> destination (dH, dW).  The kernel's tile is 16 x 32 output pixels up to a ratio of 2 on both axes, 8 x 32 above.
SHAPES = [
    ((72, 104), (36, 52)),        # exact 2x, several tiles
    ((99, 156), (33, 52)),        # 3x: the small tile
    ((128, 192), (32, 48)),       # 4x, 17 taps
    ((101, 64), (37, 53)),        # ragged, odd dW
    ((34, 71), (33, 70)),         # a ratio next to 1
    ((41, 43), (11, 11)),         # just inside 4x
    ((40, 96), (40, 48)),         # one axis at identity
    ((80, 48), (40, 48)),
    ((4, 4), (1, 1)),             # everything clamps, the 3 x 3 ring is all one pixel
    ((3, 2), (1, 1)),
    ((2, 1), (1, 1)),
    ((30, 60), (17, 33)),         # the 16 x 32 tile plus one row and one column: stage B's two-pixel ring crosses tile edges
    ((27, 99), (9, 33)),          # the 8 x 32 tile plus one row and one column
]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def contents(h, w):
    """The frames of the device test."""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    step = np.full((3, h, w), 0.25, np.float32)               # the 0.25 / 0.75 step: red and blue along x, green along y
    step[:, :, w // 2:] = 0.75
    step[1] = np.where(yy >= h // 2, 0.75, 0.25)
    return {
        "noise": rng.uniform(-0.02, 1.02, (3, h, w)).astype(np.float32),          # the full range of codes, both clamps a little
        "codes 0..3": (rng.integers(0, 4, (3, h, w)) / 65535.0).astype(np.float32),        # tiny variances: the sigma branch, denormal products
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


def _down(p, t, pq, dh, dw, a, ssim, peak=PEAK):
    """The C entry point itself."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    p._chk(p._lib.hdrtv_post_rgb48_down(p._ctx, p._stream(), t.data_ptr(), dt, h, w, pq, peak, o.data_ptr(), dh, dw, a, ssim), "post_rgb48_down")
    return o.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_down_equals_the_composition(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    total = 0
    for name, x in contents(h, w).items():
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(x).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                mit = {a: D.mitchell(codes, dh, dw, a) for a in (0, 51, 256)}
                for a, ssim in MODES:
                    want = D.ssim(codes, mit[a], dh, dw) if ssim else mit[a]
                    got = _down(proc, t, pq, dh, dw, a, ssim)
                    bad = got != want
                    print("%s %s pq=%d a=%d ssim=%d: %d of %d values differ, largest |difference| %d" % (
                        name, str(dtype), pq, a, ssim, int(bad.sum()), bad.size, int(np.abs(got.astype(int) - want.astype(int)).max())))
                    assert not bad.any(), (name, str(dtype), pq, a, ssim)
                    total += 1
                if name == "noise" and dh > 8 and pq == 0:             # the content gives both stages something to do
                    assert not np.array_equal(mit[0], D.ssim(codes, mit[0], dh, dw))
    assert total == 6 * 2 * 2 * len(MODES)


def test_equal_sizes_are_the_unscaled_bytes(proc):
    import torch
    x = contents(36, 52)["noise"]
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes = _unscaled(proc, t, pq)
            for a, ssim in MODES:
                assert np.array_equal(_down(proc, t, pq, 36, 52, a, ssim), codes), (str(dtype), pq, a, ssim)


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, dh, dw = 41, 64, 11, 33
    t = torch.rand((3, h, w), device="cuda")
    dst = torch.full((h, w, 3), 0xA5A5, dtype=torch.uint16, device="cuda")
    fn, ctx, st, i, o = proc._lib.hdrtv_post_rgb48_down, proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    bad = [(ctx, st, i, L.F32, h, w, 0, 0.0, o, h + 1, dw, 0, 0), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, w + 1, 0, 1),      # enlarging, mixed
           (ctx, st, i, L.F32, h, w, 0, 0.0, o, 10, dw, 0, 0),              # 4 * 10 == 41 - 1
           (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, 15, 0, 1),              # 4 * 15 < 64
           (ctx, st, i, L.F32, h, w, 0, 0.0, o, 10, 15, 51, 1)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, a, 0) for a in (-1, 257, 1 << 20)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 0, s) for s in (2, -1, 256)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 257, 0), (ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 0, 2)]      # equal sizes too
    for a, s in ((0, 0), (51, 1)):
        bad += [
            (None, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, a, s), (ctx, st, None, L.F32, h, w, 0, 0.0, o, dh, dw, a, s),
            (ctx, st, i, L.F32, h, w, 0, 0.0, None, dh, dw, a, s), (ctx, st, i, L.F32, 0, w, 0, 0.0, o, dh, dw, a, s),
            (ctx, st, i, L.F32, h, 0, 0, 0.0, o, dh, dw, a, s), (ctx, st, i, L.F32, h, w, 0, 0.0, o, 0, dw, a, s),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, -3, a, s), (ctx, st, i, 2, h, w, 0, 0.0, o, dh, dw, a, s),
            (ctx, st, i, L.F32, h, w, 1, 0.0, o, dh, dw, a, s), (ctx, st, i, L.F32, h, w, 1, -1.0, o, dh, dw, a, s),
        ]
    for n, a in enumerate(bad):
        assert fn(*a) == L.EINVAL, n
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    # the existing entry points keep their refusal of a smaller size
    assert proc._lib.hdrtv_post_rgb48_scaled(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw) == L.EINVAL
    assert proc._lib.hdrtv_post_rgb48_fsr(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 1, 0.2) == L.EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    codes = _unscaled(proc, t, 0)
    assert np.array_equal(_down(proc, t, 0, dh, dw, 51, 1, peak=-5.0), D.scale(codes, dh, dw, 51, True))      # pq = 0 ignores peak_nits
    assert np.array_equal(_down(proc, t, 0, 11, 16, 0, 0, peak=0.0), D.scale(codes, 11, 16))                    # 4 * 11 >= 41, 4 * 16 == 64


def test_python_surface(proc):
    import torch
    t = torch.from_numpy(contents(72, 104)["noise"]).cuda()
    codes = _unscaled(proc, t, 0)
    run = lambda ow=53, oh=37, **kw: proc.postprocess_rgb48_scaled(t, ow, oh, **kw).cpu().numpy()      # noqa: E731
    assert np.array_equal(run(downscaler="mitchell"), D.scale(codes, 37, 53))
    assert np.array_equal(run(downscaler="SSIM"), D.scale(codes, 37, 53, 0, True))
    assert np.array_equal(run(downscaler="ssim", down_antiring="auto", antiring="auto", cas="auto"), D.scale(codes, 37, 53, 51, True))
    assert np.array_equal(run(downscaler="mitchell", down_antiring=1.0), D.scale(codes, 37, 53, 256))
    assert np.array_equal(run(downscaler="ssim", pq=True, peak_nits=PEAK), D.scale(_unscaled(proc, t, 1), 37, 53, 0, True))
    assert np.array_equal(run(104, 36, downscaler="ssim"), D.scale(codes, 36, 104, 0, True))            # one axis at identity
    for kw in (dict(), dict(downscaler=None), dict(scaler="fsr"), dict(antiring="auto"),                    # as before: a smaller size raises
               dict(downscaler="mitchell", scaler="fsr"), dict(downscaler="ssim", cas=0.2), dict(downscaler="ssim", antiring=0.3),
               dict(downscaler="lanczos"), dict(downscaler=True), dict(downscaler="ssim", down_antiring=1.5),
               dict(downscaler="ssim", down_antiring="strong"), dict(down_antiring=0.2)):
        with pytest.raises(ValueError):
            run(**kw)
    for ow, oh in ((105, 37), (53, 73), (104, 72), (25, 37), (53, 17), (208, 144)):      # mixed, nothing to shrink, more than 4x, enlarging
        with pytest.raises(ValueError):
            run(ow, oh, downscaler="ssim")


def test_enqueue_frame_and_everything_behind_the_scaler_see_the_shrunk_codes(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 128, 192, 64, 96
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(W.synthetic_frame(h, w, seed=77, kind="noise")).cuda()
        st = torch.cuda.current_stream()
        new = lambda fmt, hh, ww: torch.full(L.output_format(fmt, "left", hh, ww).shape, 0xA5A5, dtype=torch.uint16, device="cuda")   # noqa: E731
        run = lambda dst, **kw: p.enqueue_frame(0, dev.data_ptr(), h, w, dst.data_ptr(), stream=st, **kw)                           # noqa: E731
        full, mit, ssim, rag = (new("rgb48le", *s) for s in ((h, w), (oh, ow), (oh, ow), (50, 192)))
        run(full)
        run(mit, out_hw=(oh, ow), downscaler="mitchell", down_antiring="auto")
        run(ssim, out_hw=(oh, ow), downscaler="ssim", antiring="auto", cas="auto")
        run(rag, out_hw=(50, 192), downscaler="ssim", down_antiring=1.0)
        torch.cuda.synchronize()
        codes = full.cpu().numpy()
        assert np.array_equal(mit.cpu().numpy(), D.scale(codes, oh, ow, 51))
        assert np.array_equal(ssim.cpu().numpy(), D.scale(codes, oh, ow, 0, True))
        assert np.array_equal(rag.cpu().numpy(), D.scale(codes, 50, 192, 256, True))
        assert not np.array_equal(ssim.cpu().numpy(), D.scale(codes, oh, ow))
        # a shrunk yuv420p10le frame = the conversion of the shrunk codes; its record = the statistic of those codes
        ycc = new("yuv420p10le", oh, ow)
        rec, want_rec = (torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") for _ in range(2))
        run(ycc, out_hw=(oh, ow), out_pix_fmt="yuv420p10le", downscaler="ssim", light_ptr=rec.data_ptr())
        p._chk(p._lib.hdrtv_rgb48_light_stats(p._ctx, p._stream(), ssim.data_ptr(), oh, ow, 0, 0, ow, oh, want_rec.data_ptr()), "rgb48_light_stats")
        torch.cuda.synchronize()
        assert np.array_equal(ycc.cpu().numpy().reshape(-1), R.pack(ssim.cpu().numpy(), "yuv420p10le", "left").reshape(-1))
        assert np.array_equal(rec.cpu().numpy(), want_rec.cpu().numpy())
        # deband sits behind the shrink too
        deb = new("rgb48le", oh, ow)
        run(deb, out_hw=(oh, ow), downscaler="ssim", cleanup=L.output_cleanup(True))
        torch.cuda.synchronize()
        assert np.array_equal(deb.cpu().numpy(), p.postprocess_deband(ssim).cpu().numpy())
        # the 4:2:0 input path carries the option too
        yuv = torch.from_numpy(np.random.default_rng(3).integers(16, 236, (h * 3 // 2, w)).astype(np.uint8)).cuda()
        yfull, ysmall = new("rgb48le", h, w), new("rgb48le", oh, ow)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, yfull.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ysmall.data_ptr(), stream=st, out_hw=(oh, ow), downscaler="ssim", down_antiring=0.2)
        torch.cuda.synchronize()
        assert np.array_equal(ysmall.cpu().numpy(), D.scale(yfull.cpu().numpy(), oh, ow, 51, True))
        for kw in (dict(downscaler="ssim", scaler="fsr"), dict(downscaler="ssim", cas=0.2), dict(downscaler="ssim", antiring=0.1),
                   dict(downscaler="area"), dict(downscaler="ssim", down_antiring=3)):
            with pytest.raises(ValueError):
                run(ssim, out_hw=(oh, ow), **kw)
        for hw in ((31, 96), (64, 193), (h, w)):                      # more than 4x, mixed, nothing to shrink
            with pytest.raises(ValueError):
                run(full, out_hw=hw, downscaler="ssim")
        with pytest.raises(ValueError):
            run(full, downscaler="mitchell")                          # no out_hw: nothing to shrink
    finally:
        p.close()


def _run_worker(golden_dir, tmp_path, tag, frames, **kw):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / tag / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    wk = HeadlessPipelineWorker(str(tmp_path / tag), use_hg=True, proc_w=192, proc_h=128, hg_weights="seeded:1234", buffer_frames=2, **kw)
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


def test_worker_delivers_a_p010_frame_through_ssim(golden_dir, tmp_path):
    from hdrtv_mi355x import weights as W
    oh, ow = 64, 96
    frames = [W.synthetic_frame(128, 192, seed=60 + i, kind="noise") for i in range(2)]
    base = _run_worker(golden_dir, tmp_path, "plain", frames)
    got = _run_worker(golden_dir, tmp_path, "ssim", frames, out_w=ow, out_h=oh, out_pix_fmt="p010le", downscaler="ssim", down_antiring="auto")
    for i in range(2):
        assert base[i].shape == (128, 192, 3)
        assert np.array_equal(got[i].reshape(-1), R.pack(D.scale(base[i], oh, ow, 51, True), "p010le", "left").reshape(-1)), i
        assert not np.array_equal(got[i].reshape(-1), R.pack(D.scale(base[i], oh, ow, 51), "p010le", "left").reshape(-1))


def test_dispatcher_workers_apply_the_downscaler(golden_dir):
    import torch
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.dispatch import FrameDispatcher
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 128, 192, 50, 96
    frame = W.synthetic_frame(h, w, seed=80, kind="noise")
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    dev = torch.from_numpy(frame).cuda()
    p.enqueue_frame(0, dev.data_ptr(), h, w, u16.data_ptr(), stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    want = D.scale(u16.cpu().numpy(), oh, ow, 128, True)
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_height=oh, out_width=ow, downscaler="ssim", down_antiring=0.5, cas="auto") as d:
        assert d.downscaler == "ssim" and d.down_antiring == 0.5
        d.submit(frame)
        d.flush(timeout=120)
    assert d.exit_codes == [0] and sorted(got) == [0]
    assert got[0].shape == (oh, ow, 3) and np.array_equal(got[0], want)
