"""hdrtv_post_rgb48_scaled on a real MI355X: RGB48 at the display size, the quantiser and the Lanczos upscale in one kernel.

The yardstick is always tests/rgb48_scale_ref.scale() of what the EXISTING entry point writes at the processing size
(hdrtv_post_rgb48, or hdrtv_post_pq_rgb48 for pq) -- those are pinned by the other GPU tests, so no quantiser is restated here.
Equality is exact: every value of every frame."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import rgb48_scale_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
# source (H, W) -> destination (dH, dW).  The kernel's tile is 32 x 64 output pixels.
SHAPES = [
    ((36, 52), (72, 104)),        # exact 2x
    ((36, 52), (97, 131)),        # non-integer, another ratio per axis, odd output: ragged tiles, rows that are not 8-byte aligned
    ((5, 7), (64, 200)),          # fewer source samples than taps: both clamps at once, ratios up to ~28
    ((100, 150), (257, 333)),     # nine tiles down, six across, ragged on both axes
    ((61, 103), (61, 103)),       # the unscaled entry point's bytes
    ((61, 103), (61, 206)),       # one axis at identity
    ((61, 103), (122, 103)),
]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _contents(h, w):
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    step = np.zeros((3, h, w), np.float32)
    step[:, :, w // 2:] = 1.0
    step[1] = yy >= h // 2                                    # green steps along the other axis
    return {
        "uniform": rng.uniform(-0.25, 1.25, (3, h, w)).astype(np.float32),          # both clamps of the quantiser act
        "checker": np.broadcast_to(((yy + xx) & 1).astype(np.float32), (3, h, w)).copy(),
        "step": step.astype(np.float32),
        "flat": np.full((3, h, w), 0.61, np.float32),
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


def _scaled(p, t, pq, dh, dw):
    out = p.postprocess_rgb48_scaled(t, dw, dh, pq=bool(pq), peak_nits=PEAK)
    assert tuple(out.shape) == (dh, dw, 3) and str(out.dtype) == "torch.uint16"
    return out.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_scaled_equals_the_rule_applied_to_the_unscaled_codes(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    for name, x in _contents(h, w).items():
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(x).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                want = R.scale(codes, dh, dw)
                got = _scaled(proc, t, pq, dh, dw)
                assert np.array_equal(got, want), (name, str(dtype), pq, int((got != want).sum()),
                                                   int(np.abs(got.astype(int) - want.astype(int)).max()))
                if (dh, dw) == (h, w):
                    assert np.array_equal(got, codes)
                if name == "flat":
                    assert (got == codes[0, 0]).all()
                if name in ("checker", "step") and (dh, dw) != (h, w) and not pq:
                    assert got.min() == 0 and got.max() == 65535


def test_tables_are_cached_per_geometry(proc):
    import torch
    t = torch.from_numpy(_contents(36, 52)["uniform"]).cuda()
    a1 = _scaled(proc, t, 0, 97, 131)
    b = _scaled(proc, t, 0, 131, 97)
    c = _scaled(proc, t[:, :30, :40].contiguous(), 0, 97, 131)      # another source size onto the first output size
    a2 = _scaled(proc, t, 0, 97, 131)
    codes = _unscaled(proc, t, 0)
    assert np.array_equal(a1, a2) and np.array_equal(a1, R.scale(codes, 97, 131))
    assert np.array_equal(b, R.scale(codes, 131, 97))
    assert np.array_equal(c, R.scale(np.ascontiguousarray(codes[:30, :40]), 97, 131))


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, dh, dw = 12, 20, 30, 44
    t = torch.rand((3, h, w), device="cuda")
    dst = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device="cuda")
    fn, ctx, st, i, o = proc._lib.hdrtv_post_rgb48_scaled, proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    bad = [
        (None, st, i, L.F32, h, w, 0, 0.0, o, dh, dw), (ctx, st, None, L.F32, h, w, 0, 0.0, o, dh, dw),
        (ctx, st, i, L.F32, h, w, 0, 0.0, None, dh, dw),
        (ctx, st, i, L.F32, 0, w, 0, 0.0, o, dh, dw), (ctx, st, i, L.F32, h, 0, 0, 0.0, o, dh, dw),
        (ctx, st, i, L.F32, -h, w, 0, 0.0, o, dh, dw), (ctx, st, i, L.F32, h, -w, 0, 0.0, o, dh, dw),
        (ctx, st, i, L.F32, h, w, 0, 0.0, o, 0, dw), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, 0),
        (ctx, st, i, L.F32, h, w, 0, 0.0, o, -dh, dw), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, -dw),
        (ctx, st, i, L.F32, h, w, 0, 0.0, o, h - 1, dw), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, w - 1),
        (ctx, st, i, 2, h, w, 0, 0.0, o, dh, dw), (ctx, st, i, -1, h, w, 0, 0.0, o, dh, dw),
        (ctx, st, i, L.F32, h, w, 1, 0.0, o, dh, dw), (ctx, st, i, L.F32, h, w, 1, -100.0, o, dh, dw),
    ]
    for k, a in enumerate(bad):
        assert fn(*a) == L.EINVAL, k
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    assert fn(ctx, st, i, L.F32, h, w, 0, -5.0, o, dh, dw) == L.OK          # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), R.scale(_unscaled(proc, t, 0), dh, dw))
    with pytest.raises(ValueError):
        proc.postprocess_rgb48_scaled(t, w - 1, dh)


def test_enqueue_frame_delivers_at_the_output_size(golden_dir):
    import torch
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 128, 192
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        frame = W.synthetic_frame(h, w, seed=77, kind="noise")
        dev = torch.from_numpy(frame).cuda()
        st = torch.cuda.current_stream()
        small = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
        big = torch.empty((oh, ow, 3), dtype=torch.uint16, device="cuda")
        p.enqueue_frame(0, dev.data_ptr(), h, w, small.data_ptr(), stream=st)
        p.enqueue_frame(0, dev.data_ptr(), h, w, big.data_ptr(), stream=st, out_hw=(oh, ow))
        same = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
        p.enqueue_frame(0, dev.data_ptr(), h, w, same.data_ptr(), stream=st, out_hw=(h, w))
        # the 4:2:0 form: grey planes
        yuv = torch.full((h * 3 // 2, w), 128, dtype=torch.uint8, device="cuda")
        ysmall, ybig = torch.empty_like(small), torch.empty_like(big)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ysmall.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ybig.data_ptr(), stream=st, out_hw=(oh, ow))
        torch.cuda.synchronize()
        assert np.array_equal(big.cpu().numpy(), R.scale(small.cpu().numpy(), oh, ow))
        assert np.array_equal(same.cpu().numpy(), small.cpu().numpy())
        assert np.array_equal(ybig.cpu().numpy(), R.scale(ysmall.cpu().numpy(), oh, ow))
    finally:
        p.close()


def _run_worker(golden_dir, tmp_path, tag, frames, **kw):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / tag / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    wk = HeadlessPipelineWorker(str(tmp_path / tag), use_hg=True, proc_w=96, proc_h=64, hg_weights="seeded:1234", **kw)
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
        ring = wk._ring_shape
        wk.close()
    return got, ring


def test_worker_delivers_at_the_output_size(golden_dir, tmp_path):
    from hdrtv_mi355x import weights as W
    oh, ow = 150, 250
    frames = [W.synthetic_frame(64, 96, seed=60 + i, kind="noise") for i in range(3)]
    base, ring0 = _run_worker(golden_dir, tmp_path, "plain", frames, buffer_frames=3)
    big, ring1 = _run_worker(golden_dir, tmp_path, "scaled", frames, buffer_frames=3, out_w=ow, out_h=oh)
    assert ring0 == (64, 96) and ring1 == (oh, ow)
    assert len(base) == len(big) == 3
    for i in range(3):
        assert base[i].shape == (64, 96, 3) and big[i].shape == (oh, ow, 3)
        assert np.array_equal(big[i], R.scale(base[i], oh, ow)), i


def test_dispatcher_delivers_at_the_output_size(golden_dir):
    import torch
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.dispatch import FrameDispatcher
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 100, 192
    frames = [W.synthetic_frame(h, w, seed=80 + i, kind="noise") for i in range(2)]
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    want = []
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    for f in frames:
        dev = torch.from_numpy(f).cuda()
        p.enqueue_frame(0, dev.data_ptr(), h, w, u16.data_ptr(), stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        want.append(R.scale(u16.cpu().numpy(), oh, ow))
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_height=oh, out_width=ow) as d:
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0]
    assert sorted(got) == [0, 1]
    for i in range(2):
        assert got[i].shape == (oh, ow, 3) and np.array_equal(got[i], want[i]), i
