"""hdrtv_post_rgb48_scaled_ex on a real MI355X: the fused quantiser + Lanczos upscale with anti-ringing, and the routes through
enqueue_frame, the worker and the dispatcher that carry the strength.

The yardstick is always tests/rgb48_antiring_ref.scale() of what the EXISTING entry point writes at the processing size
(hdrtv_post_rgb48, or hdrtv_post_pq_rgb48 for pq) -- those are pinned by the other GPU tests, so no quantiser is restated here.
Equality is exact: every value of every frame."""
import os
import threading

import numpy as np
import pytest

import rgb48_antiring_ref as A

pytestmark = pytest.mark.gpu

PEAK = 1000.0
# source (H, W) -> destination (dH, dW).  The kernel's tile is 32 x 64 output pixels.
SHAPES = [
    ((36, 52), (72, 104)),        # exact 2x
    ((36, 52), (97, 131)),        # non-integer, another ratio per axis, odd output: ragged tiles, rows that are not 8-byte aligned
    ((5, 7), (64, 200)),          # fewer source samples than taps: both clamps at once, ratios up to ~28
    ((100, 150), (257, 333)),     # nine tiles down, six across, ragged on both axes
    ((61, 103), (61, 206)),       # one axis at identity: that pass must not move
    ((61, 103), (122, 103)),
    ((61, 103), (61, 103)),       # equal sizes: the unscaled entry point's bytes whatever the strength
]
STRENGTHS = (0, 26, 77, 256)     # off, the reference's 0.10 and 0.30, full


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _contents(h, w):
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    step = np.full((3, h, w), 0.25, np.float32)               # the 0.25 / 0.75 step: red and blue along x, green along y
    step[:, :, w // 2:] = 0.75
    step[1] = np.where(yy >= h // 2, 0.75, 0.25)
    return {
        "uniform": rng.uniform(-0.25, 1.25, (3, h, w)).astype(np.float32),          # both clamps of the quantiser act
        "checker": np.broadcast_to(((yy + xx) & 1).astype(np.float32), (3, h, w)).copy(),
        "step": step,
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


def _ex(p, t, pq, dh, dw, a):
    """The C entry point itself, with the strength as its code."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    p._chk(p._lib.hdrtv_post_rgb48_scaled_ex(p._ctx, p._stream(), t.data_ptr(), dt, h, w, pq, PEAK, o.data_ptr(), dh, dw, a), "scaled_ex")
    return o.cpu().numpy()


def _plain(p, t, pq, dh, dw):
    return p.postprocess_rgb48_scaled(t, dw, dh, pq=bool(pq), peak_nits=PEAK).cpu().numpy()


def _check(p, t, pq, dh, dw, a, codes, name):
    want = A.scale(codes, dh, dw, a)
    got = _ex(p, t, pq, dh, dw, a)
    bad = got != want
    print("%s %s pq=%d a=%d: %d of %d values differ, largest |difference| %d" % (
        name, str(t.dtype), pq, a, int(bad.sum()), bad.size, int(np.abs(got.astype(int) - want.astype(int)).max())))
    assert not bad.any(), (name, str(t.dtype), pq, a)
    return got


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_ex_equals_the_rule_applied_to_the_unscaled_codes(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    for name, x in _contents(h, w).items():
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(x).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                plain = _plain(proc, t, pq, dh, dw)
                lo, hi = A.envelope(codes, dh, dw)
                for a in STRENGTHS:
                    got = _check(proc, t, pq, dh, dw, a, codes, name)
                    if a == 0:
                        assert np.array_equal(got, plain)                       # hdrtv_post_rgb48_scaled's bytes
                    if a == 256:
                        assert (got >= lo).all() and (got <= hi).all()          # inside the 2 x 2 source codes around each sample
                    if (dh, dw) == (h, w):
                        assert np.array_equal(got, codes)
                    if name == "flat":
                        assert (got == codes[0, 0]).all()
                if name == "step" and (dh, dw) != (h, w):                       # the content gives the rule something to do
                    assert ((plain > hi) | (plain < lo)).any()


def test_strengths_next_to_the_ends(proc):
    import torch
    (h, w), (dh, dw) = (36, 52), (97, 131)
    for name in ("uniform", "step"):
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(_contents(h, w)[name]).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                for a in (1, 255):
                    _check(proc, t, pq, dh, dw, a, codes, name)


def test_python_surface_maps_the_strength_and_shares_the_tables(proc):
    import torch
    from hdrtv_mi355x import lib as L
    t = torch.from_numpy(_contents(36, 52)["uniform"]).cuda()
    codes = _unscaled(proc, t, 0)
    run = lambda **kw: proc.postprocess_rgb48_scaled(t, 131, 97, **kw).cpu().numpy()      # noqa: E731
    n = len(proc._ycc_scratch)
    assert np.array_equal(run(antiring=0.3), A.scale(codes, 97, 131, 77))
    assert np.array_equal(run(), A.scale(codes, 97, 131, 0)) and np.array_equal(run(antiring=0.0), run())
    assert np.array_equal(run(antiring=1.0), A.scale(codes, 97, 131, 256))
    assert np.array_equal(run(antiring="auto"), A.scale(codes, 97, 131, L.antiring_code(L.scale_antiring(52, 36, 131, 97))))
    assert L.scale_antiring(52, 36, 131, 97) == 0.30
    assert np.array_equal(run(antiring=0.3, pq=True, peak_nits=PEAK), A.scale(_unscaled(proc, t, 1), 97, 131, 77))
    assert len(proc._ycc_scratch) == n
    for bad in (True, "0.3", None, float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError):
            run(antiring=bad)


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, dh, dw = 12, 20, 30, 44
    t = torch.rand((3, h, w), device="cuda")
    dst = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device="cuda")
    fn, ctx, st, i, o = proc._lib.hdrtv_post_rgb48_scaled_ex, proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    bad = [
        (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, -1), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 257),
        (ctx, st, i, L.F32, h, w, 1, PEAK, o, dh, dw, -1), (ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 257),
    ]
    for ar in (0, 77):                  # the refusals of the plain entry point, off and on
        bad += [
            (None, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, ar), (ctx, st, None, L.F32, h, w, 0, 0.0, o, dh, dw, ar),
            (ctx, st, i, L.F32, h, w, 0, 0.0, None, dh, dw, ar),
            (ctx, st, i, L.F32, 0, w, 0, 0.0, o, dh, dw, ar), (ctx, st, i, L.F32, h, 0, 0, 0.0, o, dh, dw, ar),
            (ctx, st, i, L.F32, -h, w, 0, 0.0, o, dh, dw, ar), (ctx, st, i, L.F32, h, -w, 0, 0.0, o, dh, dw, ar),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, 0, dw, ar), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, 0, ar),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, -dh, dw, ar), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, -dw, ar),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, h - 1, dw, ar), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, w - 1, ar),
            (ctx, st, i, 2, h, w, 0, 0.0, o, dh, dw, ar), (ctx, st, i, -1, h, w, 0, 0.0, o, dh, dw, ar),
            (ctx, st, i, L.F32, h, w, 1, 0.0, o, dh, dw, ar), (ctx, st, i, L.F32, h, w, 1, -100.0, o, dh, dw, ar),
        ]
    for k, a in enumerate(bad):
        assert fn(*a) == L.EINVAL, k
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    assert fn(ctx, st, i, L.F32, h, w, 0, -5.0, o, dh, dw, 77) == L.OK      # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), A.scale(_unscaled(proc, t, 0), dh, dw, 77))


def test_enqueue_frame_and_everything_behind_the_scaler_see_the_antiringed_codes(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 150, 250
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(W.synthetic_frame(h, w, seed=77, kind="noise")).cuda()
        st = torch.cuda.current_stream()
        sp = p._stream()
        new = lambda fmt, hh, ww: torch.full(L.output_format(fmt, "left", hh, ww).shape, 0xA5A5, dtype=torch.uint16, device="cuda")   # noqa: E731
        run = lambda dst, **kw: p.enqueue_frame(0, dev.data_ptr(), h, w, dst.data_ptr(), stream=st, **kw)                           # noqa: E731
        small, big, off, auto, same = new("rgb48le", h, w), new("rgb48le", oh, ow), new("rgb48le", oh, ow), new("rgb48le", oh, ow), new("rgb48le", h, w)
        run(small)
        run(off, out_hw=(oh, ow))
        run(big, out_hw=(oh, ow), antiring=0.22)
        run(auto, out_hw=(oh, ow), antiring="auto")
        run(same, antiring=0.22)                                    # nothing is enlarged: the unscaled frame, not anti-ringed
        torch.cuda.synchronize()
        codes = small.cpu().numpy()
        assert np.array_equal(off.cpu().numpy(), A.scale(codes, oh, ow, 0))
        assert np.array_equal(big.cpu().numpy(), A.scale(codes, oh, ow, 56))
        assert np.array_equal(auto.cpu().numpy(), A.scale(codes, oh, ow, 77))               # 96 x 64: the schedule's 0.30
        assert np.array_equal(same.cpu().numpy(), codes)
        assert not np.array_equal(big.cpu().numpy(), off.cpu().numpy())                     # the frame rings
        assert len(p._ycc_scratch) == 0                                                     # rgb48le needs no scratch
        # a scaled yuv420p10le frame = the conversion from codes of the anti-ringed frame; its record = the statistic of those codes
        ycc, want_ycc = new("yuv420p10le", oh, ow), new("yuv420p10le", oh, ow)
        rec, want_rec = (torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") for _ in range(2))
        run(ycc, out_hw=(oh, ow), out_pix_fmt="yuv420p10le", antiring=0.22, light_ptr=rec.data_ptr())
        fmt = L.output_format("yuv420p10le", "left", oh, ow)
        p._chk(p._lib.hdrtv_rgb48_to_ycbcr10(p._ctx, sp, big.data_ptr(), oh, ow, *fmt.planes(want_ycc.data_ptr())), "rgb48_to_ycbcr10")
        p._chk(p._lib.hdrtv_rgb48_light_stats(p._ctx, sp, big.data_ptr(), oh, ow, 0, 0, ow, oh, want_rec.data_ptr()), "rgb48_light_stats")
        rec2 = torch.zeros_like(rec)
        run(off, out_hw=(oh, ow), antiring=0.22, light_ptr=rec2.data_ptr())                 # the record of an rgb48le frame too
        torch.cuda.synchronize()
        assert np.array_equal(ycc.cpu().numpy(), want_ycc.cpu().numpy())
        assert np.array_equal(rec.cpu().numpy(), want_rec.cpu().numpy()) and np.array_equal(rec2.cpu().numpy(), want_rec.cpu().numpy())
        assert np.array_equal(off.cpu().numpy(), big.cpu().numpy())
        # the 4:2:0 input path carries the strength too
        yuv = torch.from_numpy(np.random.default_rng(3).integers(16, 236, (h * 3 // 2, w)).astype(np.uint8)).cuda()
        ysmall, ybig = new("rgb48le", h, w), new("rgb48le", oh, ow)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ysmall.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ybig.data_ptr(), stream=st, out_hw=(oh, ow), antiring=1.0)
        torch.cuda.synchronize()
        assert np.array_equal(ybig.cpu().numpy(), A.scale(ysmall.cpu().numpy(), oh, ow, 256))
        for bad in (True, "0.3", None, -0.1, 1.5):
            with pytest.raises(ValueError):
                run(big, out_hw=(oh, ow), antiring=bad)
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
        wk.close()
    return got


def test_worker_resolves_auto_from_the_sizes_of_each_frame(golden_dir, tmp_path):
    from hdrtv_mi355x import weights as W
    oh, ow = 150, 250
    frames = [W.synthetic_frame(64, 96, seed=60 + i, kind="noise") for i in range(2)]
    base = _run_worker(golden_dir, tmp_path, "plain", frames, buffer_frames=2, antiring="auto")      # nothing enlarged: not anti-ringed
    big = _run_worker(golden_dir, tmp_path, "auto", frames, buffer_frames=2, out_w=ow, out_h=oh, antiring="auto")
    fixed = _run_worker(golden_dir, tmp_path, "fixed", frames, buffer_frames=2, out_w=ow, out_h=oh, antiring=0.10)
    for i in range(2):
        assert base[i].shape == (64, 96, 3)
        assert np.array_equal(big[i], A.scale(base[i], oh, ow, 77)), i                                # 96 x 64 -> 0.30
        assert np.array_equal(fixed[i], A.scale(base[i], oh, ow, 26)), i
        assert not np.array_equal(big[i], A.scale(base[i], oh, ow, 0))


def test_dispatcher_workers_apply_the_strength(golden_dir):
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
        want.append(A.scale(u16.cpu().numpy(), oh, ow, 128))
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_height=oh, out_width=ow, antiring=0.5) as d:
        assert d.antiring == 0.5
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0]
    assert sorted(got) == [0, 1]
    for i in range(2):
        assert got[i].shape == (oh, ow, 3) and np.array_equal(got[i], want[i]), i
