"""hdrtv_post_rgb48_scaled_cas on a real MI355X: contrast-adaptive sharpening of the codes in front of the fused Lanczos upscale,
and the routes through postprocess_rgb48_scaled, enqueue_frame, the worker and the dispatcher that carry the strength.

The yardstick is always the composition: what the EXISTING unscaled entry point writes at the processing size (hdrtv_post_rgb48,
or hdrtv_post_pq_rgb48 for pq; pinned by the other GPU tests, so no quantiser is restated here), then tests/rgb48_cas_ref.sharpen,
then tests/rgb48_antiring_ref.scale (whose strength 0 is tests/rgb48_scale_ref.scale).  Equality is exact: every value of every
frame."""
import itertools
import os
import threading

import numpy as np
import pytest

import rgb48_antiring_ref as A
import rgb48_cas_ref as C
import ycbcr10_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
CODES = (4084, 3426, 1032)          # the weakest code lib.cas_code gives, the reference's 0.22, full strength
STRENGTHS = (0, 77, 256)            # plain passes, the reference's 0.30, full anti-ringing
PAIRS = list(itertools.product(CODES, STRENGTHS))
# source (H, W) -> destination (dH, dW).  The kernel's tile is 32 x 64 output pixels, its footprint at most 38 x 70 source pixels.
# Every geometry runs the full product frame x dtype x pq x K x a: 144 launches of a few microseconds each.
SHAPES = [
    ((36, 52), (72, 104)),        # exact 2x, several tiles
    ((5, 7), (97, 131)),          # a footprint smaller than the halo: both borders of both axes in one tile
    ((37, 53), (64, 127)),        # ragged ratios; odd dW: rows that are not 8-byte aligned, the store code by code
    ((33, 70), (34, 71)),         # a ratio next to 1: the largest footprint (70 columns), the halo at the limit of its storage
    ((40, 48), (40, 96)),         # one axis at identity: still sharpened on both
    ((40, 48), (80, 48)),
    ((1, 1), (3, 5)),             # everything clamps
]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _contents(h, w):
    rng = np.random.default_rng(1000 * h + w)
    yy = np.mgrid[0:h, 0:w][0]
    step = np.full((3, h, w), 0.25, np.float32)               # the 0.25 / 0.75 step: red and blue along x, green along y
    step[:, :, w // 2:] = 0.75
    step[1] = np.where(yy >= h // 2, 0.75, 0.25)
    border = rng.uniform(0.3, 0.7, (3, h, w)).astype(np.float32)      # the first and last two rows and columns alternate 0 / 65535
    if h >= 2:
        border[:, 0], border[:, -2], border[:, 1], border[:, -1] = 0.0, 0.0, 1.0, 1.0
    if w >= 2:
        border[:, :, 0], border[:, :, -2], border[:, :, 1], border[:, :, -1] = 0.0, 0.0, 1.0, 1.0
    return {
        "noise": rng.uniform(-0.02, 1.02, (3, h, w)).astype(np.float32),          # the full range of codes, both clamps a little
        "step": step,
        "border": border,
        "near white": rng.uniform(0.985, 1.0, (3, h, w)).astype(np.float32),      # 131070 - mx is the smaller term of q
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


def _call(p, name, t, pq, dh, dw, *codes):
    """A C entry point of the scaled family itself, with its trailing codes."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    p._chk(getattr(p._lib, name)(p._ctx, p._stream(), t.data_ptr(), dt, h, w, pq, PEAK, o.data_ptr(), dh, dw, *codes), name)
    return o.cpu().numpy()


def _cas(p, t, pq, dh, dw, a, k):
    return _call(p, "hdrtv_post_rgb48_scaled_cas", t, pq, dh, dw, a, k)


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_cas_equals_the_composition(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    ran = set()
    for name, x in _contents(h, w).items():
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(x).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                sharp = {}
                for k, a in PAIRS:
                    if k not in sharp:
                        sharp[k] = C.sharpen(codes, k)
                    want = A.scale(sharp[k], dh, dw, a)
                    got = _cas(proc, t, pq, dh, dw, a, k)
                    bad = got != want
                    print("%s %s pq=%d K=%d a=%d: %d of %d values differ, largest |difference| %d" % (
                        name, str(dtype), pq, k, a, int(bad.sum()), bad.size, int(np.abs(got.astype(int) - want.astype(int)).max())))
                    assert not bad.any(), (name, str(dtype), pq, k, a)
                    if name == "noise" and h > 1:                       # the content gives the rule something to do
                        assert not np.array_equal(sharp[k], codes) and not np.array_equal(got, A.scale(codes, dh, dw, a))
                    ran.add((k, a))
    assert ran == set(PAIRS)


def test_cas_0_is_scaled_ex_and_equal_sizes_are_the_unscaled_bytes(proc):
    import torch
    x = _contents(36, 52)["noise"]
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes = _unscaled(proc, t, pq)
            for a in STRENGTHS:
                assert np.array_equal(_cas(proc, t, pq, 97, 131, a, 0), _call(proc, "hdrtv_post_rgb48_scaled_ex", t, pq, 97, 131, a))
                for k in (0,) + CODES:
                    assert np.array_equal(_cas(proc, t, pq, 36, 52, a, k), codes)           # not sharpened: nothing is enlarged
            assert np.array_equal(_cas(proc, t, pq, 97, 131, 0, 0), _call(proc, "hdrtv_post_rgb48_scaled", t, pq, 97, 131))


def test_the_ends_of_the_code_range(proc):
    import torch
    t = torch.from_numpy(_contents(36, 52)["noise"]).cuda()
    codes = _unscaled(proc, t, 0)
    for k in (1033, 4095, 4096):
        assert np.array_equal(_cas(proc, t, 0, 64, 127, 26, k), C.scale(codes, 64, 127, k, 26)), k


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, dh, dw = 12, 20, 30, 44
    t = torch.rand((3, h, w), device="cuda")
    dst = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device="cuda")
    fn, ctx, st, i, o = proc._lib.hdrtv_post_rgb48_scaled_cas, proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    bad = [(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 0, k) for k in (-1, 1, 256, 1031, 4097, 65536, -3426)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 0, 1031), (ctx, st, i, L.F32, h, w, 1, PEAK, o, dh, dw, 77, 4097)]
    for k in (0, 3426):                 # the refusals of hdrtv_post_rgb48_scaled_ex, off and on
        bad += [
            (None, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 0, k), (ctx, st, None, L.F32, h, w, 0, 0.0, o, dh, dw, 0, k),
            (ctx, st, i, L.F32, h, w, 0, 0.0, None, dh, dw, 0, k), (ctx, st, i, L.F32, 0, w, 0, 0.0, o, dh, dw, 0, k),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, h - 1, dw, 0, k), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, w - 1, 0, k),
            (ctx, st, i, 2, h, w, 0, 0.0, o, dh, dw, 0, k), (ctx, st, i, L.F32, h, w, 1, 0.0, o, dh, dw, 0, k),
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, -1, k), (ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 257, k),
        ]
    for n, a in enumerate(bad):
        assert fn(*a) == L.EINVAL, n
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    assert fn(ctx, st, i, L.F32, h, w, 0, -5.0, o, dh, dw, 77, 3426) == L.OK      # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), C.scale(_unscaled(proc, t, 0), dh, dw, 3426, 77))


def test_python_surface_maps_the_strength(proc):
    import torch
    from hdrtv_mi355x import lib as L
    t = torch.from_numpy(_contents(36, 52)["noise"]).cuda()
    codes = _unscaled(proc, t, 0)
    run = lambda **kw: proc.postprocess_rgb48_scaled(t, 131, 97, **kw).cpu().numpy()      # noqa: E731
    n = len(proc._ycc_scratch)
    assert np.array_equal(run(cas=0.22), C.scale(codes, 97, 131, 3426))
    assert np.array_equal(run(), C.scale(codes, 97, 131, 0)) and np.array_equal(run(cas=0.0), run())
    assert np.array_equal(run(cas=1.0, antiring=0.3), C.scale(codes, 97, 131, 1032, 77))
    assert L.scale_cas(52, 36, 131, 97) == 0.22 and L.scale_antiring(52, 36, 131, 97) == 0.30
    assert np.array_equal(run(cas="auto", antiring="auto"), C.scale(codes, 97, 131, 3426, 77))
    assert np.array_equal(run(cas=0.16, pq=True, peak_nits=PEAK), C.scale(_unscaled(proc, t, 1), 97, 131, 3605))
    assert np.array_equal(proc.postprocess_rgb48_scaled(t, 52, 36, cas=0.22).cpu().numpy(), codes)      # equal sizes
    assert len(proc._ycc_scratch) == n
    for bad in (True, "0.2", None, float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError):
            run(cas=bad)


def test_enqueue_frame_and_everything_behind_the_scaler_see_the_sharpened_codes(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 150, 250
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(W.synthetic_frame(h, w, seed=77, kind="noise")).cuda()
        st = torch.cuda.current_stream()
        new = lambda fmt, hh, ww: torch.full(L.output_format(fmt, "left", hh, ww).shape, 0xA5A5, dtype=torch.uint16, device="cuda")   # noqa: E731
        run = lambda dst, **kw: p.enqueue_frame(0, dev.data_ptr(), h, w, dst.data_ptr(), stream=st, **kw)                           # noqa: E731
        small, off, on, auto, same = new("rgb48le", h, w), new("rgb48le", oh, ow), new("rgb48le", oh, ow), new("rgb48le", oh, ow), new("rgb48le", h, w)
        run(small)
        run(off, out_hw=(oh, ow))
        run(on, out_hw=(oh, ow), cas=0.16, antiring=0.22)
        run(auto, out_hw=(oh, ow), cas="auto")
        run(same, cas=0.22)                                         # nothing is enlarged: the unscaled frame, not sharpened
        torch.cuda.synchronize()
        codes = small.cpu().numpy()
        assert np.array_equal(off.cpu().numpy(), C.scale(codes, oh, ow, 0))
        assert np.array_equal(on.cpu().numpy(), C.scale(codes, oh, ow, 3605, 56))
        assert np.array_equal(auto.cpu().numpy(), C.scale(codes, oh, ow, 3426))             # 96 x 64: the schedule's 0.22
        assert np.array_equal(same.cpu().numpy(), codes)
        assert not np.array_equal(auto.cpu().numpy(), off.cpu().numpy())
        # a scaled yuv420p10le frame = the conversion of the sharpened, scaled codes; its record = the statistic of those codes
        ycc = new("yuv420p10le", oh, ow)
        rec, want_rec = (torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") for _ in range(2))
        run(ycc, out_hw=(oh, ow), out_pix_fmt="yuv420p10le", cas="auto", light_ptr=rec.data_ptr())
        p._chk(p._lib.hdrtv_rgb48_light_stats(p._ctx, p._stream(), auto.data_ptr(), oh, ow, 0, 0, ow, oh, want_rec.data_ptr()), "rgb48_light_stats")
        torch.cuda.synchronize()
        assert np.array_equal(ycc.cpu().numpy().reshape(-1), R.pack(auto.cpu().numpy(), "yuv420p10le", "left").reshape(-1))
        assert np.array_equal(rec.cpu().numpy(), want_rec.cpu().numpy())
        # the 4:2:0 input path carries the strength too
        yuv = torch.from_numpy(np.random.default_rng(3).integers(16, 236, (h * 3 // 2, w)).astype(np.uint8)).cuda()
        ysmall, ybig = new("rgb48le", h, w), new("rgb48le", oh, ow)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ysmall.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, ybig.data_ptr(), stream=st, out_hw=(oh, ow), cas=1.0)
        torch.cuda.synchronize()
        assert np.array_equal(ybig.cpu().numpy(), C.scale(ysmall.cpu().numpy(), oh, ow, 1032))
        for bad in (True, "0.2", None, -0.1, 1.5):
            with pytest.raises(ValueError):
                run(on, out_hw=(oh, ow), cas=bad)
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


def test_worker_sharpens_a_scaled_p010_frame_by_the_schedule(golden_dir, tmp_path):
    from hdrtv_mi355x import weights as W
    oh, ow = 150, 250
    frames = [W.synthetic_frame(64, 96, seed=60 + i, kind="noise") for i in range(2)]
    base = _run_worker(golden_dir, tmp_path, "plain", frames, cas="auto")                     # nothing enlarged: not sharpened
    soft = _run_worker(golden_dir, tmp_path, "soft", frames, out_w=ow, out_h=oh, out_pix_fmt="p010le")
    sharp = _run_worker(golden_dir, tmp_path, "sharp", frames, out_w=ow, out_h=oh, out_pix_fmt="p010le", cas="auto")
    for i in range(2):
        assert base[i].shape == (64, 96, 3)
        assert np.array_equal(soft[i].reshape(-1), R.pack(C.scale(base[i], oh, ow, 0), "p010le", "left").reshape(-1)), i
        assert np.array_equal(sharp[i].reshape(-1), R.pack(C.scale(base[i], oh, ow, 3426), "p010le", "left").reshape(-1)), i      # 96 x 64 -> 0.22
        assert not np.array_equal(sharp[i], soft[i])


def test_dispatcher_workers_apply_the_strength(golden_dir):
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
    want = C.scale(u16.cpu().numpy(), oh, ow, 2564, 26)
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_height=oh, out_width=ow, cas=0.5, antiring=0.1) as d:
        assert d.cas == 0.5
        d.submit(frame)
        d.flush(timeout=120)
    assert d.exit_codes == [0] and sorted(got) == [0]
    assert got[0].shape == (oh, ow, 3) and np.array_equal(got[0], want)
