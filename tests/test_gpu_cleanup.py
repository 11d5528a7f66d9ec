"""Output cleanup on a real MI355X: hdrtv_rgb48_deband, the dithered conversions hdrtv_post_ycbcr10_ex / hdrtv_rgb48_to_ycbcr10_ex, and
the routes through enqueue_frame, the worker and the dispatcher that carry them.

The yardstick is always tests/cleanup_ref (and tests/lightlevel_ref for the record) applied to the RGB48 codes the EXISTING entry
points write -- those are pinned by the other GPU tests, so no quantiser is restated here.  Equality is exact: every u16."""
import os
import threading

import numpy as np
import pytest

import cleanup_ref as K
import lightlevel_ref as LR
import ycbcr10_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
COMBOS = [("p010le", "left"), ("p010le", "topleft"), ("yuv420p10le", "left"), ("yuv420p10le", "topleft"), ("yuv422p10le", "left")]
# The deband kernel's tile is 32 x 128 pixels with a reach of 16.  The four small frames are smaller than the reach (all four clamps
# at once, odd sizes); 34 x 262 and 70 x 130 put two / six rows and six / two columns beyond one or two whole tiles in each axis.
DEBAND_SHAPES = [(1, 1), (2, 2), (5, 7), (6, 10), (34, 262), (70, 130)]
DEBAND_PARAMS = [(r, t, s) for r in (1, 16) for t in (1311, 1, 65535) for s in (0, 7)]
# The conversions' tile is 16 x 128 luma pixels, a lane's group eight: one group, a ragged group, a tile plus a ragged group, ragged
# tiles on both axes
DITHER_SHAPES = [(2, 2), (6, 10), (18, 136), (34, 262)]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


# ------------------------------------------------------------------------------------------------------------------ deband
def _smooth(h, w):
    """Steps of 514 codes every 16 columns / 12 rows, per-channel offsets and noise of +-400: both branches of the rule are taken."""
    y, x = np.mgrid[0:h, 0:w]
    base = 20000 + (x // 16 + y // 12) * 514
    noise = np.random.default_rng(100 * h + w).integers(-400, 401, (h, w, 3))
    return (base[..., None] + np.array([0, 300, -200]) + noise).astype(np.uint16)


def _edges(h, w):
    """Hard edges: 5 x 7 blocks of three far-apart levels (and the extreme codes) with +-100 of noise."""
    rng = np.random.default_rng(7 * h + w)
    levels = np.array([0, 5000, 30000, 60000, 65535])
    by, bx = -(-h // 5), -(-w // 7)
    blocks = levels[rng.integers(0, 5, (by, bx, 3))]
    f = np.repeat(np.repeat(blocks, 5, axis=0), 7, axis=1)[:h, :w]
    return np.clip(f + rng.integers(-100, 101, (h, w, 3)), 0, 65535).astype(np.uint16)


def _deband_raw(p, src_np, rng, thr, seed, offset):
    """hdrtv_rgb48_deband between buffers of 0xA5A5 whose frames start ``offset`` u16 elements in -> (result, source after the call,
    the destination's guard elements)."""
    import torch
    h, w = src_np.shape[:2]
    n = h * w * 3
    host = np.full(offset + n + 8, 0xA5A5, np.uint16)
    host[offset:offset + n] = src_np.reshape(-1)
    sbuf = torch.from_numpy(host).cuda()
    dbuf = torch.full((offset + n + 8,), 0xA5A5, dtype=torch.uint16, device="cuda")
    p._chk(p._lib.hdrtv_rgb48_deband(p._ctx, p._stream(), sbuf.data_ptr() + 2 * offset, h, w, rng, thr, seed, dbuf.data_ptr() + 2 * offset),
           "rgb48_deband")
    d, s = dbuf.cpu().numpy(), sbuf.cpu().numpy()
    return d[offset:offset + n].reshape(h, w, 3), s[offset:offset + n].reshape(h, w, 3), np.concatenate([d[:offset], d[offset + n:]])


@pytest.mark.parametrize("shape", DEBAND_SHAPES, ids=lambda v: "%dx%d" % v)
def test_deband_equals_the_rule(proc, shape):
    h, w = shape
    for kind, frame in (("smooth", _smooth(h, w)), ("edges", _edges(h, w))):
        for rng, thr, seed in DEBAND_PARAMS:
            want = K.deband(frame, rng, thr, seed)
            changed = float((want != frame).any(axis=2).mean())
            if kind == "smooth" and h * w > 1000 and (rng, thr) == (16, 1311):
                print("%dx%d seed %d: the rule changes %.1f %% of the pixels" % (h, w, seed, 100 * changed))
                assert 0.20 <= changed <= 0.80, changed              # neither branch can hide
            for offset in (0, 1):                                   # 1: no 16-byte access applies to either buffer
                got, src_after, guard = _deband_raw(proc, frame, rng, thr, seed, offset)
                tag = (kind, rng, thr, seed, offset)
                assert np.array_equal(got, want), tag + (int((got != want).sum()),)
                assert np.array_equal(src_after, frame), tag
                assert (guard == 0xA5A5).all(), tag


def test_postprocess_deband_returns_a_new_tensor_and_keeps_the_source(proc):
    import torch
    frame = _smooth(70, 130)
    src = torch.from_numpy(frame).cuda()
    out = proc.postprocess_deband(src)
    assert out.data_ptr() != src.data_ptr() and out.shape == src.shape and out.dtype == torch.uint16
    assert np.array_equal(out.cpu().numpy(), K.deband(frame)) and np.array_equal(src.cpu().numpy(), frame)
    out = proc.postprocess_deband(src, deband_range=3, deband_threshold=700, seed=0xFFFFFFFF)
    assert np.array_equal(out.cpu().numpy(), K.deband(frame, 3, 700, 0xFFFFFFFF))
    noise = np.random.default_rng(1).integers(0, 65536, (64, 96, 3)).astype(np.uint16)
    assert np.array_equal(proc.postprocess_deband(torch.from_numpy(noise).cuda()).cpu().numpy(), noise)
    for bad in (dict(deband_range=0), dict(deband_range=17), dict(deband_threshold=0), dict(deband_threshold=65536), dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError):
            proc.postprocess_deband(src, **bad)
    for bad in (torch.zeros((4, 4, 3), dtype=torch.int32, device="cuda"), src[..., :2], src.cpu(), src[0]):
        with pytest.raises(ValueError):
            proc.postprocess_deband(bad)


def test_deband_refusals_leave_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 12, 20
    n = h * w * 3
    src = torch.from_numpy(_smooth(h, w)).cuda()
    dst = torch.full((2 * n,), 0xA5A5, dtype=torch.uint16, device="cuda")
    f, ctx, st, s, d = proc._lib.hdrtv_rgb48_deband, proc._ctx, proc._stream(), src.data_ptr(), dst.data_ptr()
    bad = [(s, h, w, 0, 1311, d), (s, h, w, 17, 1311, d), (s, h, w, -1, 1311, d), (s, h, w, 16, 0, d), (s, h, w, 16, 65536, d),
           (s, h, w, 16, -7, d), (s, 0, w, 16, 1311, d), (s, h, 0, 16, 1311, d), (s, -h, w, 16, 1311, d), (None, h, w, 16, 1311, d),
           (s, h, w, 16, 1311, None),
           (d, h, w, 16, 1311, d),                                  # in place
           (d, h, w, 16, 1311, d + 2), (d + 2, h, w, 16, 1311, d),  # overlapping by all but one element
           (d, h, w, 16, 1311, d + 2 * n - 2), (d + 2 * n - 2, h, w, 16, 1311, d)]      # overlapping by one element
    for k, (a, hh, ww, r, t, b) in enumerate(bad):
        assert f(ctx, st, a, hh, ww, r, t, 0, b) == L.EINVAL, k
    assert f(None, st, s, h, w, 16, 1311, 0, d) == L.EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    two = torch.from_numpy(np.concatenate([src.cpu().numpy().reshape(-1), np.full(n, 0xA5A5, np.uint16)])).cuda()
    assert f(ctx, st, two.data_ptr(), h, w, 16, 1311, 0, two.data_ptr() + 2 * n) == L.OK      # adjacent buffers do not overlap
    torch.cuda.synchronize()
    assert np.array_equal(two.cpu().numpy()[n:].reshape(h, w, 3), K.deband(src.cpu().numpy()))


# ------------------------------------------------------------------------------------------------------------------ dither
def _input(h, w):
    """Seeded values in [-0.25, 1.25] (both clamps of the quantiser act), with exact 0 and 1 among them."""
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


def _contiguous(p, t, codes_dev, fmt, siting, pq, dither, ex, use_codes):
    """One conversion into a contiguous frame of 0xA5A5 through the ``_ex`` (``ex``) or the existing entry point."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    dst = torch.full((L.out_frame_bytes(fmt, h, w) // 2,), 0xA5A5, dtype=torch.uint16, device="cuda")
    planes = L.ycbcr10_planes(dst.data_ptr(), h, w, fmt, siting)
    tail = (dither,) if ex else ()
    lib, ctx, st = p._lib, p._ctx, p._stream()
    if use_codes:
        fn = lib.hdrtv_rgb48_to_ycbcr10_ex if ex else lib.hdrtv_rgb48_to_ycbcr10
        p._chk(fn(ctx, st, codes_dev.data_ptr(), h, w, *planes, *tail), "rgb48_to_ycbcr10")
    else:
        fn = lib.hdrtv_post_ycbcr10_ex if ex else lib.hdrtv_post_ycbcr10
        p._chk(fn(ctx, st, t.data_ptr(), L.F32 if t.dtype == torch.float32 else L.F16, h, w, pq, PEAK, *planes, *tail), "post_ycbcr10")
    return dst.cpu().numpy()


@pytest.mark.parametrize("shape", DITHER_SHAPES, ids=lambda v: "%dx%d" % v)
def test_dithered_conversions_equal_the_rule_and_dither_0_the_existing_bytes(proc, shape):
    import torch
    h, w = shape
    x = _input(h, w)
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes_dev, codes = _codes(proc, t, pq)
            for fmt, siting in COMBOS:
                tag = (fmt, siting, str(dtype), pq)
                want = K.pack(codes, fmt, siting, 1)
                got = proc.postprocess_ycbcr10(t, fmt, siting, pq=bool(pq), peak_nits=PEAK, dither="ordered").cpu().numpy()
                assert np.array_equal(got, want), tag + (int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))
                got2 = _contiguous(proc, t, codes_dev, fmt, siting, pq, 1, True, True)
                assert np.array_equal(got2, want), tag + ("from codes", int((got2 != want).sum()))
                if fmt == "p010le":
                    assert not (got & 63).any()
                # dither = 0 through the _ex entry points: the existing entry points' bytes (and the undithered rule)
                plain = R.pack(codes, fmt, siting)
                for use_codes in (False, True):
                    a = _contiguous(proc, t, codes_dev, fmt, siting, pq, 0, True, use_codes)
                    b = _contiguous(proc, t, codes_dev, fmt, siting, pq, 0, False, use_codes)
                    assert np.array_equal(a, b) and np.array_equal(a, plain), tag + (use_codes,)
                if h * w > 4:                                     # a 2 x 2 frame can dither to the rounded value
                    assert not np.array_equal(want, plain), tag


@pytest.mark.parametrize("shape", [(18, 136), (34, 262)], ids=lambda v: "%dx%d" % v)
def test_dithered_pitched_unaligned_planes_match_and_padding_stays(proc, shape):
    """y_pitch = 2 W + 2, a chroma pitch 6 bytes over its minimum, every plane base 2 bytes into its buffer."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = shape
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(_input(h, w)).to("cuda", dtype).contiguous()
        codes_dev, codes = _codes(proc, t, 0)
        for fmt, siting in COMBOS:
            y, cb, cr = K.planes(codes, fmt, siting, 1)
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
                        None if bv is None else bv.data_ptr() + 2, 2 * cp, L.DITHER_ORDERED)
                if use_codes:
                    proc._chk(proc._lib.hdrtv_rgb48_to_ycbcr10_ex(proc._ctx, proc._stream(), codes_dev.data_ptr(), h, w, *tail), "rgb48_to_ycbcr10_ex")
                else:
                    proc._chk(proc._lib.hdrtv_post_ycbcr10_ex(proc._ctx, proc._stream(), t.data_ptr(),
                                                              L.F32 if dtype == torch.float32 else L.F16, h, w, 0, 0.0, *tail), "post_ycbcr10_ex")
                bufs = [(by, h, w, yp), (bu, ch, cw, cp)] + ([] if bv is None else [(bv, ch, cw, cp)])
                for (buf, rows, n, pitch), want in zip(bufs, want_planes):
                    buf = buf.cpu().numpy()
                    expect = np.full(buf.shape, 0xA5A5, np.uint16)
                    for r in range(rows):
                        expect[1 + r * pitch: 1 + r * pitch + n] = want[r]
                    assert np.array_equal(buf, expect), (fmt, siting, str(dtype), use_codes, int((buf != expect).sum()))


def test_ex_entry_points_refuse_a_bad_dither_and_what_the_plain_ones_refuse(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 12, 20
    t = torch.rand((3, h, w), device="cuda")
    codes_dev, _ = _codes(proc, t, 0)
    dst = torch.full((h * w * 4,), 0xA5A5, dtype=torch.uint16, device="cuda")
    ctx, st, i, o = proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    u, v = o + 2 * h * w, o + 2 * h * w + h * w // 2
    ok = (L.YCC_YUV420P10, L.SITING_LEFT, o, 2 * w, u, v, w)
    f1, f2 = proc._lib.hdrtv_post_ycbcr10_ex, proc._lib.hdrtv_rgb48_to_ycbcr10_ex
    for dither in (2, -1, 255):
        assert f1(ctx, st, i, L.F32, h, w, 0, 0.0, *ok, dither) == L.EINVAL and f2(ctx, st, codes_dev.data_ptr(), h, w, *ok, dither) == L.EINVAL
    for dither in (0, 1):
        for a in ((h, w - 1) + ok, (h - 1, w) + ok, (h, w, 3) + ok[1:], (h, w, L.YCC_YUV422P10, L.SITING_TOPLEFT) + ok[2:],
                  (h, w, L.YCC_P010) + ok[1:], (h, w) + ok[:3] + (2 * w - 2,) + ok[4:], (h, w) + ok[:2] + (None,) + ok[3:]):
            assert f1(ctx, st, i, L.F32, a[0], a[1], 0, 0.0, *a[2:], dither) == L.EINVAL, a
            assert f2(ctx, st, codes_dev.data_ptr(), *a, dither) == L.EINVAL, a
        assert f1(ctx, st, i, 2, h, w, 0, 0.0, *ok, dither) == L.EINVAL and f1(ctx, st, i, L.F32, h, w, 1, 0.0, *ok, dither) == L.EINVAL
        assert f1(ctx, st, None, L.F32, h, w, 0, 0.0, *ok, dither) == L.EINVAL and f2(ctx, st, None, h, w, *ok, dither) == L.EINVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    with pytest.raises(ValueError):
        proc.postprocess_ycbcr10(t, "p010le", "left", dither="bayer")


# ------------------------------------------------------------------------------------------ end to end at 64 x 96
def _golden_frame(golden_dir):
    return np.load(os.path.join(golden_dir, "hr_64x96_noise_s0.npz"))["frame"]


def _gradient_frame():
    """A frame whose output has flat areas and gentle steps: with a threshold of 3000 the rule changes a third to a half of it."""
    from hdrtv_mi355x import weights as W
    return W.synthetic_frame(PH, PW, seed=71, kind="gradient")


def test_enqueue_frame_delivers_the_rules_of_its_cleanup(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    frame = _gradient_frame()
    h, w = frame.shape[:2]
    oh, ow = 2 * h, 2 * w
    both, deb, dit = L.output_cleanup(True, 12, 3000, "ordered"), L.output_cleanup(True, 9, 2500), L.output_cleanup(dither="ordered")
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(frame).cuda()
        st = torch.cuda.current_stream()
        new = lambda fmt, hh, ww: torch.full(L.output_format(fmt, "left", hh, ww).shape, 0xA5A5, dtype=torch.uint16, device="cuda")   # noqa: E731
        run = lambda dst, **kw: p.enqueue_frame(0, dev.data_ptr(), h, w, dst.data_ptr(), stream=st, **kw)                           # noqa: E731
        rgb, big = new("rgb48le", h, w), new("rgb48le", oh, ow)
        run(rgb)
        run(big, out_hw=(oh, ow))
        torch.cuda.synchronize()
        rgb_np, big_np = rgb.cpu().numpy(), big.cpu().numpy()
        assert len(p._ycc_scratch) == 0                           # nothing allocated so far
        cases = [("p010le", "left", None, both), ("p010le", "topleft", (oh, ow), both), ("rgb48le", "left", None, deb),
                 ("rgb48le", "left", (oh, ow), deb), ("yuv422p10le", "left", None, dit), ("yuv420p10le", "left", (oh, ow), dit),
                 ("yuv420p10le", "topleft", None, deb)]
        for fmt, siting, out_hw, c in cases:
            hh, ww = out_hw or (h, w)
            dst = new(fmt, hh, ww)
            rec = torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda")
            run(dst, out_hw=out_hw, out_pix_fmt=fmt, out_siting=siting, cleanup=c, light_ptr=rec.data_ptr())
            torch.cuda.synchronize()
            codes = big_np if out_hw else rgb_np
            want = K.cleanup(codes, fmt, siting, c.deband, c.deband_range, c.deband_threshold, c.dither_code)
            assert np.array_equal(dst.cpu().numpy(), want), (fmt, siting, out_hw, tuple(c))
            # the record describes the delivered RGB48 codes: debanded when deband is on, never dithered
            delivered = K.deband(codes, c.deband_range, c.deband_threshold) if c.deband else codes
            assert np.array_equal(rec.cpu().numpy(), LR.record(delivered)), (fmt, out_hw, tuple(c))
        for codes in (rgb_np, big_np):                            # the frame gives deband something to do
            share = float((K.deband(codes, 12, 3000) != codes).any(axis=2).mean())
            print("%dx%d: deband R = 12, T = 3000 changes %.1f %% of the pixels" % (codes.shape[1], codes.shape[0], 100 * share))
            assert share > 0.05
        # everything off: today's bytes, with None and with an inactive tuple
        for c in (None, L.output_cleanup()):
            a, b = new("rgb48le", h, w), new("p010le", h, w)
            run(a, cleanup=c)
            run(b, out_pix_fmt="p010le", cleanup=c)
            torch.cuda.synchronize()
            assert np.array_equal(a.cpu().numpy(), rgb_np) and np.array_equal(b.cpu().numpy(), R.pack(rgb_np, "p010le", "left"))
        # the 4:2:0 input path carries the cleanup too
        yuv = torch.full((h * 3 // 2, w), 128, dtype=torch.uint8, device="cuda")
        yrgb, yp = new("rgb48le", h, w), new("p010le", h, w)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, yrgb.data_ptr(), stream=st)
        p.enqueue_frame_yuv420(0, yuv.data_ptr(), h, w, yp.data_ptr(), stream=st, out_pix_fmt="p010le", cleanup=both)
        torch.cuda.synchronize()
        assert np.array_equal(yp.cpu().numpy(), K.cleanup(yrgb.cpu().numpy(), "p010le", "left", True, 12, 3000, 1))
        for bad in (dict(cleanup=dit), dict(cleanup=(True, 16, 1311, "none")), dict(out_pix_fmt="p010le", cleanup=L.OutputCleanup(True, 17, 1311, "none"))):
            with pytest.raises(ValueError):
                run(rgb, **bad)
    finally:
        p.close()


N = 2
PW, PH = 96, 64


@pytest.fixture(scope="module")
def weights_dir(golden_dir, tmp_path_factory):
    root = tmp_path_factory.mktemp("cleanup_weights")
    (root / "original").mkdir()
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), root / "original" / "HR.hdrw")
    return str(root)


@pytest.fixture(scope="module")
def frames(golden_dir):
    return [_golden_frame(golden_dir), _gradient_frame()]


def _run_worker(weights_dir, frames, **kw):
    """The frames through a worker and a collecting sink -> (delivered frames, their .light)."""
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wk = HeadlessPipelineWorker(weights_dir, use_hg=False, proc_w=PW, proc_h=PH, **kw)
    assert wk._load_model("FP16") is True
    got, light, done = [], [], threading.Event()

    def sink(payload):
        light.append(payload.light)
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
    return got, light


def test_worker_delivers_the_rules_and_measures_the_debanded_codes(weights_dir, frames):
    base, _ = _run_worker(weights_dir, frames)
    big, _ = _run_worker(weights_dir, frames, out_w=2 * PW, out_h=2 * PH)
    got, light = _run_worker(weights_dir, frames, out_pix_fmt="p010le", deband=True, deband_threshold=3000, dither="ordered", light_stats=True)
    for i in range(N):
        assert base[i].shape == (PH, PW, 3)
        assert np.array_equal(got[i], K.cleanup(base[i], "p010le", "left", True, 16, 3000, 1)), i
        assert np.array_equal(light[i], LR.record(K.deband(base[i], 16, 3000))), i
    got, light = _run_worker(weights_dir, frames, deband=True, deband_range=5, deband_threshold=3000, light_stats=True)
    for i in range(N):
        want = K.deband(base[i], 5, 3000)
        assert np.array_equal(got[i], want) and np.array_equal(light[i], LR.record(want)), i
    got, _ = _run_worker(weights_dir, frames, out_pix_fmt="yuv420p10le", out_siting="topleft", out_w=2 * PW, out_h=2 * PH, deband=True,
                         dither="ordered")
    for i in range(N):
        assert np.array_equal(got[i], K.cleanup(big[i], "yuv420p10le", "topleft", True, dither=1)), i
    assert (K.deband(base[1], 16, 3000) != base[1]).any(axis=2).mean() > 0.05 and (K.deband(big[1]) != big[1]).any()
    # everything off, spelt out: today's bytes
    got, _ = _run_worker(weights_dir, frames, deband=False, dither="none")
    for i in range(N):
        assert np.array_equal(got[i], base[i]), i


def test_dispatcher_workers_apply_the_cleanup(golden_dir, frames):
    import torch
    from hdrtv_mi355x.dispatch import FrameDispatcher
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w = PH, PW
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    want = []
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    for f in frames:
        dev = torch.from_numpy(f).cuda()
        p.enqueue_frame(0, dev.data_ptr(), h, w, u16.data_ptr(), stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        want.append(K.cleanup(u16.cpu().numpy(), "p010le", "left", True, 12, 3000, 1))
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": False}
    with FrameDispatcher(1, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=2,
                         out_pix_fmt="p010le", deband=True, deband_range=12, deband_threshold=3000, dither="ordered") as d:
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0] and sorted(got) == [0, 1]
    for i in range(N):
        assert np.array_equal(got[i], want[i]), i
