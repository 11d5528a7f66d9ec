"""8-bit 4:2:0 input (I420, NV12) on a real MI355X: hdrtv_yuv420_to_bgr_u8 against the rule (tests/yuv420_ref.py) bit for bit, at
any plane alignment and pitch; hdrtv_preprocess_yuv420 (pre_fused's YUV staging) against hdrtv_preprocess of the converted frame,
bit for bit, in both outputs, every condition mode, fp16 and fp32 contexts; the processor, playback and dispatcher surfaces
against their BGR forms; the argument rules on a real context."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import yuv420_ref as R

pytestmark = pytest.mark.gpu

LAYOUT = {"i420": 0, "nv12": 1}


def _proc(golden_dir, **kw):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    return HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=kw.pop("use_hg", False), warmup_passes=0, **kw)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Planes:
    """A 4:2:0 frame in one device buffer with the planes where a test puts them: luma at byte `off` with pitch `yp`, the chroma
    plane(s) after it at odd offsets with pitch `cp` (0: tight).  Bytes outside the planes hold noise that must not be read
    into the result."""

    def __init__(self, frame, layout, off=0, yp=0, cp=0, seed=0):
        import torch
        Y, U, V = R.split(frame, layout)
        h, w = Y.shape
        self.h, self.w, self.layout = h, w, LAYOUT[layout]
        self.yp = yp or w
        cw = w if layout == "nv12" else w // 2
        self.cp = cp or cw
        rng = np.random.default_rng(seed)
        yb = off + self.yp * h
        uoff = yb + (3 if off else 0)
        csz = self.cp * (h // 2)
        voff = uoff + csz + (1 if off else 0)
        n = voff + csz + 16
        host = rng.integers(0, 256, n, dtype=np.uint8)
        for r in range(h):
            host[off + r * self.yp: off + r * self.yp + w] = Y[r]
        if layout == "nv12":
            for r in range(h // 2):
                row = host[uoff + r * self.cp: uoff + r * self.cp + w]
                row[0::2], row[1::2] = U[r], V[r]
        else:
            for r in range(h // 2):
                host[uoff + r * self.cp: uoff + r * self.cp + w // 2] = U[r]
                host[voff + r * self.cp: voff + r * self.cp + w // 2] = V[r]
        self.buf = torch.from_numpy(host).cuda()
        base = self.buf.data_ptr()
        self.y, self.u = base + off, base + uoff
        self.v = None if layout == "nv12" else base + voff

    def args(self):
        return (self.y, self.yp, self.u, self.v, self.cp, self.layout)


def _to_bgr(p, planes, matrix=709, full=0, guard=0):
    """hdrtv_yuv420_to_bgr_u8 into a device buffer with `guard` canary bytes either side (destination at an odd address)."""
    import torch
    h, w = planes.h, planes.w
    n = h * w * 3
    dst = torch.full((n + 2 * guard + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    o = guard + 1 if guard else 0
    rc = p._lib.hdrtv_yuv420_to_bgr_u8(p._ctx, _stream(), *planes.args(), matrix, full, h, w, dst.data_ptr() + o)
    assert rc == 0, p._lib.hdrtv_last_error(p._ctx)
    host = dst.cpu().numpy()
    if guard:
        assert (host[:o] == 0xA5).all() and (host[o + n:] == 0xA5).all()
    return host[o:o + n].reshape(h, w, 3)


@pytest.fixture(scope="module")
def proc(golden_dir):
    p = _proc(golden_dir)
    yield p
    p.close()


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_device_conversion_every_matrix_and_range(proc, layout):
    f = R.random_frame(38, 54, seed=1, layout=layout)
    planes = Planes(f, layout)
    for m in (601, 709, 2020):
        for full in (0, 1):
            assert np.array_equal(_to_bgr(proc, planes, m, full), R.to_bgr(f, layout, m, bool(full))), (m, full)


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840)])
def test_device_conversion_full_size(proc, h, w):
    for layout in ("i420", "nv12"):
        f = R.random_frame(h, w, seed=h, layout=layout)
        assert np.array_equal(_to_bgr(proc, Planes(f, layout)), R.to_bgr(f, layout)), layout


@pytest.mark.parametrize("off", [1, 3])
def test_device_conversion_pitched_misaligned_planes_and_guard_bytes(proc, off):
    for layout, (h, w) in (("i420", (30, 46)), ("nv12", (30, 46)), ("i420", (64, 130))):
        f = R.random_frame(h, w, seed=off + w, layout=layout)
        planes = Planes(f, layout, off=off, yp=w + 5 + off, cp=(w if layout == "nv12" else w // 2) + 3 * off, seed=off)
        assert np.array_equal(_to_bgr(proc, planes, guard=64), R.to_bgr(f, layout)), (layout, h, w)


# The smallest frames the chroma walk of csrc/ycc_in.h can still go wrong at: Hc = 1 or Wc = 1 puts the j - 1, j + 1 and i + 1 clamps on
# the same sample.  The stand-alone converter needs no hdrtv_reserve (whose minimum is 8 x 8).
TINY = [(2, 2), (2, 6), (6, 2)]


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("h,w", TINY)
def test_device_conversion_smallest_frames(proc, h, w, layout):
    """Tight pitches; luma and chroma pitches padded by one dword; the plane bases offset by one sample (one byte); both."""
    f = R.random_frame(h, w, seed=10 * h + w, layout=layout)
    want = R.to_bgr(f, layout)
    cw = w if layout == "nv12" else w // 2
    for off, pad in ((0, 0), (0, 4), (1, 0), (1, 4)):
        planes = Planes(f, layout, off=off, yp=w + pad, cp=cw + pad, seed=off + pad)
        assert np.array_equal(_to_bgr(proc, planes, guard=16), want), (off, pad)


def _both(p, planes, h, w):
    """(fused YUV preprocess, BGR preprocess of the device-converted frame) as host arrays."""
    import torch
    dt = torch.float32 if p._fp32 else torch.float16
    rgb = [torch.empty((3, h, w), dtype=dt, device="cuda") for _ in range(2)]
    cond = [torch.empty((3, h // 4, w // 4), dtype=dt, device="cuda") for _ in range(2)]
    bgr = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    lib, ctx, st = p._lib, p._ctx, _stream()
    assert lib.hdrtv_reserve(ctx, h, w) == 0
    assert lib.hdrtv_preprocess_yuv420(ctx, st, *planes.args(), 709, 0, h, w, rgb[0].data_ptr(), cond[0].data_ptr()) == 0, \
        lib.hdrtv_last_error(ctx)
    assert lib.hdrtv_yuv420_to_bgr_u8(ctx, st, *planes.args(), 709, 0, h, w, bgr.data_ptr()) == 0
    assert lib.hdrtv_preprocess(ctx, st, bgr.data_ptr(), h, w, rgb[1].data_ptr(), cond[1].data_ptr()) == 0
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in rgb], [t.cpu().numpy() for t in cond]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32),
                                                 b.view(np.uint16 if b.dtype == np.float16 else np.uint32))


@pytest.mark.parametrize("h,w", [(68, 100), (132, 260), (1080, 1920), (2160, 3840)])
def test_fused_yuv_preprocess_equals_the_composition(proc, h, w):
    for mode in (0, 1, 2):
        assert proc._lib.hdrtv_set_cond_mode(proc._ctx, mode) == 0
        for layout in ("i420", "nv12"):
            f = R.random_frame(h, w, seed=7 * h + mode, layout=layout)
            off = 1 if layout == "nv12" else 3
            planes = Planes(f, layout, off=off, yp=w + 2 * off + 1, cp=(w if layout == "nv12" else w // 2) + off, seed=mode)
            (a, b), (ca, cb) = _both(proc, planes, h, w)
            assert _same_bits(a, b), (mode, layout)
            assert _same_bits(ca, cb), (mode, layout)
    assert proc._lib.hdrtv_set_cond_mode(proc._ctx, 0) == 0


def test_fused_yuv_preprocess_fp32_context(golden_dir):
    p = _proc(golden_dir, precision="fp32")
    try:
        for h, w in ((68, 100), (132, 260)):
            for mode in (0, 1, 2):
                assert p._lib.hdrtv_set_cond_mode(p._ctx, mode) == 0
                for layout in ("i420", "nv12"):
                    f = R.random_frame(h, w, seed=h + mode, layout=layout)
                    (a, b), (ca, cb) = _both(p, Planes(f, layout, off=1, yp=w + 3, cp=0), h, w)
                    assert a.dtype == np.float32 and _same_bits(a, b) and _same_bits(ca, cb), (h, w, mode, layout)
    finally:
        p.close()


def test_processor_surfaces_equal_their_bgr_forms(golden_dir):
    import torch
    p = _proc(golden_dir, lanes=2)
    try:
        h, w = 72, 128
        for layout, m, full in (("i420", 709, False), ("nv12", 601, True)):
            f = R.random_frame(h, w, seed=11, layout=layout)
            bgr = R.to_bgr(f, layout, m, full)
            kw = dict(layout=layout, matrix=m, full_range=full)
            t, c = p.preprocess_yuv420(f, **kw)
            t, c = t.clone(), c.clone()
            t2, c2 = p.preprocess(bgr)
            assert torch.equal(t, t2) and torch.equal(c, c2), layout
            # letterboxed: a 96x160 source onto the 72x128 canvas (INTER_AREA) and a 48x64 one (INTER_CUBIC)
            for sh, sw in ((96, 160), (48, 64)):
                g = R.random_frame(sh, sw, seed=sh, layout=layout)
                t, c = p.preprocess_yuv420_letterboxed(g, w, h, **kw)
                t, c = t.clone(), c.clone()
                t2, c2 = p.preprocess_letterboxed(R.to_bgr(g, layout, m, full), w, h)
                assert torch.equal(t, t2) and torch.equal(c, c2), (layout, sh, sw)
            out = p.process_yuv420(f, **kw).copy()
            assert np.array_equal(out, p.process(bgr)), layout
            # enqueue_frame_yuv420 on both lanes against enqueue_frame of the converted frame
            dev_yuv = torch.from_numpy(f).cuda()
            dev_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).cuda()
            for lane in (0, 1):
                o1 = torch.zeros((h, w, 3), dtype=torch.uint16, device="cuda")
                o2 = torch.ones((h, w, 3), dtype=torch.uint16, device="cuda")
                torch.cuda.synchronize()
                p.enqueue_frame_yuv420(lane, dev_yuv.data_ptr(), h, w, o1.data_ptr(), **kw)
                p.enqueue_frame(lane, dev_bgr.data_ptr(), h, w, o2.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(o1, o2), (layout, lane)
        with pytest.raises(ValueError):
            p.preprocess_yuv420(np.zeros((10, 8), np.uint8))               # 10 rows is not H*3//2 of an even H
        with pytest.raises(ValueError):
            p.preprocess_yuv420(R.random_frame(8, 8, 0), layout="yuy2")
    finally:
        p.close()


def test_staged_uploads_wait_for_the_previous_upload(golden_dir):
    """Two calls with different frames and no synchronisation between them: each returned tensor (cloned in stream order) equals
    the one the same call returns alone after a device synchronise, bit for bit -- for every host-fed path that stages a frame
    in a reused pinned slot (``HDRTVNetMI355X._upload``).  Without the wait for the previous upload the second memcpy may land in
    the slot before the first upload has read it, and both calls see the second frame.  At 64x96 the first copy is nearly always
    done by then, so on the code before the shared helper this test rarely failed: it pins the contract; the proof is the code,
    which has one upload routine with one wait."""
    import torch
    from hdrtv_mi355x import weights as W
    p = _proc(golden_dir)
    try:
        bgr = [W.synthetic_frame(64, 96, seed=70 + i, kind="noise") for i in range(2)]
        yuv = [R.random_frame(64, 96, seed=80 + i) for i in range(2)]
        calls = {"preprocess_letterboxed": [lambda f=f: p.preprocess_letterboxed(f, 128, 96) for f in bgr],
                 "preprocess_yuv420": [lambda f=f: p.preprocess_yuv420(f) for f in yuv],
                 "preprocess_yuv420_letterboxed": [lambda f=f: p.preprocess_yuv420_letterboxed(f, 128, 96) for f in yuv]}
        for name, pair in calls.items():
            alone = []
            for call in pair:
                torch.cuda.synchronize()
                alone.append([t.clone() for t in call()])
            torch.cuda.synchronize()
            assert not torch.equal(alone[0][0], alone[1][0]), name          # the two frames do differ
            back_to_back = [[t.clone() for t in call()] for call in pair]
            torch.cuda.synchronize()
            for k in range(2):
                for got, want in zip(back_to_back[k], alone[k]):
                    assert got.shape == want.shape and torch.equal(got, want), (name, k)
    finally:
        p.close()


def test_playback_yuv420p_clip_into_rgb48le_sink(golden_dir, tmp_path):
    """End to end: a yuv420p rawvideo clip -> prefetch -> worker (device conversion) -> rgb48le sink writes the bytes the bgr24
    path writes for the rule-converted clip."""
    from hdrtv_mi355x import playback as P
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / "weights" / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    h, w, n = 64, 96, 4
    frames = [R.random_frame(h, w, seed=60 + i) for i in range(n)]
    (tmp_path / "clip.yuv").write_bytes(b"".join(f.tobytes() for f in frames))
    (tmp_path / "clip.bgr").write_bytes(b"".join(R.to_bgr(f).tobytes() for f in frames))
    outs = []
    for path, fmt in (("clip.yuv", "yuv420p"), ("clip.bgr", "bgr24")):
        wk = HeadlessPipelineWorker(str(tmp_path / "weights"), use_hg=True, proc_w=w, proc_h=h, hg_weights="seeded:1234")
        assert wk._load_model("FP16")
        buf = io.BytesIO()
        sink = P.Rgb48leSink(buf, w, h, 30.0)
        wk._start_hdr_feeder(sink)
        feed = P.PinnedPrefetch(P.RawVideoSource(str(tmp_path / path), w, h, 30.0, pix_fmt=fmt))
        res = P.RealtimePlayback(wk, feed, sink=True, realtime=False).run()
        import time
        deadline = time.perf_counter() + 10.0
        while sink.frames < res["frames_processed"] and time.perf_counter() < deadline:
            time.sleep(0.01)
        wk._stop_hdr_feeder()
        feed.release()
        wk.close()
        assert res["frames_processed"] == n and sink.frames == n, fmt
        outs.append(buf.getvalue())
    assert len(outs[0]) == n * h * w * 6 and outs[0] == outs[1]


def test_dispatcher_yuv420p_on_the_device(golden_dir):
    import torch
    from hdrtv_mi355x.dispatch import FrameDispatcher
    h, w, n = 288, 512, 5
    frames = [R.random_frame(h, w, seed=300 + i) for i in range(n)]
    p = _proc(golden_dir, use_hg=True, hg_weights="seeded:1234")
    want = []
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    dev = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    for f in frames:
        dev.copy_(torch.from_numpy(R.to_bgr(f)))
        p.enqueue_frame(0, dev.data_ptr(), h, w, u16.data_ptr(), stream=torch.cuda.current_stream())
        want.append(u16.cpu().numpy().copy())
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(2, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0, 0], slots=2,
                         pix_fmt="yuv420p") as d:
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0, 0]
    assert sorted(got) == list(range(n))
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i


def test_argument_rules_on_a_real_context(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    p = _proc(golden_dir)
    try:
        lib, ctx, st = p._lib, p._ctx, _stream()
        h, w = 64, 96                                          # (hdrtv_reserve's smallest sizes are larger than 4:2:0 needs)
        b = torch.zeros(32768, dtype=torch.uint8, device="cuda")
        y, u, v, o = b.data_ptr(), b.data_ptr() + 6144, b.data_ptr() + 9216, b.data_ptr() + 12288
        out = torch.empty((3, h, w), dtype=torch.float16, device="cuda")
        cond = torch.empty((3, h // 4, w // 4), dtype=torch.float16, device="cuda")

        def conv(*a):
            return lib.hdrtv_yuv420_to_bgr_u8(ctx, st, *a, o)

        good = (y, w, u, v, w // 2, L.YUV_I420, 709, 0, h, w)
        assert conv(*good) == L.OK
        bad = [(None, w, u, v, w // 2, 0, 709, 0, h, w), (y, w, None, v, w // 2, 0, 709, 0, h, w), (y, w, u, None, w // 2, 0, 709, 0, h, w),
               (y, w, u, v, w // 2, 0, 709, 0, h + 1, w), (y, w, u, v, w // 2, 0, 709, 0, h, w - 1), (y, w - 1, u, v, w // 2, 0, 709, 0, h, w),
               (y, w, u, v, w // 2 - 1, 0, 709, 0, h, w), (y, w, u, None, w - 1, 1, 709, 0, h, w), (y, w, u, v, w, 1, 709, 0, h, w),
               (y, w, u, v, w // 2, 2, 709, 0, h, w), (y, w, u, v, w // 2, 0, 700, 0, h, w), (y, w, u, v, w // 2, 0, 709, 2, h, w)]
        for a in bad:
            assert conv(*a) == L.EINVAL, a
        assert lib.hdrtv_yuv420_to_bgr_u8(ctx, st, *good, None) == L.EINVAL
        # preprocess: the same rules, ESTATE before a reservation of this size, null outputs
        assert lib.hdrtv_preprocess_yuv420(ctx, st, *good, out.data_ptr(), cond.data_ptr()) == L.ESTATE
        assert lib.hdrtv_reserve(ctx, h, w) == L.OK
        assert lib.hdrtv_preprocess_yuv420(ctx, st, *good, out.data_ptr(), cond.data_ptr()) == L.OK
        assert lib.hdrtv_preprocess_yuv420(ctx, st, y, w, u, None, w, L.YUV_NV12, 2020, 1, h, w, out.data_ptr(), cond.data_ptr()) == L.OK
        for a in bad:
            assert lib.hdrtv_preprocess_yuv420(ctx, st, *a, out.data_ptr(), cond.data_ptr()) == L.EINVAL, a
        assert lib.hdrtv_preprocess_yuv420(ctx, st, *good, None, cond.data_ptr()) == L.EINVAL
        assert lib.hdrtv_preprocess_yuv420(ctx, st, *good, out.data_ptr(), None) == L.EINVAL
        torch.cuda.synchronize()
    finally:
        p.close()
