"""The tone map on a real MI355X: hdrtv_rgb48_tonemap, the fused hdrtv_post_rgb48_tonemap, and the routes through the processor's
output stage, the worker and the dispatcher that carry the curve.

The yardstick is tests/tonemap_ref.apply -- the pixel rule of include/hdrtv_mi355x.h in NumPy, with ``lin`` read from the library's
host table and ``code`` from the oracle -- applied to what the EXISTING entry points and paths write (hdrtv_post_rgb48 /
hdrtv_post_pq_rgb48 and ``_post_out`` without a curve, pinned by the other GPU tests), at the place the tone map has in the chain:
behind scale, grain and deband, in front of the light level record and the conversion to Y'CbCr.  Equality is exact: every value of
every frame, no tolerance."""
import ctypes as C
import itertools
import os
import threading

import numpy as np
import pytest

import film_grain_ref as G
import lightlevel_ref as LL
import tonemap_ref as T
import ycbcr10_ref as Y

pytestmark = pytest.mark.gpu

F = np.float32
PEAK = 1000.0
FILL = 0xA5A5
# odd pitch: 16-byte aligned on one row in eight, code by code on the others; aligned: the packed path; one pixel; narrower than a vector
FRAME_SIZES = ((33, 47), (64, 128), (1, 1), (5, 7))


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def lin():
    return T.lin_table()


@pytest.fixture(scope="module")
def gains():
    """name -> (host float32[65536], device tensor): the three curves at 1000 -> 600 and 1000 -> 203, all ones, and a random table in
    [0, 1.5] whose products pass 1 and meet the clamp."""
    import torch
    from hdrtv_mi355x import tonemap as TM
    host = {"%s-%d" % (k, t): TM.tone_curve(k, float(t)).gain_table() for k in TM.KINDS for t in (600, 203)}
    host["ones"] = np.ones(65536, F)
    host["random"] = np.random.default_rng(42).uniform(0.0, 1.5, 65536).astype(F)
    return {k: (v, torch.from_numpy(v).cuda()) for k, v in host.items()}


def _dt(t):
    import torch
    from hdrtv_mi355x import lib as L
    return L.F32 if t.dtype == torch.float32 else L.F16


def _unscaled(p, t, pq):
    import torch
    h, w = t.shape[-2:]
    o = torch.empty((h, w, 3), dtype=torch.uint16, device=t.device)
    if pq:
        p._chk(p._lib.hdrtv_post_pq_rgb48(p._ctx, p._stream(), t.data_ptr(), _dt(t), h, w, PEAK, o.data_ptr()), "post_pq_rgb48")
    else:
        p._chk(p._lib.hdrtv_post_rgb48(p._ctx, p._stream(), t.data_ptr(), _dt(t), h, w, o.data_ptr()), "post_rgb48")
    return o.cpu().numpy()


def _tone_codes(p, codes, gain_dev, in_place=False):
    import torch
    src = torch.from_numpy(codes).cuda()
    dst = src if in_place else torch.full_like(src, FILL)
    h, w = codes.shape[:2]
    p._chk(p._lib.hdrtv_rgb48_tonemap(p._ctx, p._stream(), src.data_ptr(), h, w, gain_dev.data_ptr(), dst.data_ptr()), "rgb48_tonemap")
    out = dst.cpu().numpy()
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), codes)                            # the source is not touched
    return out


def _tone_fused(p, t, pq, gain_dev):
    import torch
    h, w = t.shape[-2:]
    o = torch.full((h, w, 3), FILL, dtype=torch.uint16, device=t.device)
    p._chk(p._lib.hdrtv_post_rgb48_tonemap(p._ctx, p._stream(), t.data_ptr(), _dt(t), h, w, pq, PEAK, gain_dev.data_ptr(), o.data_ptr()),
           "post_rgb48_tonemap")
    return o.cpu().numpy()


def _tensor(h, w):
    """Values below 0 and above 1 and a full ramp: every code, both clamps."""
    rng = np.random.default_rng(100 * h + w)
    x = rng.uniform(-0.05, 1.05, (3, h, w)).astype(F)
    ramp = np.linspace(0.0, 1.0, h * w, dtype=F).reshape(h, w)
    x[0, : h // 2] = ramp[: h // 2]
    x[1, h // 2:] = ramp[::-1][h // 2:]
    x[2, 0, : min(w, 4)] = (-1.0, 2.0, 0.0, 1.0)[: min(w, 4)]
    return x


@pytest.mark.parametrize("size", FRAME_SIZES, ids=lambda v: "%dx%d" % v)
def test_standalone_equals_the_rule(proc, lin, gains, size):
    h, w = size
    rng = np.random.default_rng(h)
    codes = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
    codes[0, 0], codes[-1, -1] = 0, 65535
    for name, (gain, dev) in gains.items():
        want = T.apply(codes, gain, lin)
        if name == "ones":
            assert np.array_equal(want, codes)                                     # a gain of 1.0f is the identity on every byte
        for in_place in (False, True):
            got = _tone_codes(proc, codes, dev, in_place)
            bad = got != want
            print("%dx%d %s in_place=%d: %d of %d values differ" % (h, w, name, in_place, int(bad.sum()), bad.size))
            assert not bad.any(), (name, in_place)


def test_every_gain_entry_is_read(proc, lin, gains):
    """256 x 256: pixel i has max channel i (in the channel i mod 3), the other two random and at or below it."""
    rng = np.random.default_rng(9)
    m = np.arange(65536, dtype=np.int64)
    px = (rng.random((65536, 3)) * (m[:, None] + 1)).astype(np.int64)
    px[m, m % 3] = m
    codes = px.astype(np.uint16).reshape(256, 256, 3)
    assert np.array_equal(codes.max(axis=2).reshape(-1), m)
    for name, (gain, dev) in gains.items():
        want = T.apply(codes, gain, lin)
        got = _tone_codes(proc, codes, dev)
        bad = got != want
        print("%s: %d of %d values differ" % (name, int(bad.sum()), bad.size))
        assert not bad.any(), name
        if name == "ones":
            assert np.array_equal(got, codes)
        if name == "random":
            assert (got == 65535).any() and (got[codes.max(axis=2) > 0] != codes[codes.max(axis=2) > 0]).any()      # the clamp at 1 is met


@pytest.mark.parametrize("size", FRAME_SIZES, ids=lambda v: "%dx%d" % v)
def test_fused_equals_the_twin_then_the_rule(proc, lin, gains, size):
    import torch
    h, w = size
    x = _tensor(h, w)
    for dtype, pq in itertools.product((torch.float32, torch.float16), (0, 1)):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        codes = _unscaled(proc, t, pq)
        if not pq and h * w > 1:
            assert codes.min() == 0 and codes.max() == 65535
        for name in ("spline-600", "bt.2390-203", "clip-600", "ones", "random"):
            gain, dev = gains[name]
            got = _tone_fused(proc, t, pq, dev)
            want = T.apply(codes, gain, lin)
            bad = got != want
            print("%dx%d %s pq=%d %s: %d of %d values differ" % (h, w, dtype, pq, name, int(bad.sum()), bad.size))
            assert not bad.any(), (str(dtype), pq, name)
            if name == "ones":
                assert np.array_equal(got, codes)                                  # the twin's bytes


def test_every_refused_call_leaves_dst_alone(proc, gains):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 12, 20
    t = torch.rand((3, h, w), device="cuda")
    src = torch.zeros((h, w, 3), dtype=torch.uint16, device="cuda")
    dst = torch.full((h, w, 3), FILL, dtype=torch.uint16, device="cuda")
    g = gains["spline-600"][1].data_ptr()
    lib, ctx, st, i, s, o = proc._lib, proc._ctx, proc._stream(), t.data_ptr(), src.data_ptr(), dst.data_ptr()
    bad = [lib.hdrtv_rgb48_tonemap(*a) for a in ((None, st, s, h, w, g, o), (ctx, st, None, h, w, g, o), (ctx, st, s, 0, w, g, o),
                                                 (ctx, st, s, h, 0, g, o), (ctx, st, s, -1, w, g, o), (ctx, st, s, h, w, None, o),
                                                 (ctx, st, s, h, w, g, None))]
    for a in ((None, st, i, L.F32, h, w, 0, 0.0, g, o), (ctx, st, None, L.F32, h, w, 0, 0.0, g, o), (ctx, st, i, L.F32, h, w, 0, 0.0, None, o),
              (ctx, st, i, L.F32, h, w, 0, 0.0, g, None), (ctx, st, i, L.F32, 0, w, 0, 0.0, g, o), (ctx, st, i, L.F32, h, -3, 0, 0.0, g, o),
              (ctx, st, i, 2, h, w, 0, 0.0, g, o), (ctx, st, i, L.F32, h, w, 1, 0.0, g, o), (ctx, st, i, L.F32, h, w, 1, float("nan"), g, o)):
        bad.append(lib.hdrtv_post_rgb48_tonemap(*a))
    assert len(bad) == 16 and all(rc == L.EINVAL for rc in bad), bad
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    assert lib.hdrtv_post_rgb48_tonemap(ctx, st, i, L.F32, h, w, 0, -5.0, g, o) == L.OK            # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), T.apply(_unscaled(proc, t, 0), gains["spline-600"][0]))


def _post_out(p, t, key, pix_fmt="rgb48le", out_hw=None, light=False, **kw):
    """``HDRTVNetMI355X._post_out`` of the tensor ``t`` -> (delivered frame, light level record or None)."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    oh, ow = out_hw or (h, w)
    out = L.output_format(pix_fmt, "left", oh, ow)
    dst = torch.full(out.shape, FILL, dtype=torch.uint16, device="cuda")
    rec = torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") if light else None
    grain = kw.get("film_grain", 0.0)
    plan = L.SCALE_OFF.plan(w, h, ow, oh, grain, kw.get("grain_seed", 0.0)) if grain else L.SCALE_OFF.plan(w, h, ow, oh)
    p._post_out(C.c_void_p(torch.cuda.current_stream().cuda_stream), t.data_ptr(), _dt(t), h, w, dst.data_ptr(), out, key,
                rec.data_ptr() if light else None, None, kw.pop("cleanup", None), plan, **kw)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), (rec.cpu().numpy() if light else None)


def test_post_out_places_the_tone_map(proc, lin):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import tonemap as TM
    h, w = 40, 72
    t = torch.from_numpy(_tensor(h, w)).to("cuda", torch.float16).contiguous()
    tone = L.tone_mapping("spline", 600)
    gain = tone.gain_table()
    top = int(np.floor(65535.0 * float(TM.pq_oetf(600.0)) + 0.5))             # the target peak's code
    n0 = len(proc._ycc_scratch)

    def check(tag, want_rgb, got, rec, fmt="rgb48le"):
        want = want_rgb if fmt == "rgb48le" else Y.pack(want_rgb, fmt, "left")
        assert np.array_equal(got.reshape(-1), want.reshape(-1)), tag
        assert np.array_equal(rec, LL.record(want_rgb)), tag                   # the record of the tone-mapped codes
        print(tag, "max_code", int(rec[4099]), "target peak's code", top)
        assert rec[4099] <= top + 1, tag

    # unscaled RGB48: the fused launch
    base, rec0 = _post_out(proc, t, "tm", light=True)
    assert rec0[4099] == 65535 and len(proc._ycc_scratch) == n0                # without a curve: the full range, and no scratch
    got, rec = _post_out(proc, t, "tm", light=True, tone=tone)
    check("unscaled", T.apply(base, gain, lin), got, rec)
    assert len(proc._ycc_scratch) == n0                                        # no new scratch
    # scaled, Lanczos 2x: in place on the scaled codes
    big, _ = _post_out(proc, t, "tm", out_hw=(2 * h, 2 * w))
    got, rec = _post_out(proc, t, "tm", out_hw=(2 * h, 2 * w), light=True, tone=tone)
    check("lanczos 2x", T.apply(big, gain, lin), got, rec)
    # P010 at the processing size: through the codes scratch, in front of the conversion
    got, rec = _post_out(proc, t, "tm", pix_fmt="p010le", light=True, tone=tone)
    check("p010", T.apply(base, gain, lin), got, rec, "p010le")
    plain, _ = _post_out(proc, t, "tm", pix_fmt="p010le")
    assert np.array_equal(plain.reshape(-1), Y.pack(base, "p010le", "left").reshape(-1))
    # grain on: behind the grain
    seed = L.film_grain_seed(1234, 5)
    grained, _ = _post_out(proc, t, "tm", film_grain=0.01, grain_seed=seed)
    assert np.array_equal(grained, G.apply(base, h, w, seed, 0.01))
    got, rec = _post_out(proc, t, "tm", light=True, film_grain=0.01, grain_seed=seed, tone=tone)
    check("grain", T.apply(grained, gain, lin), got, rec)
    # deband on: behind the deband, and scaled P010 with grain: everything at once
    cl = L.output_cleanup(deband=True)
    smooth, _ = _post_out(proc, t, "tm", cleanup=cl)
    got, rec = _post_out(proc, t, "tm", light=True, cleanup=cl, tone=tone)
    check("deband", T.apply(smooth, gain, lin), got, rec)
    both, _ = _post_out(proc, t, "tm", out_hw=(2 * h, 2 * w), film_grain=0.01, grain_seed=seed)
    got, rec = _post_out(proc, t, "tm", pix_fmt="yuv420p10le", out_hw=(2 * h, 2 * w), light=True, film_grain=0.01, grain_seed=seed, tone=tone)
    check("scaled grain yuv420p10le", T.apply(both, gain, lin), got, rec, "yuv420p10le")
    # another curve is another table; a curve that resolves to off is not a record
    got, rec = _post_out(proc, t, "tm", light=True, tone=L.tone_mapping("bt.2390", 203))
    assert np.array_equal(got, T.apply(base, L.tone_mapping("bt.2390", 203).gain_table(), lin))
    assert rec[4099] <= int(np.floor(65535.0 * float(TM.pq_oetf(203.0)) + 0.5)) + 1
    with pytest.raises(ValueError):
        _post_out(proc, t, "tm", tone=("spline", 600.0))


def test_python_surface_and_the_cache_bound(golden_dir, lin):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    try:
        codes = np.random.default_rng(3).integers(0, 65536, (33, 47, 3), dtype=np.uint16)
        dev = torch.from_numpy(codes).cuda()
        tone = L.tone_mapping("spline", 600)
        assert np.array_equal(p.postprocess_tonemap(dev, tone).cpu().numpy(), T.apply(codes, tone.gain_table(), lin))
        assert np.array_equal(p.postprocess_tonemap(dev, None).cpu().numpy(), codes) and np.array_equal(dev.cpu().numpy(), codes)
        assert len(p._tone_tables) == 1
        p.postprocess_tonemap(dev, L.tone_mapping("spline", 600.0))                # the same record: the same table
        assert len(p._tone_tables) == 1
        for bad in (codes, dev.float(), dev[:, :, :2]):
            with pytest.raises(ValueError):
                p.postprocess_tonemap(bad, tone)
        with pytest.raises(ValueError):
            p.postprocess_tonemap(dev, "spline")
        for i in range(1, p.TONE_TABLES_MAX):
            p._tone_gain(L.tone_mapping("clip", 100.0 + i))
        assert len(p._tone_tables) == p.TONE_TABLES_MAX == 16
        with pytest.raises(ValueError, match="16 tone curves"):
            p._tone_gain(L.tone_mapping("clip", 50.0))
        assert np.array_equal(p.postprocess_tonemap(dev, tone).cpu().numpy(), T.apply(codes, tone.gain_table(), lin))      # kept
    finally:
        p.close()


N, PW, PH = 2, 96, 64


@pytest.fixture(scope="module")
def frames():
    from hdrtv_mi355x import weights as W
    return [W.synthetic_frame(PH, PW, seed=70 + i, kind="noise" if i % 2 else "gradient") for i in range(N)]


def _worker_run(golden_dir, tmp_path, tag, frames, **kw):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / tag / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    wk = HeadlessPipelineWorker(str(tmp_path / tag), use_hg=False, proc_w=PW, proc_h=PH, **kw)
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
        assert done.wait(30.0)
    finally:
        wk._stop_hdr_feeder()
        wk.close()
    return got, light


@pytest.fixture(scope="module")
def plain(golden_dir, tmp_path_factory, frames):
    return _worker_run(golden_dir, tmp_path_factory.mktemp("tm"), "plain", frames)[0]


def test_worker_rolls_every_frame_off(golden_dir, tmp_path, frames, plain, lin):
    from hdrtv_mi355x import lib as L
    gain = L.tone_mapping("spline", 600).gain_table()
    got, light = _worker_run(golden_dir, tmp_path, "tone", frames, tone_mapping="spline", target_peak=600, light_stats=True)
    for i in range(N):
        want = T.apply(plain[i], gain, lin)
        assert got[i].shape == (PH, PW, 3) and np.array_equal(got[i], want) and not np.array_equal(got[i], plain[i]), i
        assert np.array_equal(light[i], LL.record(want)), i
    # off -- "none", or a target at the source peak -- is the worker built without the arguments, byte for byte
    for tag, kw in (("none", dict(tone_mapping="none")), ("same", dict(tone_mapping="spline", target_peak=1000.0))):
        off, _ = _worker_run(golden_dir, tmp_path, tag, frames[:1], **kw)
        assert np.array_equal(off[0], plain[0]), tag


def test_dispatcher_rolls_a_frame_off(golden_dir, frames, plain, lin):
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.dispatch import FrameDispatcher
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": False}
    with FrameDispatcher(1, PH, PW, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=3, tone_mapping="bt.2390",
                         target_peak=203) as d:
        assert d.tone == L.tone_mapping("bt.2390", 203)
        d.submit(frames[0])
        d.flush(timeout=120)
    assert d.exit_codes == [0] and sorted(got) == [0]
    assert np.array_equal(got[0], T.apply(plain[0], d.tone.gain_table(), lin))
