"""The film grain on a real MI355X: hdrtv_rgb48_film_grain, the three fused entry points hdrtv_post_rgb48_grain / _scaled_grain /
_fsr_grain, and the routes through the processor, the worker and the dispatcher that carry the intensity and the per-frame seed.

The yardstick is always a composition of references that exist: what the EXISTING entry points write (hdrtv_post_rgb48 /
hdrtv_post_pq_rgb48 at the processing size, pinned by the other GPU tests, so no quantiser is restated here), tests/rgb48_cas_ref,
tests/rgb48_antiring_ref (whose strength 0 is tests/rgb48_scale_ref) and tests/rgb48_fsr_ref, with tests/film_grain_ref.apply where
the reference's shader chain has the grain: on the processing-size codes (behind cas) in front of the Lanczos passes, behind EASU and
RCAS at the delivered size.  Equality is exact: every value of every frame, no tolerance."""
import itertools
import os
import threading

import numpy as np
import pytest

import film_grain_ref as G
import lightlevel_ref as LL
import rgb48_antiring_ref as A
import rgb48_cas_ref as C
import rgb48_fsr_ref as FSR
import ycbcr10_ref as Y

pytestmark = pytest.mark.gpu

F = np.float32
PEAK = 1000.0
SEEDS = (0.0, float(F(0.37)), float(np.nextafter(F(1), F(0))))      # ... the largest float32 below 1
INTENSITIES = (0.01, 0.1)
FRAME_SIZES = ((33, 47), (64, 128))          # odd pitch: the code-by-code path on every other row; aligned: the packed path
FILL = 0xA5A5


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


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


def _call(p, name, t, pq, dh, dw, *tail):
    """A C entry point of the scaled family, with what follows dH, dW."""
    import torch
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), FILL, dtype=torch.uint16, device=t.device)
    p._chk(getattr(p._lib, name)(p._ctx, p._stream(), t.data_ptr(), _dt(t), h, w, pq, PEAK, o.data_ptr(), dh, dw, *tail), name)
    return o.cpu().numpy()


def _grain_unscaled(p, t, pq, intensity, seed):
    import torch
    h, w = t.shape[-2:]
    o = torch.full((h, w, 3), FILL, dtype=torch.uint16, device=t.device)
    p._chk(p._lib.hdrtv_post_rgb48_grain(p._ctx, p._stream(), t.data_ptr(), _dt(t), h, w, pq, PEAK, o.data_ptr(), intensity, seed),
           "post_rgb48_grain")
    return o.cpu().numpy()


def _grain_codes(p, codes, intensity, seed, in_place=False):
    import torch
    src = torch.from_numpy(codes).cuda()
    dst = src if in_place else torch.full_like(src, FILL)
    h, w = codes.shape[:2]
    p._chk(p._lib.hdrtv_rgb48_film_grain(p._ctx, p._stream(), src.data_ptr(), h, w, intensity, seed, dst.data_ptr()), "rgb48_film_grain")
    out = dst.cpu().numpy()
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), codes)                            # the source is not touched
    return out


def _tensor(h, w):
    """Values below 0 and above 1 and a full ramp: every code, both clamps."""
    rng = np.random.default_rng(100 * h + w)
    x = rng.uniform(-0.05, 1.05, (3, h, w)).astype(F)
    ramp = np.linspace(0.0, 1.0, h * w, dtype=F).reshape(h, w)
    x[0, : h // 2] = ramp[: h // 2]
    x[1, h // 2:] = ramp[::-1][h // 2:]
    x[2, 0, :4] = (-1.0, 2.0, 0.0, 1.0)
    return x


def _border(h, w):
    """Strong content at all four borders: the first and last two rows and columns alternate 0 / 1, so a grain taken at a tap's own
    position outside the frame instead of the clamped pixel's would show."""
    rng = np.random.default_rng(7 * h + w)
    x = rng.uniform(0.3, 0.7, (3, h, w)).astype(F)
    x[:, 0], x[:, -2], x[:, 1], x[:, -1] = 0.0, 0.0, 1.0, 1.0
    x[:, :, 0], x[:, :, -2], x[:, :, 1], x[:, :, -1] = 0.0, 0.0, 1.0, 1.0
    return x


@pytest.mark.parametrize("size", FRAME_SIZES, ids=lambda v: "%dx%d" % v)
def test_standalone_equals_the_rule(proc, size):
    h, w = size
    rng = np.random.default_rng(h)
    codes = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
    codes[0, :3], codes[-1, -3:] = 0, 65535
    for seed, inten in itertools.product(SEEDS, INTENSITIES):
        want = G.apply(codes, h, w, seed, inten)
        assert not np.array_equal(want, codes)
        for in_place in (False, True):
            got = _grain_codes(proc, codes, inten, seed, in_place)
            bad = got != want
            print("%dx%d seed=%r I=%r in_place=%d: %d of %d values differ" % (h, w, seed, inten, in_place, int(bad.sum()), bad.size))
            assert not bad.any(), (seed, inten, in_place)
    if (h, w) == FRAME_SIZES[-1]:                         # every code once per channel: the kernel's s = c / 65535 has no division
        every = np.arange(65536, dtype=np.uint16).reshape(128, 512, 1).repeat(3, 2)
        every[:, :, 1], every[:, :, 2] = every[::-1, :, 1].copy(), every[:, ::-1, 2].copy()
        for inten in INTENSITIES:
            assert np.array_equal(_grain_codes(proc, every, inten, SEEDS[1]), G.apply(every, 128, 512, SEEDS[1], inten)), inten
    for v in (0, 65535):                                  # the clamp: all-black and all-white frames stay in range
        flat = np.full((h, w, 3), v, np.uint16)
        got = _grain_codes(proc, flat, 0.1, SEEDS[1])
        assert np.array_equal(got, G.apply(flat, h, w, SEEDS[1], 0.1)) and (got == v).any() and (got != v).any()


@pytest.mark.parametrize("size", FRAME_SIZES, ids=lambda v: "%dx%d" % v)
def test_unscaled_fused_equals_the_two_launch_route(proc, size):
    import torch
    h, w = size
    x = _tensor(h, w)
    for dtype, pq in itertools.product((torch.float32, torch.float16), (0, 1)):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        codes = _unscaled(proc, t, pq)
        if not pq:
            assert codes.min() == 0 and codes.max() == 65535
        for seed, inten in ((SEEDS[0], 0.01), (SEEDS[1], 0.1), (SEEDS[2], 0.01)):
            got = _grain_unscaled(proc, t, pq, inten, seed)
            want = G.apply(codes, h, w, seed, inten)
            bad = got != want
            print("%dx%d %s pq=%d seed=%r I=%r: %d of %d values differ" % (h, w, dtype, pq, seed, inten, int(bad.sum()), bad.size))
            assert not bad.any(), (str(dtype), pq, seed, inten)
            assert np.array_equal(got, _grain_codes(proc, codes, inten, seed))     # hdrtv_post_rgb48 + hdrtv_rgb48_film_grain


LANCZOS_SHAPES = [((45, 70), (67, 131)),      # several tiles, a ragged last tile, odd dW: rows that are not 8-byte aligned
                  ((40, 72), (80, 144))]      # exact 2x
LANCZOS_OPTS = ((0, 0), (77, 0), (0, 2048), (256, 1032))          # (antiring, cas)


@pytest.mark.parametrize("src,dst", LANCZOS_SHAPES, ids=lambda v: "%dx%d" % v)
def test_lanczos_chain_grains_the_processing_size_codes(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    seed, inten = SEEDS[1], 0.01
    for (name, x), dtype in itertools.product((("tensor", _tensor(h, w)), ("border", _border(h, w))), (torch.float32, torch.float16)):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes = _unscaled(proc, t, pq)
            grained = {}
            for a, k in LANCZOS_OPTS:
                if k not in grained:
                    grained[k] = G.apply(C.sharpen(codes, k) if k else codes, h, w, seed, inten)
                want = A.scale(grained[k], dh, dw, a)
                got = _call(proc, "hdrtv_post_rgb48_scaled_grain", t, pq, dh, dw, a, k, inten, seed)
                bad = got != want
                print("%s %s pq=%d a=%d K=%d: %d of %d values differ" % (name, dtype, pq, a, k, int(bad.sum()), bad.size))
                assert not bad.any(), (name, str(dtype), pq, a, k)
                assert not np.array_equal(got, _call(proc, "hdrtv_post_rgb48_scaled_cas", t, pq, dh, dw, a, k))        # the grain shows
    # another seed and the largest intensity, once
    t = torch.from_numpy(_border(h, w)).cuda()
    codes = _unscaled(proc, t, 0)
    got = _call(proc, "hdrtv_post_rgb48_scaled_grain", t, 0, dh, dw, 77, 3426, 0.1, SEEDS[2])
    assert np.array_equal(got, A.scale(G.apply(C.sharpen(codes, 3426), h, w, SEEDS[2], 0.1), dh, dw, 77))


@pytest.mark.parametrize("dst", [(80, 144), (61, 100)], ids=lambda v: "%dx%d" % v)
def test_fsr_grains_the_delivered_codes(proc, dst):
    import torch
    h, w = 40, 72
    dh, dw = dst
    x = _tensor(h, w)
    for dtype, pq, rcas in itertools.product((torch.float32, torch.float16), (0, 1), (0, 1)):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        plain = FSR.scale(_unscaled(proc, t, pq), dh, dw, 0.2 if rcas else None)
        twin = _call(proc, "hdrtv_post_rgb48_fsr", t, pq, dh, dw, rcas, 0.2)
        assert np.array_equal(twin, plain)
        for seed, inten in ((SEEDS[1], 0.01), (SEEDS[2], 0.1)):
            got = _call(proc, "hdrtv_post_rgb48_fsr_grain", t, pq, dh, dw, rcas, 0.2, inten, seed)
            want = G.apply(plain, dh, dw, seed, inten)
            bad = got != want
            print("%dx%d %s pq=%d rcas=%d seed=%r I=%r: %d of %d values differ" % (dh, dw, dtype, pq, rcas, seed, inten, int(bad.sum()), bad.size))
            assert not bad.any(), (str(dtype), pq, rcas, seed, inten)
            assert not np.array_equal(got, twin)


def test_off_means_off_and_equal_sizes_delegate(proc):
    import torch
    h, w, dh, dw = 40, 72, 61, 100
    x = _tensor(h, w)
    for dtype, pq in itertools.product((torch.float32, torch.float16), (0, 1)):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        codes = _unscaled(proc, t, pq)
        # intensity 0: the twin's bytes, whatever the seed
        assert np.array_equal(_grain_unscaled(proc, t, pq, 0.0, 0.5), codes)
        assert np.array_equal(_grain_codes(proc, codes, 0.0, 0.5), codes) and np.array_equal(_grain_codes(proc, codes, 0.0, 0.5, True), codes)
        for a, k in LANCZOS_OPTS:
            assert np.array_equal(_call(proc, "hdrtv_post_rgb48_scaled_grain", t, pq, dh, dw, a, k, 0.0, 0.5),
                                  _call(proc, "hdrtv_post_rgb48_scaled_cas", t, pq, dh, dw, a, k)), (a, k)
        for rcas in (0, 1):
            assert np.array_equal(_call(proc, "hdrtv_post_rgb48_fsr_grain", t, pq, dh, dw, rcas, 0.2, 0.0, 0.5),
                                  _call(proc, "hdrtv_post_rgb48_fsr", t, pq, dh, dw, rcas, 0.2)), rcas
        # equal sizes: hdrtv_post_rgb48_grain's bytes, whatever the scaler's options
        want = _grain_unscaled(proc, t, pq, 0.01, SEEDS[1])
        assert np.array_equal(want, G.apply(codes, h, w, SEEDS[1], 0.01))
        assert np.array_equal(_call(proc, "hdrtv_post_rgb48_scaled_grain", t, pq, h, w, 77, 3426, 0.01, SEEDS[1]), want)
        assert np.array_equal(_call(proc, "hdrtv_post_rgb48_fsr_grain", t, pq, h, w, 1, 0.2, 0.01, SEEDS[1]), want)


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, dh, dw = 12, 20, 22, 36
    t = torch.rand((3, h, w), device="cuda")
    src = torch.zeros((dh, dw, 3), dtype=torch.uint16, device="cuda")
    dst = torch.full((dh, dw, 3), FILL, dtype=torch.uint16, device="cuda")
    lib, ctx, st, i, s, o = proc._lib, proc._ctx, proc._stream(), t.data_ptr(), src.data_ptr(), dst.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad_grain = [(nan, 0.0), (inf, 0.0), (-0.01, 0.0), (0.1001, 0.0), (1.0, 0.0), (0.01, nan), (0.01, -0.1), (0.01, 1.0), (0.01, inf),
                 (0.0, 1.0), (0.0, nan)]                  # the seed is checked with the grain off too
    n = 0
    for g in bad_grain:
        assert lib.hdrtv_rgb48_film_grain(ctx, st, s, dh, dw, *g, o) == L.EINVAL, g
        assert lib.hdrtv_post_rgb48_grain(ctx, st, i, L.F32, h, w, 0, 0.0, o, *g) == L.EINVAL, g
        assert lib.hdrtv_post_rgb48_scaled_grain(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 0, 0, *g) == L.EINVAL, g
        assert lib.hdrtv_post_rgb48_scaled_grain(ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 0, 0, *g) == L.EINVAL, g
        assert lib.hdrtv_post_rgb48_fsr_grain(ctx, st, i, L.F32, h, w, 0, 0.0, o, dh, dw, 1, 0.2, *g) == L.EINVAL, g
        n += 5
    for g in ((0.01, 0.25), (0.0, 0.25)):                 # everything the twins refuse, grain on and off
        bad = [lib.hdrtv_rgb48_film_grain(*a, *g, o) for a in ((None, st, s, dh, dw), (ctx, st, None, dh, dw), (ctx, st, s, 0, dw), (ctx, st, s, dh, -1))]
        bad.append(lib.hdrtv_rgb48_film_grain(ctx, st, s, dh, dw, *g, None))
        for a in ((None, st, i, L.F32, h, w, 0, 0.0, o), (ctx, st, None, L.F32, h, w, 0, 0.0, o), (ctx, st, i, L.F32, h, w, 0, 0.0, None),
                  (ctx, st, i, L.F32, 0, w, 0, 0.0, o), (ctx, st, i, 2, h, w, 0, 0.0, o), (ctx, st, i, L.F32, h, w, 1, 0.0, o)):
            bad.append(lib.hdrtv_post_rgb48_grain(*a, *g))
            bad.append(lib.hdrtv_post_rgb48_scaled_grain(*a, dh, dw, 0, 0, *g))
            bad.append(lib.hdrtv_post_rgb48_fsr_grain(*a, dh, dw, 1, 0.2, *g))
        ok = (ctx, st, i, L.F32, h, w, 0, 0.0, o)
        for tail in ((h - 1, dw, 0, 0), (dh, w - 1, 0, 0), (dh, dw, -1, 0), (dh, dw, 257, 0), (dh, dw, 0, 1031), (dh, dw, 0, 4097)):
            bad.append(lib.hdrtv_post_rgb48_scaled_grain(*ok, *tail, *g))
        for tail in ((h - 1, dw, 1, 0.2), (2 * h + 1, dw, 1, 0.2), (dh, 2 * w + 1, 0, 0.2), (dh, dw, 2, 0.2), (dh, dw, 1, 2.5), (dh, dw, 1, nan)):
            bad.append(lib.hdrtv_post_rgb48_fsr_grain(*ok, *tail, *g))
        assert bad and all(rc == L.EINVAL for rc in bad), (g, bad)
        n += len(bad)
    torch.cuda.synchronize()
    assert n > 100 and (dst.cpu().numpy() == FILL).all()
    assert lib.hdrtv_post_rgb48_scaled_grain(ctx, st, i, L.F32, h, w, 0, -5.0, o, dh, dw, 77, 3426, 0.1, 0.0) == L.OK      # pq = 0 ignores peak_nits; the ends of both ranges
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), A.scale(G.apply(C.sharpen(_unscaled(proc, t, 0), 3426), h, w, 0.0, 0.1), dh, dw, 77))


def test_python_surface(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w, oh, ow = 40, 72, 61, 100
    t = torch.from_numpy(_tensor(h, w)).cuda()
    codes = _unscaled(proc, t, 0)
    seed = L.film_grain_seed(1234, 59)
    assert F(seed) == G.seed(1234, 59)
    dev = torch.from_numpy(codes).cuda()
    assert np.array_equal(proc.postprocess_film_grain(dev, seed=seed).cpu().numpy(), G.apply(codes, h, w, seed, 0.01))
    assert np.array_equal(proc.postprocess_film_grain(dev, intensity=0.05, seed=seed).cpu().numpy(), G.apply(codes, h, w, seed, 0.05))
    assert np.array_equal(proc.postprocess_film_grain(dev, intensity=False).cpu().numpy(), codes) and np.array_equal(dev.cpu().numpy(), codes)
    run = lambda **kw: proc.postprocess_rgb48_scaled(t, ow, oh, **kw).cpu().numpy()      # noqa: E731
    assert np.array_equal(run(film_grain=True, grain_seed=seed), A.scale(G.apply(codes, h, w, seed, 0.01), oh, ow, 0))
    assert np.array_equal(run(film_grain=0.05, grain_seed=seed, cas=0.22, antiring=0.3),
                          A.scale(G.apply(C.sharpen(codes, 3426), h, w, seed, 0.05), oh, ow, 77))
    assert np.array_equal(run(film_grain=True, grain_seed=seed, scaler="fsr"), G.apply(FSR.scale(codes, oh, ow, 0.2), oh, ow, seed, 0.01))
    assert np.array_equal(run(film_grain=False, grain_seed=seed), run()) and np.array_equal(run(), A.scale(codes, oh, ow, 0))
    assert np.array_equal(proc.postprocess_rgb48_scaled(t, w, h, film_grain=True, grain_seed=seed, pq=True, peak_nits=PEAK).cpu().numpy(),
                          G.apply(_unscaled(proc, t, 1), h, w, seed, 0.01))                  # equal sizes: hdrtv_post_rgb48_grain
    for kw in (dict(film_grain=0.2), dict(film_grain="1"), dict(film_grain=True, grain_seed=1.0), dict(film_grain=True, scaler="spline36"),
               dict(film_grain=True, scaler="ssim_superres")):
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError):
        proc.postprocess_rgb48_scaled(t, w // 2, h // 2, downscaler="ssim", film_grain=True)
    for bad in (codes, dev.float(), dev[:, :, :2]):
        with pytest.raises(ValueError):
            proc.postprocess_film_grain(bad)


N, PW, PH, STREAM = 4, 96, 64, 1234


@pytest.fixture(scope="module")
def frames():
    from hdrtv_mi355x import weights as W
    return [W.synthetic_frame(PH, PW, seed=70 + i, kind="noise" if i % 2 else "gradient") for i in range(N)]


def _enqueue_run(golden_dir, frames, lanes, **kw):
    """The frames through enqueue_frame on ``lanes`` lanes, frame i with the seed of stream index i -> (frames, light records)."""
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    grain = kw.pop("film_grain", 0.0)
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0, lanes=lanes)
    try:
        fmt = L.output_format(kw.get("out_pix_fmt", "rgb48le"), "left", *kw.get("out_hw", (PH, PW)))
        n0 = len(p._ycc_scratch)
        srcs = [torch.from_numpy(f).cuda() for f in frames]
        dsts = [torch.full(fmt.shape, FILL, dtype=torch.uint16, device="cuda") for _ in frames]
        recs = [torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") for _ in frames]
        torch.cuda.synchronize()
        for i in range(len(frames)):
            g = dict(film_grain=grain, grain_seed=L.film_grain_seed(STREAM, i)) if grain else {}
            p.enqueue_frame(i % lanes, srcs[i].data_ptr(), PH, PW, dsts[i].data_ptr(), light_ptr=recs[i].data_ptr(), **g, **kw)
        torch.cuda.synchronize()
        if not grain and fmt.is_rgb48 and "out_hw" not in kw:
            assert len(p._ycc_scratch) == n0                                       # off: no new scratch
        return [d.cpu().numpy() for d in dsts], [r.cpu().numpy() for r in recs]
    finally:
        p.close()


@pytest.fixture(scope="module")
def plain(golden_dir, frames):
    return _enqueue_run(golden_dir, frames, 1)


def test_enqueue_frame_on_one_and_two_lanes(golden_dir, frames, plain):
    base, _ = plain
    d1, r1 = _enqueue_run(golden_dir, frames, 1, film_grain=True)
    d2, r2 = _enqueue_run(golden_dir, frames, 2, film_grain=True)
    for i in range(N):
        want = G.apply(base[i], PH, PW, G.seed(STREAM, i), 0.01)
        assert np.array_equal(d1[i], want) and np.array_equal(d2[i], d1[i]), i
        assert np.array_equal(r1[i], LL.record(want)) and np.array_equal(r2[i], r1[i]), i          # the record of the grained codes
    # the delivered size and a Y'CbCr layout: converted from the grained codes through the scratch
    oh, ow = 128, 192
    ycc, rec = _enqueue_run(golden_dir, frames[:2], 2, film_grain=0.05, out_hw=(oh, ow), out_pix_fmt="yuv420p10le", scaler="fsr")
    same, rec0 = _enqueue_run(golden_dir, frames[:2], 1, film_grain=0.05, out_pix_fmt="p010le")
    for i in range(2):
        want = G.apply(FSR.scale(base[i], oh, ow, 0.2), oh, ow, G.seed(STREAM, i), 0.05)
        assert np.array_equal(ycc[i].reshape(-1), Y.pack(want, "yuv420p10le", "left").reshape(-1)), i
        assert np.array_equal(rec[i], LL.record(want)), i
        want0 = G.apply(base[i], PH, PW, G.seed(STREAM, i), 0.05)
        assert np.array_equal(same[i].reshape(-1), Y.pack(want0, "p010le", "left").reshape(-1)) and np.array_equal(rec0[i], LL.record(want0)), i


def _worker_run(golden_dir, tmp_path, tag, frames, first_index=0, **kw):
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
            wk._process_frame(frame=f, frame_idx=first_index + i, mpv_w=True)
        assert done.wait(30.0)
    finally:
        wk._stop_hdr_feeder()
        cl = wk.content_light
        wk.close()
    return got, light, cl


def test_worker_grains_every_frame_with_its_own_seed(golden_dir, tmp_path, frames):
    from hdrtv_mi355x.lightlevel import ContentLightLevel
    base, _, _ = _worker_run(golden_dir, tmp_path, "plain", frames)
    got, light, cl = _worker_run(golden_dir, tmp_path, "grain", frames, film_grain=True, grain_stream_seed=STREAM, light_stats=True)
    want_cl = ContentLightLevel()
    for i in range(N):
        want = G.apply(base[i], PH, PW, G.seed(STREAM, i), 0.01)
        assert got[i].shape == (PH, PW, 3) and np.array_equal(got[i], want), i
        assert np.array_equal(light[i], LL.record(want)), i
        want_cl.update(LL.record(want))
    assert cl.as_dict() == want_cl.as_dict()
    # consecutive frames carry different grain: the same picture at two indices differs, and by exactly the seeds
    twice, _, _ = _worker_run(golden_dir, tmp_path, "twice", [frames[0], frames[0]], first_index=7, film_grain=True, grain_stream_seed=STREAM)
    assert not np.array_equal(twice[0], twice[1])
    for j in range(2):
        assert np.array_equal(twice[j], G.apply(base[0], PH, PW, G.seed(STREAM, 7 + j), 0.01)), j


def test_dispatcher_seeds_by_the_frame_index_whatever_the_lane(golden_dir, frames, plain):
    from hdrtv_mi355x.dispatch import FrameDispatcher
    base, _ = plain
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": False, "lanes": 2}
    with FrameDispatcher(1, PH, PW, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0], slots=3, film_grain=True,
                         grain_stream_seed=STREAM) as d:
        assert d.film_grain == 0.01 and d.grain_stream_seed == STREAM
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0] and sorted(got) == list(range(N))
    for i in range(N):
        assert np.array_equal(got[i], G.apply(base[i], PH, PW, G.seed(STREAM, i), 0.01)), i
