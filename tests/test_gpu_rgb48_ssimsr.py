"""hdrtv_post_rgb48_ssimsr on a real MI355X: the spline36 upscale of the RGB48 output, optionally with the SSimSuperRes passes behind
it, and the routes through postprocess_rgb48_scaled and enqueue_frame that carry the two scaler names.

The yardstick is always the composition: what the EXISTING unscaled entry point writes at the processing size (hdrtv_post_rgb48, or
hdrtv_post_pq_rgb48 for pq; pinned by the other GPU tests, so no quantiser is restated here), then tests/rgb48_ssimsr_ref (integer
stage A, float32 stage B op by op).  Equality is exact: every value of every frame."""
import os

import numpy as np
import pytest

import rgb48_scale_ref as S
import rgb48_ssimsr_ref as R
import ycbcr10_ref as Y
from test_gpu_rgb48_fsr import PEAK, _unscaled, contents

pytestmark = pytest.mark.gpu

# source (H, W) -> destination (dH, dW).  The kernel's tile is 16 x 32 output pixels.
SHAPES = [
    ((36, 52), (72, 104)),        # exact 2x, several tiles
    ((17, 33), (33, 65)),         # just under 2x; one row and column past a tile
    ((24, 40), (36, 60)),         # 1.5x: the rounding ties of the final pass
    ((37, 53), (64, 101)),        # ragged ratios; odd dW
    ((33, 70), (34, 71)),         # a ratio next to 1: the largest low-resolution footprint
    ((5, 7), (10, 14)),
    ((2, 3), (3, 4)),
    ((1, 1), (2, 2)),             # everything clamps
]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _ssimsr(p, t, pq, dh, dw, ssim):
    """The C entry point itself."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device=t.device)
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    p._chk(p._lib.hdrtv_post_rgb48_ssimsr(p._ctx, p._stream(), t.data_ptr(), dt, h, w, pq, PEAK, o.data_ptr(), dh, dw, ssim), "post_rgb48_ssimsr")
    return o.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_ssimsr_equals_the_composition(proc, src, dst):
    import torch
    (h, w), (dh, dw) = src, dst
    total = 0
    for name, x in contents(h, w).items():
        for dtype in (torch.float32, torch.float16):
            t = torch.from_numpy(x).to("cuda", dtype).contiguous()
            for pq in (0, 1):
                codes = _unscaled(proc, t, pq)
                want = {0: R.scale(codes, dh, dw), 1: R.scale(codes, dh, dw, ssim=True)}
                for ssim in (0, 1):
                    got = _ssimsr(proc, t, pq, dh, dw, ssim)
                    bad = got != want[ssim]
                    print("%s %s pq=%d ssim=%d: %d of %d values differ, largest |difference| %d" % (
                        name, str(dtype), pq, ssim, int(bad.sum()), bad.size, int(np.abs(got.astype(int) - want[ssim].astype(int)).max())))
                    assert not bad.any(), (name, str(dtype), pq, ssim)
                    total += 1
                if name == "noise" and h > 2 and pq == 0:              # the content gives both stages something to do
                    assert not np.array_equal(want[0], want[1])
                    assert not np.array_equal(want[0], S.scale(codes, dh, dw))
    assert total == 6 * 2 * 2 * 2


def test_equal_sizes_are_the_unscaled_bytes(proc):
    import torch
    x = contents(36, 52)["noise"]
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            codes = _unscaled(proc, t, pq)
            for ssim in (0, 1):
                assert np.array_equal(_ssimsr(proc, t, pq, 36, 52, ssim), codes), (str(dtype), pq, ssim)


def test_every_refused_call_leaves_dst_alone(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 40, 48
    t = torch.rand((3, h, w), device="cuda")
    dst = torch.full((2 * h + 1, 2 * w, 3), 0xA5A5, dtype=torch.uint16, device="cuda")
    fn, ctx, st, i, o = proc._lib.hdrtv_post_rgb48_ssimsr, proc._ctx, proc._stream(), t.data_ptr(), dst.data_ptr()
    bad = []
    for s in (0, 1):
        bad += [
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, 40, 96, s), (ctx, st, i, L.F32, h, w, 0, 0.0, o, 80, 48, s),        # one axis at identity
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, 81, 96, s), (ctx, st, i, L.F32, h, w, 0, 0.0, o, 80, 97, s),        # more than 2x
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, 39, 96, s), (ctx, st, i, L.F32, h, w, 0, 0.0, o, 80, 47, s),        # shrinking
            (ctx, st, i, L.F32, h, w, 0, 0.0, o, 39, 47, s), (ctx, st, i, L.F32, h, w, 0, 0.0, o, 0, 0, s),
            (None, st, i, L.F32, h, w, 0, 0.0, o, 80, 96, s), (ctx, st, None, L.F32, h, w, 0, 0.0, o, 80, 96, s),
            (ctx, st, i, L.F32, h, w, 0, 0.0, None, 80, 96, s), (ctx, st, i, L.F32, 0, w, 0, 0.0, o, 80, 96, s),
            (ctx, st, i, 2, h, w, 0, 0.0, o, 80, 96, s), (ctx, st, i, L.F32, h, w, 1, 0.0, o, 80, 96, s),
            (ctx, st, i, L.F32, h, w, 1, -1.0, o, h, w, s),                                                          # equal sizes too
        ]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, 80, 96, s) for s in (2, -1, 256)]
    bad += [(ctx, st, i, L.F32, h, w, 0, 0.0, o, h, w, 2)]
    for n, a in enumerate(bad):
        assert fn(*a) == L.EINVAL, n
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0xA5A5).all()
    assert fn(ctx, st, i, L.F32, h, w, 0, -5.0, o, 80, 96, 1) == L.OK          # pq = 0 ignores peak_nits
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(-1)[:80 * 96 * 3].reshape(80, 96, 3)
    assert np.array_equal(got, R.scale(_unscaled(proc, t, 0), 80, 96, ssim=True))


def test_python_surface(proc):
    import torch
    t = torch.from_numpy(contents(36, 52)["noise"]).cuda()
    codes = _unscaled(proc, t, 0)
    run = lambda **kw: proc.postprocess_rgb48_scaled(t, 101, 64, **kw).cpu().numpy()      # noqa: E731
    n = len(proc._ycc_scratch)
    for s, ssim in (("spline36", False), ("ssim_superres", True)):                        # 36x52 -> 72x104
        assert np.array_equal(proc.postprocess_rgb48_scaled(t, 104, 72, scaler=s).cpu().numpy(), R.scale(codes, 72, 104, ssim=ssim))
    assert np.array_equal(run(scaler="spline36"), R.scale(codes, 64, 101))
    assert np.array_equal(run(scaler="SSIM_SuperRes", cas="auto", antiring="auto"), R.scale(codes, 64, 101, ssim=True))
    assert np.array_equal(run(scaler="ssim_superres", pq=True, peak_nits=PEAK), R.scale(_unscaled(proc, t, 1), 64, 101, ssim=True))
    assert np.array_equal(proc.postprocess_rgb48_scaled(t, 52, 36, scaler="ssim_superres").cpu().numpy(), codes)      # equal sizes
    # "lanczos", or leaving it out, gives the bytes of a call that names no scaler
    assert np.array_equal(run(), S.scale(codes, 64, 101)) and np.array_equal(run(scaler="lanczos"), run())
    assert len(proc._ycc_scratch) == n
    for s in ("spline36", "ssim_superres"):
        for kw in (dict(cas=0.2), dict(antiring=0.3), dict(downscaler="ssim")):
            with pytest.raises(ValueError):
                run(scaler=s, **kw)
        with pytest.raises(ValueError, match="2x"):
            proc.postprocess_rgb48_scaled(t, 105, 72, scaler=s)                            # 105 > 2 * 52
        with pytest.raises(ValueError, match="both axes"):
            proc.postprocess_rgb48_scaled(t, 52, 72, scaler=s)


def test_enqueue_frame_and_everything_behind_the_scaler_see_the_new_codes(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w, oh, ow = 64, 96, 128, 192          # the model refuses 36x52 (too small for its classifier): the smallest size of the sibling tests
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        dev = torch.from_numpy(W.synthetic_frame(h, w, seed=77, kind="noise")).cuda()
        st = torch.cuda.current_stream()
        new = lambda fmt, hh, ww: torch.full(L.output_format(fmt, "left", hh, ww).shape, 0xA5A5, dtype=torch.uint16, device="cuda")   # noqa: E731
        run = lambda dst, **kw: p.enqueue_frame(0, dev.data_ptr(), h, w, dst.data_ptr(), stream=st, **kw)                           # noqa: E731
        small, lan, lan2, sp, sr, same = (new("rgb48le", *s) for s in ((h, w), (oh, ow), (oh, ow), (oh, ow), (oh, ow), (h, w)))
        run(small)
        run(lan, out_hw=(oh, ow))
        run(lan2, out_hw=(oh, ow), scaler="lanczos")
        run(sp, out_hw=(oh, ow), scaler="spline36")
        run(sr, out_hw=(oh, ow), scaler="ssim_superres", cas="auto", antiring="auto")
        run(same, scaler="ssim_superres")                           # nothing is enlarged: the unscaled frame
        torch.cuda.synchronize()
        codes = small.cpu().numpy()
        assert np.array_equal(lan.cpu().numpy(), S.scale(codes, oh, ow)) and np.array_equal(lan2.cpu().numpy(), lan.cpu().numpy())
        assert np.array_equal(sp.cpu().numpy(), R.scale(codes, oh, ow))
        assert np.array_equal(sr.cpu().numpy(), R.scale(codes, oh, ow, ssim=True))
        assert np.array_equal(same.cpu().numpy(), codes)
        assert not np.array_equal(sr.cpu().numpy(), sp.cpu().numpy()) and not np.array_equal(sp.cpu().numpy(), lan.cpu().numpy())
        # a scaled p010le frame = the conversion of the SSimSuperRes codes; its record = the statistic of those codes
        ycc = new("p010le", oh, ow)
        rec, want_rec = (torch.zeros(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda") for _ in range(2))
        run(ycc, out_hw=(oh, ow), out_pix_fmt="p010le", scaler="ssim_superres", light_ptr=rec.data_ptr())
        p._chk(p._lib.hdrtv_rgb48_light_stats(p._ctx, p._stream(), sr.data_ptr(), oh, ow, 0, 0, ow, oh, want_rec.data_ptr()), "rgb48_light_stats")
        torch.cuda.synchronize()
        assert np.array_equal(ycc.cpu().numpy().reshape(-1), Y.pack(sr.cpu().numpy(), "p010le", "left").reshape(-1))
        assert np.array_equal(rec.cpu().numpy(), want_rec.cpu().numpy())
        # deband sits behind the scaler too
        deb = new("rgb48le", oh, ow)
        run(deb, out_hw=(oh, ow), scaler="ssim_superres", cleanup=L.output_cleanup(True))
        torch.cuda.synchronize()
        assert np.array_equal(deb.cpu().numpy(), p.postprocess_deband(sr).cpu().numpy())
        for kw in (dict(scaler="ssim_superres", cas=0.2), dict(scaler="spline36", antiring=0.1), dict(scaler="ssim")):
            with pytest.raises(ValueError):
                run(sr, out_hw=(oh, ow), **kw)
        with pytest.raises(ValueError, match="2x"):
            run(new("rgb48le", 129, 192), out_hw=(129, 192), scaler="ssim_superres")
        with pytest.raises(ValueError, match="both axes"):
            run(new("rgb48le", 64, 192), out_hw=(64, 192), scaler="spline36")
    finally:
        p.close()
