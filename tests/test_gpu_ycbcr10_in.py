"""10-bit Y'CbCr input (P010, yuv420p10le, yuv422p10le) on a real MI355X: hdrtv_ycbcr10_to_rgb10 against the rule
(tests/ycbcr10_in_ref.py) bit for bit, at two-byte plane alignment and padded pitches; hdrtv_preprocess_ycbcr10 (pre_fused's 10-bit
staging) against fp16(code / 1023) of those codes bit for bit, its condition map against the oracle, and both outputs against
hdrtv_preprocess of the BGR frame where the two must agree exactly (grey frames of black and white); the fp32 context; the argument
rules on a real context; the processor, worker and dispatcher surfaces against the direct calls."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import ycbcr10_in_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (64, 96), (46, 142), (90, 270)]          # (H, W): tiny, one tile, a patch edge, a ragged multi-tile frame
PAIRS = [(m, full) for m in (709, 601, 2020) for full in (0, 1)]
# hdrtv_preprocess_ycbcr10 needs hdrtv_reserve(H, W), and hdrtv_reserve refuses 8 x 8 (the AGCM classifier's fourth block needs two
# spatial elements: ceil(H/4 / 16) * ceil(W/4 / 16) >= 2, as the reference raises there).  The preprocess tests therefore run the two
# smallest frames a context can reserve, 8 x 68 and 68 x 8, in the place of 8 x 8; what holds for 8 x 8 itself (no reservation, so
# HDRTV_ESTATE and untouched destinations) is test_preprocess_of_an_unreservable_8x8_frame_is_estate.
PRE_SIZES = [(8, 68), (68, 8)] + SIZES[1:]
COND_TOL = 1e-3                                            # tests/test_gpu_parity.py's bound for the condition map against the oracle


def _proc(golden_dir, **kw):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    return HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=kw.pop("use_hg", False), warmup_passes=0, **kw)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _frame(h, w, fmt, seed=0):
    return R.random_frame(h, w, seed=1000 * h + w + seed, pix_fmt=fmt, noisy_pad=True)


@functools.lru_cache(maxsize=None)
def _codes(h, w, fmt, matrix=709, full=0, seed=0):
    """The rule's codes of ``_frame``: computed once, shared by the tests, never written to."""
    c = R.to_rgb10(_frame(h, w, fmt, seed), fmt, matrix, bool(full))
    c.setflags(write=False)
    return c


GUARD = 8     # u16 words of canary either side of every plane


class Planes:
    """A 10-bit frame in one device buffer with the planes where a test puts them: luma at byte ``off`` (even) past the first guard,
    pitches of minimum + ``extra`` bytes (even), GUARD words of noise around every plane and noise in the pitch padding.  The kernels
    only read it: ``unchanged()`` says whether the whole buffer, guards included, came back as it was."""

    def __init__(self, frame, fmt, off=0, extra=0, seed=0):
        import torch
        Y, U, V = R.split(frame, fmt)
        h, w = Y.shape
        hc = U.shape[0]
        self.h, self.w, self.fmt = h, w, R.FMT[fmt]
        self.yp = 2 * w + extra
        self.cp = (2 * w if fmt == "p010le" else w) + extra
        ypw, cpw = self.yp // 2, self.cp // 2
        rng = np.random.default_rng(seed)
        yo = off // 2 + GUARD
        uo = yo + ypw * h + GUARD
        vo = uo + cpw * hc + GUARD
        n = (vo if fmt == "p010le" else vo + cpw * hc + GUARD) + 2
        host = rng.integers(0, 65536, n, dtype=np.uint16)
        for r in range(h):
            host[yo + r * ypw: yo + r * ypw + w] = Y[r]
        for r in range(hc):
            if fmt == "p010le":
                row = host[uo + r * cpw: uo + r * cpw + w]
                row[0::2], row[1::2] = U[r], V[r]
            else:
                host[uo + r * cpw: uo + r * cpw + w // 2] = U[r]
                host[vo + r * cpw: vo + r * cpw + w // 2] = V[r]
        self.host = host
        self.buf = torch.from_numpy(host.copy()).cuda()
        base = self.buf.data_ptr()
        self.y, self.u = base + 2 * yo, base + 2 * uo
        self.v = None if fmt == "p010le" else base + 2 * vo

    def args(self):
        return (self.y, self.yp, self.u, self.v, self.cp, self.fmt)

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.host)


def _to_rgb10(p, planes, matrix=709, full=0, guard=0):
    """hdrtv_ycbcr10_to_rgb10 into a device buffer with `guard` canary words either side (destination at an odd word)."""
    import torch
    h, w = planes.h, planes.w
    n = h * w * 3
    dst = torch.full((n + 2 * guard + 1,), 0xA5A5, dtype=torch.uint16, device="cuda")
    o = guard + 1 if guard else 0
    rc = p._lib.hdrtv_ycbcr10_to_rgb10(p._ctx, _stream(), *planes.args(), matrix, full, h, w, dst.data_ptr() + 2 * o)
    assert rc == 0, p._lib.hdrtv_last_error(p._ctx)
    host = dst.cpu().numpy()
    if guard:
        assert (host[:o] == 0xA5A5).all() and (host[o + n:] == 0xA5A5).all()
    return host[o:o + n].reshape(h, w, 3)


@pytest.fixture(scope="module")
def proc(golden_dir):
    p = _proc(golden_dir)
    yield p
    p.close()


# ---- 1. the rule on its own -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.PIX_FMTS)
@pytest.mark.parametrize("h,w", SIZES + [(1080, 1920)])
def test_device_codes_equal_the_rule_every_fmt_matrix_and_range(proc, h, w, fmt):
    planes = Planes(_frame(h, w, fmt), fmt)
    for m, full in PAIRS:
        got = _to_rgb10(proc, planes, m, full)
        assert got.max() <= 1023
        assert np.array_equal(got, _codes(h, w, fmt, m, full)), (m, full)
    assert planes.unchanged()


# The smallest frames the chroma walk of csrc/ycc_in.h can still go wrong at: Hc = 1 or Wc = 1 puts the j - 1, j + 1 and i + 1 clamps on
# the same sample, and the odd-height 4:2:2 frames are legal by the argument rule.  The stand-alone converter needs no hdrtv_reserve.
TINY = [(2, 2), (2, 6), (6, 2)]
TINY_CASES = [(h, w, fmt) for fmt in R.PIX_FMTS for h, w in TINY] + [(1, 2, "yuv422p10le"), (3, 4, "yuv422p10le")]


@pytest.mark.parametrize("h,w,fmt", TINY_CASES)
def test_device_codes_smallest_frames(proc, h, w, fmt):
    """Tight pitches; luma and chroma pitches padded by one dword; the plane bases offset by one sample (two bytes); both."""
    want = _codes(h, w, fmt)
    for off, extra in ((0, 0), (0, 4), (2, 0), (2, 4)):
        planes = Planes(_frame(h, w, fmt), fmt, off=off, extra=extra, seed=off + extra)
        assert np.array_equal(_to_rgb10(proc, planes, guard=16), want), (off, extra)
        assert planes.unchanged()


# ---- 2. two-byte alignment, padded pitches, guard words, the six unused bits ------------------------------------------------------
@pytest.mark.parametrize("extra", [2, 6])
def test_device_codes_offset_planes_padded_pitches_and_guard_words(proc, extra):
    for fmt in R.PIX_FMTS:
        for h, w in ((46, 142), (90, 270)):
            noisy = _frame(h, w, fmt)                                    # the six unused bits of every word are noise ...
            Y, U, V = (R.values(p, fmt) for p in R.split(noisy, fmt))
            clean = R.from_values(Y, U, V, fmt)                          # ... and here zero: the same codes
            assert not np.array_equal(noisy, clean)
            want = _codes(h, w, fmt)
            for f in (noisy, clean):
                planes = Planes(f, fmt, off=2, extra=extra, seed=extra)
                assert planes.y % 4 == 2                                 # a plane base that is two-byte aligned and no more
                assert np.array_equal(_to_rgb10(proc, planes, guard=64), want), (fmt, h, w)
                assert planes.unchanged(), (fmt, h, w)


# ---- 3. the fused preprocess, fp16 -------------------------------------------------------------------------------------------------
def _preprocess(p, planes, matrix, full):
    import torch
    h, w = planes.h, planes.w
    dt = torch.float32 if p._fp32 else torch.float16
    rgb = torch.full((3, h, w), -7.0, dtype=dt, device="cuda")
    cond = torch.full((3, h // 4, w // 4), -7.0, dtype=dt, device="cuda")
    lib, ctx = p._lib, p._ctx
    assert lib.hdrtv_reserve(ctx, h, w) == 0, lib.hdrtv_last_error(ctx)
    rc = lib.hdrtv_preprocess_ycbcr10(ctx, _stream(), *planes.args(), matrix, full, h, w, rgb.data_ptr(), cond.data_ptr())
    assert rc == 0, lib.hdrtv_last_error(ctx)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), cond.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32),
                                                                        b.view(np.uint16 if b.dtype == np.float16 else np.uint32))


def _cond_ref(tensor, mode):
    """The oracle's condition map of a [3][H][W] tensor in condition mode ``mode``: the 0.25x antialiased bicubic
    (oracle.bicubic_aa_quarter), mode 1 its fast bilinear form, mode 2 zero."""
    from oracle import hdrtvnet_oracle as O
    t = tensor.astype(np.float32)
    if mode == 0:
        return O.bicubic_aa_quarter(t)
    if mode == 1:
        return O.bilinear_quarter(t)
    return np.zeros((3, t.shape[1] // 4, t.shape[2] // 4), np.float32)


FMT_PAIR = {"p010le": (709, 0), "yuv420p10le": (601, 1), "yuv422p10le": (2020, 0)}


@pytest.mark.parametrize("fmt", R.PIX_FMTS)
@pytest.mark.parametrize("h,w", PRE_SIZES + [(1080, 1920)])
def test_fused_preprocess_tensor_is_the_rule_and_cond_is_the_oracles(proc, h, w, fmt):
    m, full = FMT_PAIR[fmt]
    want = R.tensor_f16(_codes(h, w, fmt, m, full))
    small = h * w < 100000
    planes = Planes(_frame(h, w, fmt), fmt, off=2 if small else 0, extra=6 if small else 0)
    try:
        for mode in (0, 1, 2):
            assert proc._lib.hdrtv_set_cond_mode(proc._ctx, mode) == 0
            t, c = _preprocess(proc, planes, m, full)
            assert _same_bits(t, want), (mode, int((t.view(np.uint16) != want.view(np.uint16)).sum()))
            ref = _cond_ref(want, mode).astype(np.float16).astype(np.float32)
            err = float(np.abs(c.astype(np.float32) - ref).max())        # every pixel of the map
            print(f"{fmt} {h}x{w} mode {mode}: |cond - oracle|max = {err:.3e}")
            assert c.shape == ref.shape and err <= COND_TOL, (mode, err)
        assert planes.unchanged()
    finally:
        assert proc._lib.hdrtv_set_cond_mode(proc._ctx, 0) == 0


def test_preprocess_of_an_unreservable_8x8_frame_is_estate(proc):
    import torch
    from hdrtv_mi355x import lib as L
    lib, ctx = proc._lib, proc._ctx
    assert lib.hdrtv_reserve(ctx, 8, 8) == L.EINVAL and b"too small" in lib.hdrtv_last_error(ctx)
    rgb = torch.full((3, 8, 8), -7.0, dtype=torch.float16, device="cuda")
    cond = torch.full((3, 2, 2), -7.0, dtype=torch.float16, device="cuda")
    for fmt in R.PIX_FMTS:
        planes = Planes(_frame(8, 8, fmt), fmt)
        assert lib.hdrtv_preprocess_ycbcr10(ctx, _stream(), *planes.args(), 709, 0, 8, 8, rgb.data_ptr(), cond.data_ptr()) == L.ESTATE
    torch.cuda.synchronize()
    assert (rgb.cpu().numpy() == -7.0).all() and (cond.cpu().numpy() == -7.0).all()


# ---- 4. the shared half, bit for bit: grey frames of black and white against hdrtv_preprocess of the BGR frame ---------------------
@pytest.mark.parametrize("h,w", [(46, 142), (90, 270)])
def test_grey_frames_equal_preprocess_of_the_bgr_frame_bit_for_bit(proc, h, w):
    import torch
    rng = np.random.default_rng(h)
    yy, xx = np.mgrid[0:h, 0:w]
    lib, ctx = proc._lib, proc._ctx
    try:
        for name, bits in (("noise", rng.integers(0, 2, (h, w))), ("checker", (yy + xx) & 1)):
            bgr = torch.from_numpy(np.ascontiguousarray(np.repeat((bits * 255).astype(np.uint8)[..., None], 3, axis=2))).cuda()
            for mode in (0, 1, 2):
                assert lib.hdrtv_set_cond_mode(ctx, mode) == 0
                assert lib.hdrtv_reserve(ctx, h, w) == 0
                t8 = torch.empty((3, h, w), dtype=torch.float16, device="cuda")
                c8 = torch.empty((3, h // 4, w // 4), dtype=torch.float16, device="cuda")
                assert lib.hdrtv_preprocess(ctx, _stream(), bgr.data_ptr(), h, w, t8.data_ptr(), c8.data_ptr()) == 0
                torch.cuda.synchronize()
                t8, c8 = t8.cpu().numpy(), c8.cpu().numpy()
                assert set(np.unique(t8).tolist()) == {0.0, 1.0}
                for fmt in R.PIX_FMTS:
                    planes = Planes(R.grey_frame(np.where(bits, 940, 64), fmt), fmt, off=2, extra=2)
                    t, c = _preprocess(proc, planes, 709, 0)
                    assert _same_bits(t, t8), (name, mode, fmt)
                    assert _same_bits(c, c8), (name, mode, fmt, int((c.view(np.uint16) != c8.view(np.uint16)).sum()))
    finally:
        assert lib.hdrtv_set_cond_mode(ctx, 0) == 0


# ---- 5. the fp32 context -----------------------------------------------------------------------------------------------------------
def test_fp32_context_tensor_exact_and_cond_within_the_bound(golden_dir):
    p = _proc(golden_dir, precision="fp32")
    try:
        for h, w in ((46, 142), (90, 270)):
            for fmt in R.PIX_FMTS:
                m, full = FMT_PAIR[fmt]
                want = R.tensor_f32(_codes(h, w, fmt, m, full))
                planes = Planes(_frame(h, w, fmt), fmt, off=2, extra=2)
                for mode in (0, 1, 2):
                    assert p._lib.hdrtv_set_cond_mode(p._ctx, mode) == 0
                    t, c = _preprocess(p, planes, m, full)
                    assert t.dtype == np.float32 and _same_bits(t, want), (h, w, fmt, mode)
                    err = float(np.abs(c - _cond_ref(want, mode)).max())
                    print(f"fp32 {fmt} {h}x{w} mode {mode}: |cond - oracle|max = {err:.3e}")
                    assert err <= COND_TOL, (h, w, fmt, mode, err)
    finally:
        p.close()


# ---- 6. argument rules ---------------------------------------------------------------------------------------------------------------
def test_argument_rules_on_a_real_context(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    p = _proc(golden_dir)
    try:
        lib, ctx, st = p._lib, p._ctx, _stream()
        h, w = 64, 96
        b = torch.zeros(65536, dtype=torch.uint16, device="cuda")
        y = b.data_ptr()
        u, v = y + 2 * h * w, y + 2 * h * w + h * w          # planar 4:2:2 needs the most: H rows of W bytes per chroma plane
        codes = torch.full((h * w * 3,), 0x5A5A, dtype=torch.uint16, device="cuda")
        out = torch.full((3, h, w), -3.0, dtype=torch.float16, device="cuda")
        cond = torch.full((3, h // 4, w // 4), -3.0, dtype=torch.float16, device="cuda")
        P010, P420, P422 = L.YCC_P010, L.YCC_YUV420P10, L.YCC_YUV422P10
        good = [(y, 2 * w, u, None, 2 * w, P010, 709, 0, h, w), (y, 2 * w, u, v, w, P420, 601, 1, h, w),
                (y, 2 * w + 2, u, v, w + 2, P422, 2020, 0, h - 1, w)]       # an odd height is fine for 4:2:2
        bad = [(None, 2 * w, u, v, w, P420, 709, 0, h, w), (y, 2 * w, None, v, w, P420, 709, 0, h, w),       # NULL planes
               (y, 2 * w, u, v, w, P420, 709, 0, h, 0), (y, 2 * w, u, v, w, P420, 709, 0, h, -2),            # non-positive W
               (y, 2 * w, u, v, w, P420, 709, 0, h, w - 1), (y, 2 * w, u, v, w, P422, 709, 0, h, w - 1),     # odd W
               (y, 2 * w, u, v, w, P420, 709, 0, 0, w),                                                      # non-positive H
               (y, 2 * w, u, v, w, P420, 709, 0, h - 1, w), (y, 2 * w, u, None, 2 * w, P010, 709, 0, h - 1, w),   # odd H with 4:2:0
               (y, 2 * w - 2, u, v, w, P420, 709, 0, h, w), (y, 2 * w + 1, u, v, w, P420, 709, 0, h, w),     # short / odd luma pitch
               (y, 2 * w, u, v, w - 2, P420, 709, 0, h, w), (y, 2 * w, u, v, w + 1, P422, 709, 0, h, w),     # short / odd chroma pitch
               (y, 2 * w, u, None, 2 * w - 2, P010, 709, 0, h, w), (y, 2 * w, u, None, 2 * w + 1, P010, 709, 0, h, w),
               (y, 2 * w, u, v, w, 3, 709, 0, h, w), (y, 2 * w, u, v, w, -1, 709, 0, h, w),                  # unknown fmt
               (y, 2 * w, u, v, w, P420, 700, 0, h, w), (y, 2 * w, u, v, w, P420, 709, 2, h, w),             # unknown matrix / range
               (y, 2 * w, u, v, 2 * w, P010, 709, 0, h, w),                                                  # P010 with dev_v
               (y, 2 * w, u, None, w, P420, 709, 0, h, w), (y, 2 * w, u, None, w, P422, 709, 0, h, w)]       # planar without dev_v
        for a in good:
            assert lib.hdrtv_ycbcr10_to_rgb10(ctx, st, *a, codes.data_ptr()) == L.OK, (a, lib.hdrtv_last_error(ctx))
        codes.fill_(0x5A5A)
        torch.cuda.synchronize()
        for a in bad:
            assert lib.hdrtv_ycbcr10_to_rgb10(ctx, st, *a, codes.data_ptr()) == L.EINVAL, a
        assert lib.hdrtv_ycbcr10_to_rgb10(ctx, st, *good[0], None) == L.EINVAL
        # preprocess: ESTATE before a reservation of this size, then the same rules and null outputs
        for a in good[:2]:
            assert lib.hdrtv_preprocess_ycbcr10(ctx, st, *a, out.data_ptr(), cond.data_ptr()) == L.ESTATE
        assert lib.hdrtv_reserve(ctx, h, w) == L.OK
        for a in bad:
            assert lib.hdrtv_preprocess_ycbcr10(ctx, st, *a, out.data_ptr(), cond.data_ptr()) == L.EINVAL, a
        assert lib.hdrtv_preprocess_ycbcr10(ctx, st, *good[0], None, cond.data_ptr()) == L.EINVAL
        assert lib.hdrtv_preprocess_ycbcr10(ctx, st, *good[0], out.data_ptr(), None) == L.EINVAL
        assert lib.hdrtv_preprocess_ycbcr10(ctx, st, *good[2], out.data_ptr(), cond.data_ptr()) == L.ESTATE     # 63 rows: not reserved
        torch.cuda.synchronize()
        # every refusal left the poisoned destinations as they were
        assert (codes.cpu().numpy() == 0x5A5A).all()
        assert (out.cpu().numpy() == -3.0).all() and (cond.cpu().numpy() == -3.0).all()
        for a in good[:2]:
            assert lib.hdrtv_preprocess_ycbcr10(ctx, st, *a, out.data_ptr(), cond.data_ptr()) == L.OK, lib.hdrtv_last_error(ctx)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() != -3.0).all() and (cond.cpu().numpy() != -3.0).all()
    finally:
        p.close()


# ---- 7. surfaces -------------------------------------------------------------------------------------------------------------------
def _rgb48_of(p, out, h, w):
    """hdrtv_post_rgb48 of the model's output tensor, as a host array."""
    import torch
    o = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    p._chk(p._lib.hdrtv_post_rgb48(p._ctx, p._stream(), out.data_ptr(), p._out_dt, h, w, o.data_ptr()), "hdrtv_post_rgb48")
    torch.cuda.synchronize()
    return o.cpu().numpy()


def test_processor_surfaces_equal_the_direct_calls(golden_dir):
    import torch
    p = _proc(golden_dir, use_hg=True, hg_weights="seeded:1234", lanes=2)
    try:
        h, w = 72, 128
        for fmt in R.PIX_FMTS:
            m, full = FMT_PAIR[fmt]
            kw = dict(pix_fmt=fmt, matrix=m, full_range=bool(full))
            f = _frame(h, w, fmt)
            t, c = p.preprocess_ycbcr10(f, **kw)
            assert _same_bits(t.cpu().numpy()[0], R.tensor_f16(_codes(h, w, fmt, m, full))), fmt
            out, _ = p.infer((t, c))
            want_u8 = p.postprocess(out).copy()
            want48 = _rgb48_of(p, out, h, w)
            assert np.array_equal(p.process_ycbcr10(f, **kw), want_u8), fmt
            dev = torch.from_numpy(f).cuda()
            for lane in (0, 1):
                o = torch.zeros((h, w, 3), dtype=torch.uint16, device="cuda")
                torch.cuda.synchronize()
                p.enqueue_frame_ycbcr10(lane, dev.data_ptr(), h, w, o.data_ptr(), **kw)
                torch.cuda.synchronize()
                assert np.array_equal(o.cpu().numpy(), want48), (fmt, lane)
        with pytest.raises(ValueError):
            p.preprocess_ycbcr10(np.zeros((12, 8), np.uint8), pix_fmt="p010le")            # not u16
        with pytest.raises(ValueError):
            p.preprocess_ycbcr10(np.zeros((10, 8), np.uint16), pix_fmt="yuv420p10le")      # 10 rows is not H*3//2 of an even H
        with pytest.raises(ValueError):
            p.preprocess_ycbcr10(np.zeros((12, 8), np.uint16), pix_fmt="yuv444p10le")
        with pytest.raises(ValueError):
            p.preprocess_ycbcr10(np.zeros((12, 8), np.uint16), pix_fmt="p010le", matrix=700)
    finally:
        p.close()


def test_playback_yuv422p10le_clip_into_rgb48le_sink(golden_dir, tmp_path):
    """End to end: a three-frame yuv422p10le rawvideo clip -> prefetch -> worker (device conversion) -> rgb48le sink writes the
    bytes the direct calls give; a source of another size is refused (no 10-bit letterbox)."""
    from hdrtv_mi355x import playback as P
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    wdir = tmp_path / "weights" / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    h, w, n, fmt = 64, 96, 3, "yuv422p10le"
    frames = [_frame(h, w, fmt, seed=60 + i) for i in range(n)]
    (tmp_path / "clip.yuv").write_bytes(b"".join(f.astype("<u2").tobytes() for f in frames))
    p = _proc(golden_dir, use_hg=True, hg_weights="seeded:1234")
    want = b""
    for f in frames:
        out, _ = p.infer(p.preprocess_ycbcr10(f, pix_fmt=fmt, matrix=2020, full_range=True))
        want += _rgb48_of(p, out, h, w).tobytes()
    p.close()
    wk = HeadlessPipelineWorker(str(tmp_path / "weights"), use_hg=True, proc_w=w, proc_h=h, hg_weights="seeded:1234")
    assert wk._load_model("FP16")
    buf = io.BytesIO()
    sink = P.Rgb48leSink(buf, w, h, 30.0)
    wk._start_hdr_feeder(sink)
    feed = P.PinnedPrefetch(P.RawVideoSource(str(tmp_path / "clip.yuv"), w, h, 30.0, pix_fmt=fmt, yuv_matrix=2020, yuv_full_range=True))
    res = P.RealtimePlayback(wk, feed, sink=True, realtime=False).run()
    import time
    deadline = time.perf_counter() + 10.0
    while sink.frames < res["frames_processed"] and time.perf_counter() < deadline:
        time.sleep(0.01)
    wk._stop_hdr_feeder()
    feed.release()
    assert wk._yuv_format == {"pix_fmt": fmt, "matrix": 2020, "full_range": True}
    with pytest.raises(ValueError, match="letterbox"):
        wk._process_frame(frame=_frame(32, 48, fmt), frame_idx=0, mpv_w=False)
    wk.close()
    assert res["frames_processed"] == n and sink.frames == n
    assert len(buf.getvalue()) == n * h * w * 6 and buf.getvalue() == want


def test_dispatcher_p010le_on_the_device(golden_dir):
    import torch
    from hdrtv_mi355x.dispatch import FrameDispatcher
    h, w, n, fmt = 288, 512, 4, "p010le"
    frames = [_frame(h, w, fmt, seed=300 + i) for i in range(n)]
    p = _proc(golden_dir, use_hg=True, hg_weights="seeded:1234")
    want = []
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    for f in frames:
        dev = torch.from_numpy(f).cuda()
        p.enqueue_frame_ycbcr10(0, dev.data_ptr(), h, w, u16.data_ptr(), pix_fmt=fmt, matrix=601, full_range=True,
                                stream=torch.cuda.current_stream())
        want.append(u16.cpu().numpy().copy())
    p.close()
    got = {}
    args = {"model_path": os.path.join(golden_dir, "hr_weights.hdrw"), "use_hg": True, "hg_weights": "seeded:1234"}
    with FrameDispatcher(2, h, w, lambda i, v: got.__setitem__(i, v.copy()), init_args=args, devices=[0, 0], slots=2,
                         pix_fmt=fmt, yuv_matrix=601, yuv_full_range=True) as d:
        for f in frames:
            d.submit(f)
        d.flush(timeout=120)
    assert d.exit_codes == [0, 0]
    assert sorted(got) == list(range(n))
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i
