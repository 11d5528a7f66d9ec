"""The 10-bit letterbox on a real MI355X: hdrtv_letterbox_ycbcr10 against the rule (tests/letterbox10_ref.py) bit for bit in every
resize mode, every layout, at two-byte plane alignment and padded pitches; the 4x cap; hdrtv_preprocess_ycbcr10_letterboxed against
fp16(code / 1023) of those codes bit for bit and its condition map against the oracle's map of that tensor, fp16 and fp32 contexts,
every condition mode; equal sizes against preprocess_ycbcr10; the argument and reservation rules; the playback command line end to
end.  Sizes are W x H, source -> destination.  The device-buffer helpers are those of tests/test_gpu_ycbcr10_in.py."""
import functools
import json
import os

import numpy as np
import pytest

import letterbox10_ref as LB
import ycbcr10_in_ref as R
from test_gpu_ycbcr10_in import COND_TOL, Planes, _cond_ref, _proc, _rgb48_of, _same_bits, _stream

pytestmark = pytest.mark.gpu

DW, DH = 96, 64
# (sw, sh, dw, dh, the mode the geometry takes)
CASES = [(192, 128, 96, 64, "area_int"),      # 2x2, 3 x 8 tiles
         (288, 192, 96, 64, "area_int"),      # 3x3
         (384, 256, 96, 64, "area_int"),      # 4x4, the cap
         (140, 76, 70, 38, "area_int"),       # 2x2, ragged tiles
         (144, 96, 96, 64, "area_frac"),      # 1.5
         (200, 116, 96, 64, "area_frac"),     # rectangle 96x56: top and bottom bars
         (64, 96, 96, 64, "area_frac"),       # rectangle 43x64: side bars at an odd offset
         (96, 40, 96, 64, "copy"),            # the codes themselves between bars
         (48, 32, 96, 64, "cubic"),           # 2x
         (50, 30, 96, 64, "cubic")]           # rectangle 96x58
# matrix and range per layout, on every case: BT.2020 full range for 4:2:2, BT.709 limited for the two 4:2:0 layouts
FMT_PAIR = {"p010le": (709, 0), "yuv420p10le": (709, 0), "yuv422p10le": (2020, 1)}
PRE_CASES = [CASES[0], CASES[5], CASES[8]]    # 2x2, fractional with bars, cubic -- all onto the reserved 96x64


@functools.lru_cache(maxsize=None)
def _frame(sw, sh, fmt):
    return R.random_frame(sh, sw, seed=7000 + 10 * sw + sh, pix_fmt=fmt, noisy_pad=True)


@functools.lru_cache(maxsize=None)
def _want(sw, sh, dw, dh, fmt, matrix, full):
    """The rule's letterboxed codes of ``_frame``: computed once, shared by the tests, never written to."""
    c = LB.letterbox10(_frame(sw, sh, fmt), dw, dh, fmt, matrix, bool(full))
    c.setflags(write=False)
    return c


def _letterbox(p, planes, dw, dh, matrix, full, guard=0, expect=0):
    """hdrtv_letterbox_ycbcr10 into a poisoned device buffer with ``guard`` canary words either side (destination at an odd word)."""
    import torch
    n = dh * dw * 3
    dst = torch.full((n + 2 * guard + 1,), 0xA5A5, dtype=torch.uint16, device="cuda")
    o = guard + 1 if guard else 0
    rc = p._lib.hdrtv_letterbox_ycbcr10(p._ctx, _stream(), *planes.args(), matrix, full, planes.h, planes.w, dst.data_ptr() + 2 * o, dh, dw)
    assert rc == expect, (rc, p._lib.hdrtv_last_error(p._ctx))
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    if guard:
        assert (host[:o] == 0xA5A5).all() and (host[o + n:] == 0xA5A5).all()
    return host[o:o + n].reshape(dh, dw, 3)


@pytest.fixture(scope="module")
def proc(golden_dir):
    p = _proc(golden_dir)
    yield p
    p.close()


# ---- 1. the codes, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.PIX_FMTS)
@pytest.mark.parametrize("sw,sh,dw,dh,mode", CASES)
def test_device_codes_equal_the_rule(proc, sw, sh, dw, dh, mode, fmt):
    assert LB.mode_of(sw, sh, dw, dh) == mode
    m, full = FMT_PAIR[fmt]
    planes = Planes(_frame(sw, sh, fmt), fmt)
    got = _letterbox(proc, planes, dw, dh, m, full)
    want = _want(sw, sh, dw, dh, fmt, m, full)
    assert got.max() <= 1023
    assert np.array_equal(got, want), (mode, fmt, int((got != want).any(axis=2).sum()))
    assert planes.unchanged()


def test_device_codes_bt601_once(proc):
    for sw, sh, dw, dh, _ in (CASES[4], CASES[9]):           # a fractional shrink and a cubic enlargement
        planes = Planes(_frame(sw, sh, "yuv420p10le"), "yuv420p10le")
        assert np.array_equal(_letterbox(proc, planes, dw, dh, 601, 1), _want(sw, sh, dw, dh, "yuv420p10le", 601, 1))


@pytest.mark.parametrize("fmt", R.PIX_FMTS)
def test_device_codes_offset_planes_padded_pitches_and_guard_words(proc, fmt):
    m, full = FMT_PAIR[fmt]
    for sw, sh, dw, dh, _ in (CASES[3], CASES[6], CASES[9]):  # ragged 2x2, fractional with an odd x0, cubic
        planes = Planes(_frame(sw, sh, fmt), fmt, off=2, extra=6, seed=3)
        assert planes.y % 4 == 2                                 # a plane base that is two-byte aligned and no more
        got = _letterbox(proc, planes, dw, dh, m, full, guard=64)
        assert np.array_equal(got, _want(sw, sh, dw, dh, fmt, m, full)), (fmt, sw, sh)
        assert planes.unchanged(), (fmt, sw, sh)


# ---- 2. the cap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.PIX_FMTS)
def test_a_5x_shrink_is_einval_and_leaves_the_destination(proc, fmt):
    from hdrtv_mi355x import lib as L
    planes = Planes(_frame(480, 40, fmt), fmt)
    got = _letterbox(proc, planes, 96, 8, 709, 0, guard=16, expect=L.EINVAL)
    assert (got == 0xA5A5).all()
    assert b"4x" in proc._lib.hdrtv_last_error(proc._ctx)


# ---- 3. the letterboxed preprocess -----------------------------------------------------------------------------------------------
def _preprocess(p, planes, matrix, full, h=DH, w=DW, expect=0, reserve=True):
    import torch
    dt = torch.float32 if p._fp32 else torch.float16
    rgb = torch.full((3, h, w), -7.0, dtype=dt, device="cuda")
    cond = torch.full((3, h // 4, w // 4), -7.0, dtype=dt, device="cuda")
    lib, ctx = p._lib, p._ctx
    if reserve:
        assert lib.hdrtv_reserve(ctx, h, w) == 0, lib.hdrtv_last_error(ctx)
    rc = lib.hdrtv_preprocess_ycbcr10_letterboxed(ctx, _stream(), *planes.args(), matrix, full, planes.h, planes.w, h, w,
                                                  rgb.data_ptr(), cond.data_ptr())
    assert rc == expect, (rc, lib.hdrtv_last_error(ctx))
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), cond.cpu().numpy()


def _check_preprocess(p, tensor_of, label):
    try:
        for sw, sh, dw, dh, kind in PRE_CASES:
            for fmt in R.PIX_FMTS:
                m, full = FMT_PAIR[fmt]
                want = tensor_of(_want(sw, sh, dw, dh, fmt, m, full))
                planes = Planes(_frame(sw, sh, fmt), fmt, off=2, extra=2)
                for mode in (0, 1, 2):
                    assert p._lib.hdrtv_set_cond_mode(p._ctx, mode) == 0
                    t, c = _preprocess(p, planes, m, full)
                    assert t.dtype == want.dtype and _same_bits(t, want), (kind, fmt, mode)
                    ref = _cond_ref(want, mode)                              # the oracle's map of that tensor
                    err = float(np.abs(c.astype(np.float32) - ref).max())    # every pixel of the map
                    print(f"{label} {fmt} {sw}x{sh} -> {dw}x{dh} ({kind}) mode {mode}: |cond - oracle|max = {err:.3e}")
                    assert c.shape == ref.shape and err <= COND_TOL, (kind, fmt, mode, err)
                assert planes.unchanged()
    finally:
        assert p._lib.hdrtv_set_cond_mode(p._ctx, 0) == 0


def test_letterboxed_preprocess_fp16_tensor_is_the_rule_and_cond_is_the_oracles(proc):
    _check_preprocess(proc, R.tensor_f16, "fp16")


def test_letterboxed_preprocess_fp32_tensor_exact_and_cond_within_the_bound(golden_dir):
    p = _proc(golden_dir, precision="fp32")
    try:
        _check_preprocess(p, R.tensor_f32, "fp32")
    finally:
        p.close()


def test_equal_sizes_give_the_bytes_of_preprocess_ycbcr10(proc):
    import torch
    lib, ctx = proc._lib, proc._ctx
    try:
        for fmt in R.PIX_FMTS:
            m, full = FMT_PAIR[fmt]
            f = _frame(DW, DH, fmt)
            kw = dict(pix_fmt=fmt, matrix=m, full_range=bool(full))
            t0, c0 = (x.cpu().numpy().copy() for x in proc.preprocess_ycbcr10(f, **kw))
            t1, c1 = (x.cpu().numpy().copy() for x in proc.preprocess_ycbcr10_letterboxed(f, DW, DH, **kw))
            assert _same_bits(t0, t1) and _same_bits(c0, c1), fmt
            # the C entry point itself at equal sizes (a COPY without bars), against hdrtv_preprocess_ycbcr10, in every condition mode
            planes = Planes(f, fmt)
            for mode in (0, 1, 2):
                assert lib.hdrtv_set_cond_mode(ctx, mode) == 0
                assert lib.hdrtv_reserve(ctx, DH, DW) == 0
                rgb = torch.empty((3, DH, DW), dtype=torch.float16, device="cuda")
                cond = torch.empty((3, DH // 4, DW // 4), dtype=torch.float16, device="cuda")
                assert lib.hdrtv_preprocess_ycbcr10(ctx, _stream(), *planes.args(), m, full, DH, DW, rgb.data_ptr(), cond.data_ptr()) == 0
                torch.cuda.synchronize()
                t, c = _preprocess(proc, planes, m, full)
                assert _same_bits(t, rgb.cpu().numpy()), (fmt, mode)
                assert _same_bits(c, cond.cpu().numpy()), (fmt, mode)
    finally:
        assert lib.hdrtv_set_cond_mode(ctx, 0) == 0


# ---- 4. argument and reservation rules -------------------------------------------------------------------------------------------
def test_estate_before_reserve_and_einval_leave_the_destinations(golden_dir):
    import torch
    from hdrtv_mi355x import lib as L
    p = _proc(golden_dir)
    try:
        lib, ctx, st = p._lib, p._ctx, _stream()
        fmt = "yuv420p10le"
        planes = Planes(_frame(192, 128, fmt), fmt)
        t, c = _preprocess(p, planes, 709, 0, expect=L.ESTATE, reserve=False)          # nothing reserved yet
        assert (t == -7.0).all() and (c == -7.0).all()
        assert lib.hdrtv_reserve(ctx, DH, DW) == L.OK
        t, c = _preprocess(p, planes, 709, 0, h=128, w=192, expect=L.ESTATE, reserve=False)     # another size than the reserved one
        assert (t == -7.0).all() and (c == -7.0).all()
        rgb = torch.full((3, DH, DW), -3.0, dtype=torch.float16, device="cuda")
        cond = torch.full((3, DH // 4, DW // 4), -3.0, dtype=torch.float16, device="cuda")
        codes = torch.full((DH * DW * 3,), 0x5A5A, dtype=torch.uint16, device="cuda")
        a = planes.args()
        pre = lambda args, sh, sw, h, w, r, cc: lib.hdrtv_preprocess_ycbcr10_letterboxed(ctx, st, *args, 709, 0, sh, sw, h, w, r, cc)   # noqa: E731
        box = lambda args, sh, sw, d, dh, dw: lib.hdrtv_letterbox_ycbcr10(ctx, st, *args, 709, 0, sh, sw, d, dh, dw)                    # noqa: E731
        assert pre(a, 128, 192, DH, DW, None, cond.data_ptr()) == L.EINVAL
        assert pre(a, 128, 192, DH, DW, rgb.data_ptr(), None) == L.EINVAL
        assert pre((None,) + a[1:], 128, 192, DH, DW, rgb.data_ptr(), cond.data_ptr()) == L.EINVAL            # NULL luma plane
        assert pre(a, 128, 191, DH, DW, rgb.data_ptr(), cond.data_ptr()) == L.EINVAL                          # what ycc_check refuses
        assert pre(a, 0, 192, DH, DW, rgb.data_ptr(), cond.data_ptr()) == L.EINVAL
        assert pre(a, 128, 192, 0, DW, rgb.data_ptr(), cond.data_ptr()) == L.EINVAL
        assert pre(a, 128, 192, DH, -4, rgb.data_ptr(), cond.data_ptr()) == L.EINVAL
        assert box(a, 128, 192, None, DH, DW) == L.EINVAL
        assert box(a, 128, 192, codes.data_ptr(), 0, DW) == L.EINVAL
        assert box(a, 128, 192, codes.data_ptr(), DH, 0) == L.EINVAL
        assert box(a[:3] + (None,) + a[4:], 128, 192, codes.data_ptr(), DH, DW) == L.EINVAL                   # planar without dev_v
        assert box(a, 128, 192, codes.data_ptr(), 8, 96) == L.EINVAL                                          # 192x128 -> 12x8: 16x
        assert lib.hdrtv_preprocess_ycbcr10_letterboxed(ctx, st, *a, 700, 0, 128, 192, DH, DW, rgb.data_ptr(), cond.data_ptr()) == L.EINVAL
        wide = Planes(_frame(480, 40, fmt), fmt)
        assert lib.hdrtv_reserve(ctx, 8, 96) == L.OK
        small_t = torch.full((3, 8, 96), -3.0, dtype=torch.float16, device="cuda")
        small_c = torch.full((3, 2, 24), -3.0, dtype=torch.float16, device="cuda")
        assert pre(wide.args(), 40, 480, 8, 96, small_t.data_ptr(), small_c.data_ptr()) == L.EINVAL          # 5x
        torch.cuda.synchronize()
        assert (rgb.cpu().numpy() == -3.0).all() and (cond.cpu().numpy() == -3.0).all() and (codes.cpu().numpy() == 0x5A5A).all()
        assert (small_t.cpu().numpy() == -3.0).all() and (small_c.cpu().numpy() == -3.0).all()
        assert lib.hdrtv_reserve(ctx, DH, DW) == L.OK
        assert pre(a, 128, 192, DH, DW, rgb.data_ptr(), cond.data_ptr()) == L.OK, lib.hdrtv_last_error(ctx)
        assert box(a, 128, 192, codes.data_ptr(), DH, DW) == L.OK, lib.hdrtv_last_error(ctx)
        torch.cuda.synchronize()
        assert (rgb.cpu().numpy() != -3.0).all() and (cond.cpu().numpy() != -3.0).all() and (codes.cpu().numpy() != 0x5A5A).all()
    finally:
        p.close()


# ---- 5. the surfaces -------------------------------------------------------------------------------------------------------------
def test_processor_method_equals_the_rule(proc):
    for sw, sh, dw, dh, kind in PRE_CASES:
        fmt = "p010le"
        m, full = FMT_PAIR[fmt]
        t, _ = proc.preprocess_ycbcr10_letterboxed(_frame(sw, sh, fmt), dw, dh, pix_fmt=fmt, matrix=m, full_range=bool(full))
        assert _same_bits(t.cpu().numpy()[0], R.tensor_f16(_want(sw, sh, dw, dh, fmt, m, full))), kind


def test_playback_src_size_yuv422p10le_clip_into_rgb48le_sink(golden_dir, tmp_path, capsys):
    """End to end: ``playback --src-size 192x128 --size 96x64`` reads a three-frame yuv422p10le rawvideo clip at 192x128, the worker
    letterboxes it on the device at ten bits, and the rgb48le sink receives the bytes of the direct calls."""
    from hdrtv_mi355x import playback as P
    wdir = tmp_path / "weights" / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    sw, sh, n, fmt = 192, 128, 3, "yuv422p10le"
    frames = [R.random_frame(sh, sw, seed=90 + i, pix_fmt=fmt, noisy_pad=True) for i in range(n)]
    (tmp_path / "clip.yuv").write_bytes(b"".join(f.astype("<u2").tobytes() for f in frames))
    p = _proc(golden_dir, use_hg=True, hg_weights="seeded:1234")
    want = b""
    for f in frames:
        out, _ = p.infer(p.preprocess_ycbcr10_letterboxed(f, DW, DH, pix_fmt=fmt, matrix=2020, full_range=True))
        want += _rgb48_of(p, out, DH, DW).tobytes()
    p.close()
    rc = P.main(["--weights-dir", str(tmp_path / "weights"), "--hg-weights", "seeded:1234", "--input", str(tmp_path / "clip.yuv"),
                 "--pix-fmt", fmt, "--yuv-matrix", "2020", "--yuv-range", "full", "--src-size", f"{sw}x{sh}", "--size", f"{DW}x{DH}",
                 "--frames", str(n), "--max-throughput", "--out", str(tmp_path / "out.rgb")])
    assert rc == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["frames_processed"] == n and res["sink_frames"] == n and res["src_res"] == f"{sw}x{sh}"
    got = (tmp_path / "out.rgb").read_bytes()
    assert len(got) == n * DH * DW * 6 and got == want
