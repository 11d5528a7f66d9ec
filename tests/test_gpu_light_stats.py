"""HDR10 content light level records on a real MI355X: hdrtv_light_stats (the model's tensor) and hdrtv_rgb48_light_stats (RGB48
codes already on the device), through ctypes.

The yardstick for the tensor entry point is tests/lightlevel_ref applied to the bytes the EXISTING entry points write for the same
tensor (hdrtv_post_rgb48, or hdrtv_post_pq_rgb48 for pq) -- those are pinned by the other GPU tests, so no quantiser is restated
here.  Equality is exact: every one of the 4104 words."""
import os

import numpy as np
import pytest

import lightlevel_ref as R

pytestmark = pytest.mark.gpu

PEAK = 1000.0
# (H, W).  A lane takes eight pixels, a workgroup 256 lanes: one pixel; a ragged group; an odd plane size (the f16 planes and the
# rows are not 16-byte aligned: the element-wise path throughout); rows of whole aligned groups; 5000 groups (20 workgroups, and
# many passes of a small grid).
SHAPES = [(1, 1), (2, 3), (37, 53), (64, 136), (40, 1000)]
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


def _input(h, w):
    """Seeded values in [-0.25, 1.25] (both clamps of the quantiser act), no NaN, with exact 0 and 1 among them."""
    x = np.random.default_rng(1000 * h + w).uniform(-0.25, 1.25, (3, h, w)).astype(np.float32)
    x[0, 0, 0], x[1, 0, -1], x[2, -1, -1], x[0, -1, 0] = 0.0, 1.0, 1.0, 0.0
    return x


def _rects(h, w):
    """The full frame, one pixel, an interior rectangle with odd x0, odd rw and y0 > 0 (where the frame has room), and one that
    touches the right and bottom edges."""
    out = [(0, 0, w, h), (w // 2, h // 2, 1, 1), (w // 3, h // 3, w - w // 3, h - h // 3)]
    if w >= 6 and h >= 4:
        rw = w - 4 if (w - 4) % 2 else w - 5
        out.append((3, 1, rw, h - 2))
    return out


def _codes(p, t, pq):
    """What the existing RGB48 entry points write for the tensor -> (device tensor, numpy)."""
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


def _new_record():
    import torch
    from hdrtv_mi355x import lib as L
    return torch.from_numpy(np.full(L.LIGHT_WORDS, SENTINEL, dtype=np.uint32)).cuda()


def _tensor_stats(p, t, pq, rect, rec=None):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    rec = _new_record() if rec is None else rec
    dt = L.F32 if t.dtype == torch.float32 else L.F16
    p._chk(p._lib.hdrtv_light_stats(p._ctx, p._stream(), t.data_ptr(), dt, h, w, pq, PEAK if pq else 0.0, *rect, rec.data_ptr()), "light_stats")
    return rec.cpu().numpy()


def _codes_stats(p, ptr, h, w, rect, rec=None):
    rec = _new_record() if rec is None else rec
    p._chk(p._lib.hdrtv_rgb48_light_stats(p._ctx, p._stream(), ptr, h, w, *rect, rec.data_ptr()), "rgb48_light_stats")
    return rec.cpu().numpy()


def _same(got, want, tag):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, tag + (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert int(got[:R.BINS].astype(np.int64).sum()) == int(got[4102]) and got[4103] == 0, tag


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "%dx%d" % v)
def test_tensor_entry_point_equals_the_rule_on_the_delivered_codes(proc, shape):
    import torch
    h, w = shape
    x = _input(h, w)
    for dtype in (torch.float32, torch.float16):
        t = torch.from_numpy(x).to("cuda", dtype).contiguous()
        for pq in (0, 1):
            _, codes = _codes(proc, t, pq)
            for rect in _rects(h, w):
                _same(_tensor_stats(proc, t, pq, rect), R.record(codes, rect), (str(dtype), pq, rect))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "%dx%d" % v)
def test_rgb48_entry_point_equals_the_rule(proc, shape):
    import torch
    h, w = shape
    a = np.random.default_rng(7 * h + w).integers(0, 65536, (h, w, 3), dtype=np.uint16)
    # at a 16-byte boundary (torch allocations are aligned far beyond that) and 2 bytes past one
    buf = torch.zeros(h * w * 3 + 1, dtype=torch.uint16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for off in (0, 1):
        buf[off:off + h * w * 3] = torch.from_numpy(a.reshape(-1)).cuda()
        for rect in _rects(h, w):
            _same(_codes_stats(proc, buf.data_ptr() + 2 * off, h, w, rect), R.record(a, rect), (off, rect))


def test_record_does_not_depend_on_the_grid(proc):
    """40 x 1000 is 5000 groups: one workgroup walks them in 20 passes, six workgroups in four, the default grid and the
    largest in one."""
    import torch
    h, w = 40, 1000
    t = torch.from_numpy(_input(h, w)).to("cuda", torch.float16).contiguous()
    codes_dev, codes = _codes(proc, t, 0)
    rect = (3, 1, 991, 38)
    want = R.record(codes, rect)
    default = proc.get_variant("light_wgs")
    try:
        for ncu, wgs in ((1, 1), (2, 3), (0, default), (0, 8)):
            proc.set_variant("force_ncu", ncu)
            proc.set_variant("light_wgs", wgs)
            _same(_tensor_stats(proc, t, 0, rect), want, ("tensor", ncu, wgs))
            _same(_codes_stats(proc, codes_dev.data_ptr(), h, w, rect), want, ("codes", ncu, wgs))
    finally:
        proc.set_variant("force_ncu", 0)
        proc.set_variant("light_wgs", default)


@pytest.mark.parametrize("level", [0.0, 1.0])
def test_constant_frames_every_lane_on_one_bin_and_a_sum_past_32_bits(proc, level):
    import torch
    h, w = 264, 256                                               # 67 584 pixels: 67 584 * 65 535 > 2^32
    code = int(level * 65535)
    for dtype in (torch.float16, torch.float32):
        t = torch.full((3, h, w), level, dtype=dtype, device="cuda")
        codes_dev, codes = _codes(proc, t, 0)
        assert (codes == code).all()
        want = R.record(codes)
        assert want[code >> 4] == h * w and (int(want[4100]) | (int(want[4101]) << 32)) == h * w * code
        assert level == 0.0 or want[4101] > 0
        _same(_tensor_stats(proc, t, 0, (0, 0, w, h)), want, (str(dtype), "tensor"))
        _same(_codes_stats(proc, codes_dev.data_ptr(), h, w, (0, 0, w, h)), want, (str(dtype), "codes"))
    # a flat frame whose width is not a multiple of 8 (the element-wise path) and a rectangle that cuts into groups
    t = torch.full((3, 50, 203), level, dtype=torch.float16, device="cuda")
    _, codes = _codes(proc, t, 0)
    for rect in ((0, 0, 203, 50), (5, 2, 191, 47)):
        _same(_tensor_stats(proc, t, 0, rect), R.record(codes, rect), ("ragged", rect))


def test_ramp_puts_both_ends_of_every_bin(proc):
    """Codes 16 b and 16 b + 15 for each of the 4096 bins, the maximum moving through the channels: every bin holds exactly
    two pixels, and an off-by-one in m >> 4 would move one of them."""
    import torch
    b = np.arange(4096)
    m = np.stack([16 * b, 16 * b + 15], axis=1).reshape(-1).astype(np.uint16)       # 8192 values
    a = np.zeros((8192, 3), dtype=np.uint16)
    ch = np.arange(8192) % 3
    a[np.arange(8192), ch] = m
    a[np.arange(8192), (ch + 1) % 3] = m // 2
    a = a.reshape(64, 128, 3)
    dev = torch.from_numpy(a).cuda()
    got = _codes_stats(proc, dev.data_ptr(), 64, 128, (0, 0, 128, 64))
    assert (got[:4096] == 2).all()
    _same(got, R.record(a), ("ramp",))
    assert got[4099] == 65535 and max(got[4096:4099]) == 65535


def test_maximum_in_a_different_channel_in_each_third(proc):
    import torch
    h, w = 30, 96
    x = np.full((3, h, w), 0.1, dtype=np.float32)
    x[0, :, :32], x[1, :, 32:64], x[2, :, 64:] = 0.9, 0.8, 0.7
    x[1, :, :32], x[2, :, 32:64], x[0, :, 64:] = 0.3, 0.25, 0.2
    t = torch.from_numpy(x).cuda()
    for pq in (0, 1):
        _, codes = _codes(proc, t, pq)
        want = R.record(codes)
        got = _tensor_stats(proc, t, pq, (0, 0, w, h))
        _same(got, want, ("thirds", pq))
        assert np.count_nonzero(got[:4096]) == 3 and (got[:4096][got[:4096] > 0] == h * 32).all()
        # each third alone: its own channel carries the maximum
        for k, x0 in enumerate((0, 32, 64)):
            part = _tensor_stats(proc, t, pq, (x0, 0, 32, h))
            _same(part, R.record(codes, (x0, 0, 32, h)), ("third", pq, k))
            assert part[4099] == part[4096 + k] == codes[0, x0, k]


def test_two_calls_agree_and_a_record_is_overwritten(proc):
    import torch
    h, w = 37, 53
    t1 = torch.from_numpy(_input(h, w)).cuda()
    t2 = torch.from_numpy(_input(h, w)[:, ::-1].copy() * 0.5).cuda()
    rect = (0, 0, w, h)
    a, b = _tensor_stats(proc, t1, 1, rect), _tensor_stats(proc, t1, 1, rect)
    assert np.array_equal(a, b)
    rec = _new_record()
    first = _tensor_stats(proc, t1, 0, rect, rec)
    second = _tensor_stats(proc, t2, 0, rect, rec)                # the same buffer: nothing of the first frame may remain
    _same(first, R.record(_codes(proc, t1, 0)[1]), ("first",))
    _same(second, R.record(_codes(proc, t2, 0)[1]), ("second",))
    assert not np.array_equal(first, second)
    third = _codes_stats(proc, _codes(proc, t1, 0)[0].data_ptr(), h, w, rect, rec)
    assert np.array_equal(third, first)


def test_processor_light_stats(proc):
    import torch
    h, w = 64, 136
    t = torch.from_numpy(_input(h, w)).to("cuda", torch.float16)[None]
    _, codes = _codes(proc, t[0], 0)
    rec = proc.light_stats(t)
    assert str(rec.dtype) == "torch.uint32" and rec.is_cuda and rec.numel() == R.WORDS
    _same(rec.cpu().numpy(), R.record(codes), ("light_stats",))
    _same(proc.light_stats(t, rect=(3, 1, 131, 60)).cpu().numpy(), R.record(codes, (3, 1, 131, 60)), ("light_stats rect",))


def test_bad_arguments_leave_the_record_untouched(proc):
    import torch
    from hdrtv_mi355x import lib as L
    h, w = 8, 16
    t = torch.zeros((3, h, w), dtype=torch.float16, device="cuda")
    c = torch.zeros((h, w, 3), dtype=torch.uint16, device="cuda")
    rec = _new_record()
    lib, ctx, st, rp = proc._lib, proc._ctx, proc._stream(), rec.data_ptr()
    full = (0, 0, w, h)
    bad_rects = [(0, 0, 0, h), (0, 0, w, 0), (0, 0, -1, h), (-1, 0, 4, 4), (0, -1, 4, 4), (1, 0, w, h), (0, 1, w, h), (w, 0, 1, 1),
                 (0, h, 1, 1), (2 ** 31 - 1, 0, 2, 1)]
    calls = [
        lambda: lib.hdrtv_light_stats(None, st, t.data_ptr(), L.F16, h, w, 0, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, None, L.F16, h, w, 0, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, 0, w, 0, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, h, -3, 0, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, h, w, 0, 0.0, *full, rp + 4),      # 4-byte aligned only
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), 2, h, w, 0, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), -1, h, w, 0, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, h, w, 1, 0.0, *full, rp),
        lambda: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, h, w, 1, -5.0, *full, rp),
        lambda: lib.hdrtv_rgb48_light_stats(None, st, c.data_ptr(), h, w, *full, rp),
        lambda: lib.hdrtv_rgb48_light_stats(ctx, st, None, h, w, *full, rp),
        lambda: lib.hdrtv_rgb48_light_stats(ctx, st, c.data_ptr(), 0, w, *full, rp),
        lambda: lib.hdrtv_rgb48_light_stats(ctx, st, c.data_ptr(), h, w, *full, rp + 4),
    ]
    for r in bad_rects:
        calls.append(lambda r=r: lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, h, w, 0, 0.0, *r, rp))
        calls.append(lambda r=r: lib.hdrtv_rgb48_light_stats(ctx, st, c.data_ptr(), h, w, *r, rp))
    for i, call in enumerate(calls):
        assert call() == L.EINVAL, i
    assert lib.hdrtv_light_stats(ctx, st, t.data_ptr(), L.F16, h, w, 0, 0.0, *full, None) == L.EINVAL
    assert lib.hdrtv_rgb48_light_stats(ctx, st, c.data_ptr(), h, w, *full, None) == L.EINVAL
    torch.cuda.synchronize()
    assert (rec.cpu().numpy() == SENTINEL).all()
    # and the buffer works afterwards
    got = _tensor_stats(proc, t, 0, full, rec)
    assert got[0] == h * w and got[4102] == h * w and got[4099] == 0
