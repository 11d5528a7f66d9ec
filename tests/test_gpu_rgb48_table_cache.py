"""The table cache of the four RGB48 scaler families on a real MI355X: one context keeps the device tables of every family per
geometry (H, W, dH, dW) under one type, and each family must find only its own.

The yardstick is the composition, as in the families' own tests: what hdrtv_post_rgb48 writes at the processing size, then the
family's NumPy reference.  Equality is exact.  Sizes: 20x24 -> 30x36 is the smallest geometry every enlarging family accepts under
the same key (both axes enlarged, at most 2x) with 18 distinct geometries 20x24 -> (21 + i) x (25 + i) below 2x beside it."""
import os

import numpy as np
import pytest

import rgb48_down_ref as D
import rgb48_fsr_ref as F
import rgb48_scale_ref as S
import rgb48_ssimsr_ref as R

pytestmark = pytest.mark.gpu

H, W, DH, DW = 20, 24, 30, 36
SHARP = 0.2
WALK = [(21 + i, 25 + i) for i in range(18)] + [(21, 25)]        # past the limit of 16 geometries, then the first one again


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)        # one context, its caches empty
    yield p
    p.close()


def _source(h, w):
    import torch
    x = np.random.default_rng(100 * h + w).uniform(-0.25, 1.25, (3, h, w)).astype(np.float32)
    return torch.from_numpy(x).to("cuda").contiguous()


def _call(p, entry, t, dh, dw, *args):
    """The C entry point ``entry`` on the f32 tensor ``t`` -> u16 (dh, dw, 3) on the host."""
    import torch
    from hdrtv_mi355x import lib as L
    h, w = t.shape[-2:]
    o = torch.full((dh, dw, 3), 0xA5A5, dtype=torch.uint16, device=t.device)
    common = () if entry == "hdrtv_post_rgb48" else (0, 0.0)
    size = () if entry == "hdrtv_post_rgb48" else (dh, dw)
    p._chk(getattr(p._lib, entry)(p._ctx, p._stream(), t.data_ptr(), L.F32, h, w, *common, o.data_ptr(), *size, *args), entry)
    return o.cpu().numpy()


@pytest.fixture(scope="module")
def frame(proc):
    """(the source tensor, its unscaled codes)"""
    t = _source(H, W)
    return t, _call(proc, "hdrtv_post_rgb48", t, H, W)


# (what, entry point, the arguments behind dW, the reference on the unscaled codes)
KINDS = [
    ("lanczos", "hdrtv_post_rgb48_scaled", (), lambda c, dh, dw: S.scale(c, dh, dw)),
    ("fsr", "hdrtv_post_rgb48_fsr", (1, SHARP), lambda c, dh, dw: F.scale(c, dh, dw, SHARP)),
    ("spline36", "hdrtv_post_rgb48_ssimsr", (0,), lambda c, dh, dw: R.scale(c, dh, dw, ssim=False)),
    ("ssim_superres", "hdrtv_post_rgb48_ssimsr", (1,), lambda c, dh, dw: R.scale(c, dh, dw, ssim=True)),
]


def test_a_shared_key_hands_every_family_its_own_tables(proc, frame):
    t, codes = frame
    want = {what: ref(codes, DH, DW) for what, _, _, ref in KINDS}
    assert len({v.tobytes() for v in want.values()}) == len(KINDS)                 # the four results differ: a swap would show
    for what, entry, args, _ in KINDS + KINDS[::-1]:
        got = _call(proc, entry, t, DH, DW, *args)
        assert np.array_equal(got, want[what]), what
    # the same four numbers name a shrinking geometry when read the other way round
    big = _source(DH, DW)
    small = _call(proc, "hdrtv_post_rgb48_down", big, H, W, D.AUTO_ANTIRING, 1)
    assert np.array_equal(small, D.scale(_call(proc, "hdrtv_post_rgb48", big, DH, DW), H, W, a=D.AUTO_ANTIRING, ssim=True))


def test_eviction_frees_one_family_only(proc, frame):
    t, codes = frame
    ssimsr = _call(proc, "hdrtv_post_rgb48_ssimsr", t, DH, DW, 1)                   # its tables are cached from here on
    assert np.array_equal(ssimsr, R.scale(codes, DH, DW, ssim=True))
    for what, entry, args, ref in KINDS[:2]:
        want = {}
        for dh, dw in WALK:
            if (dh, dw) not in want:
                want[dh, dw] = ref(codes, dh, dw)
            assert np.array_equal(_call(proc, entry, t, dh, dw, *args), want[dh, dw]), (what, dh, dw)
        assert len(want) == 18
    assert np.array_equal(_call(proc, "hdrtv_post_rgb48_ssimsr", t, DH, DW, 1), ssimsr)
