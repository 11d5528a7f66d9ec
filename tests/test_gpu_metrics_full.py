"""hdrtv_full_reference_metrics and its pieces on a real MI355X against the numpy rule of tests/metrics_full_ref.py
(include/hdrtv_mi355x.h R1 .. R6): border counts, 16-bit INTER_AREA, gains / biases and normalised codes bit for bit; the six
metrics within the tolerances tests/test_metrics.py applies to the same arithmetic (1e-3 dB, 2e-5 SSIM, 2e-3 relative dE-ITP)."""
import functools
import os

import numpy as np
import pytest

import metrics_full_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [s[:4] for s in R.GPU_SHAPES]


@pytest.fixture(scope="module")
def proc(golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def case(h, w, max_side, bars):
    """The frames of one shape and everything the rule says about them, computed once."""
    pred, ref = R.ramp_pair(h, w, h, bars=bars)
    ep, er, rect, cropped = R.evaluation_pair(pred, ref, max_side)
    return {"pred": pred, "ref": ref, "ep": ep, "er": er, "rect": rect, "cropped": cropped,
            "want": R.full_reference(pred, ref, max_side=max_side)}


def _close(got, want):
    for raw, norm in (("psnr_db", "psnr_norm_db"), ("sssim", "sssim_norm"), ("delta_e_itp", "delta_e_itp_norm")):
        for k in (raw, norm):
            print("  ", k, got[k], want[k])
    for k in ("psnr_db", "psnr_norm_db"):
        assert abs(got[k] - want[k]) < 1e-3, k
    for k in ("sssim", "sssim_norm"):
        assert abs(got[k] - want[k]) < 2e-5, k
    for k in ("delta_e_itp", "delta_e_itp_norm"):
        assert abs(got[k] - want[k]) < 2e-3 * max(1.0, want[k]), k


@pytest.mark.parametrize("h,w,max_side,bars", SHAPES)
def test_border_counts_are_exact(proc, h, w, max_side, bars):
    c = case(h, w, max_side, bars)
    got = proc.rgb48_border_counts(c["pred"], c["ref"]).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, R.counts_record(c["pred"], c["ref"]))


def test_border_counts_of_pillarboxed_and_black_frames(proc):
    pred, ref = R.ramp_pair(70, 300, 9)                        # more than one 256-column block, more than two 32-row blocks
    pred[:, :21] = 0
    ref[:, 290:] = 131                                         # one below the signal threshold
    z = np.zeros_like(ref)
    for a, b in ((pred, ref), (z, pred)):
        got = proc.rgb48_border_counts(a, b).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, R.counts_record(a, b))


@pytest.mark.parametrize("h,w,max_side,bars", SHAPES)
def test_area_reduce_is_exact(proc, h, w, max_side, bars):
    c = case(h, w, max_side, bars)
    nh, nw = c["ep"].shape[:2]
    for src, want in ((c["pred"], c["ep"]), (c["ref"], c["er"])):
        got = proc.rgb48_area_reduce(src, nw, nh, rect=c["rect"]).cpu().numpy()
        assert np.array_equal(got, want), (np.count_nonzero(got != want), np.abs(got.astype(int) - want.astype(int)).max())


def test_area_reduce_saturates_and_takes_two_strips(proc):
    src = np.full((33, 450, 3), 65535, np.uint16)             # 450 -> 150: three 64-column strips, the last one ragged; table rows
    src[:, ::7] = 65534
    got = proc.rgb48_area_reduce(src, 150, 16).cpu().numpy()
    assert np.array_equal(got, R.resize_area16(src, 150, 16)) and got.max() == 65535


def test_a_17x_shrink_is_refused(proc):
    from hdrtv_mi355x.lib import HdrtvError
    with pytest.raises(HdrtvError, match=r"\(-1\)"):
        proc.rgb48_area_reduce(np.zeros((4, 34, 3), np.uint16), 2, 2)
    pred, ref = R.ramp_pair(2, 600, 1)
    with pytest.raises(HdrtvError, match=r"\(-1\)"):          # 600 -> 32 is 18.75x
        proc.full_reference_metrics(pred, ref, max_side=32)
    with pytest.raises(HdrtvError, match=r"\(-1\)"):
        proc.full_reference_metrics(pred, ref, max_side=1)
    with pytest.raises(HdrtvError, match=r"\(-1\)"):
        proc.full_reference_metrics(pred, ref, peak_nits=0.0)


@pytest.mark.parametrize("h,w,max_side,bars", SHAPES)
def test_gains_and_biases_are_exact(proc, h, w, max_side, bars):
    c = case(h, w, max_side, bars)
    got = proc.rgb48_grade_match(c["ep"], c["er"])
    want = R.grade_match(c["ep"], c["er"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def test_gains_and_biases_of_a_flat_frame(proc):
    _, ref = R.ramp_pair(70, 300, 4)
    flat = np.full_like(ref, 12345)                            # one bin holds everything
    for a, b in ((flat, ref), (ref, flat), (flat, flat)):
        got, want = proc.rgb48_grade_match(a, b), R.grade_match(a, b)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert (proc.rgb48_grade_match(flat, ref)[[0, 1, 2, 6, 7, 8]] == 1).all()


@pytest.mark.parametrize("h,w,max_side,bars", SHAPES[:3])
def test_normalised_codes_are_exact(proc, h, w, max_side, bars):
    """Scoring the prediction with the grade match applied at load equals scoring a frame built from the rule's normalised codes:
    PSNR sums every squared code difference in float64, so one code off anywhere moves it."""
    c = case(h, w, max_side, bars)
    ep, er = c["ep"], c["er"]
    built = R.normalised_codes(ep, R.grade_match(ep, er))
    assert np.count_nonzero(built != ep) > ep.size // 2        # the grade match has something to do
    at_load = proc.full_reference_metrics(ep, er, max_side=4096, crop=False, normalized=True)
    from_rule = proc.full_reference_metrics(built, er, max_side=4096, crop=False, normalized=False)
    assert at_load["psnr_norm_db"] == from_rule["psnr_db"] and at_load["sssim_norm"] == from_rule["sssim"]
    off = built.copy()
    off[3, 5, 1] ^= 1                                          # the check can tell: one code off by one
    assert proc.full_reference_metrics(off, er, max_side=4096, crop=False, normalized=False)["psnr_db"] != from_rule["psnr_db"]


@pytest.mark.parametrize("h,w,max_side,bars", SHAPES)
def test_all_six_metrics(proc, h, w, max_side, bars):
    c = case(h, w, max_side, bars)
    got = proc.full_reference_metrics(c["pred"], c["ref"], max_side=max_side)
    assert got == proc.full_reference_metrics(c["pred"], c["ref"], max_side=max_side)           # fixed reduction order
    want = c["want"]
    assert got["crop_rect"] == want["crop_rect"] and got["eval_size"] == want["eval_size"] and got["obj_note"] == want["obj_note"]
    assert (got["crop_rect"] != (0, h, 0, w)) == bool(bars)
    _close(got, want)
    live = proc.full_reference_metrics(c["pred"], c["ref"], max_side=max_side, crop=False, normalized=False)
    assert live["psnr_norm_db"] is None and live["sssim_norm"] is None and live["delta_e_itp_norm"] is None
    assert live["crop_rect"] == (0, h, 0, w)
    if not bars:
        assert all(live[k] == got[k] for k in ("psnr_db", "sssim", "delta_e_itp"))


def test_identical_frames(proc):
    for h, w, max_side, bars in (SHAPES[2], SHAPES[5]):
        ref = case(h, w, max_side, bars)["ref"]
        m = proc.full_reference_metrics(ref, ref, max_side=max_side)
        assert m["psnr_db"] == 99.0 and m["psnr_norm_db"] == 99.0
        assert abs(m["sssim"] - 1.0) < 1e-6 and abs(m["sssim_norm"] - 1.0) < 1e-6
        assert abs(m["delta_e_itp"] - 720e-6) < 1e-8 and abs(m["delta_e_itp_norm"] - 720e-6) < 1e-8


def test_playback_reference_mode(golden_dir, tmp_path):
    import torch
    from hdrtv_mi355x import playback as P
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    from oracle import hdrtvnet_oracle as O
    from oracle import metrics_oracle as M
    wdir = tmp_path / "weights" / "original"
    wdir.mkdir(parents=True)
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), wdir / "HR.hdrw")
    w = HeadlessPipelineWorker(str(tmp_path / "weights"), use_hg=False, proc_w=96, proc_h=64)
    assert w._load_model("FP16")
    gt16 = R.ramp_pair(64, 96, 7)[1]
    gt_t = torch.from_numpy(R.unit_planes(gt16))

    class Gt:
        def __init__(self, frame):
            self.frame = frame

        def read(self):
            return True, self.frame

    def run(**kw):
        src = P.SyntheticSource(96, 64, fps=60.0, n_frames=3, pool=1, kind="gradient")
        pb = P.RealtimePlayback(w, src, sink=False, realtime=False, objective_every=1, **kw)
        pb.run()
        return pb.last_metrics, src

    m, src = run(gt_source=Gt(gt16), objective_mode="reference")
    frame = src._pool[0]                                       # pool=1: every frame of the run was this one
    prepared = w._process_frame(frame=frame, frame_idx=0, mpv_w=None)[2]
    out = prepared.float().cpu().numpy()[0]
    want = R.full_reference(O.post_rgb48(out), gt16, crop=False, normalized=False)
    assert m["objective_enabled"] is True
    assert abs(m["psnr_db"] - want["psnr_db"]) < 1e-3 and abs(m["sssim"] - want["sssim"]) < 2e-5
    assert abs(m["delta_e_itp"] - want["delta_e_itp"]) < 2e-3 * max(1.0, want["delta_e_itp"])
    # the default mode: the tensor against a unit-range tensor, as before
    m0, _ = run(gt_source=Gt(gt_t[None]))
    want0 = M.metrics(prepared.float().cpu().numpy()[0], gt_t.numpy())
    assert abs(m0["psnr_db"] - want0["psnr_db"]) < 1e-3 and abs(m0["sssim"] - want0["sssim"]) < 2e-5
    assert abs(m0["delta_e_itp"] - want0["delta_e_itp"]) < 2e-3 * max(1.0, want0["delta_e_itp"])
    assert m0["psnr_db"] != m["psnr_db"]
    with pytest.raises(ValueError):
        P.RealtimePlayback(w, src, objective_mode="codes")
    w.close()
