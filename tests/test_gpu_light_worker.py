"""HDR10 content light level through the worker on a real MI355X: every delivered frame carries the record of what the sink
received (``.light``), ``worker.content_light`` accumulates MaxCLL / MaxFALL from them, for RGB48 and Y'CbCr output, scaled output
and a measuring rectangle; with the feature off nothing changes.  96 x 64 frames without HG, as tests/test_gpu_worker.py uses."""
import os
import threading

import numpy as np
import pytest

import lightlevel_ref as R

pytestmark = pytest.mark.gpu

N = 4
PW, PH = 96, 64


@pytest.fixture(scope="module")
def weights_dir(golden_dir, tmp_path_factory):
    root = tmp_path_factory.mktemp("light_weights")
    (root / "original").mkdir()
    os.symlink(os.path.join(golden_dir, "hr_weights.hdrw"), root / "original" / "HR.hdrw")
    return str(root)


@pytest.fixture(scope="module")
def frames():
    from hdrtv_mi355x import weights as W
    return [W.synthetic_frame(PH, PW, seed=70 + i, kind="noise" if i % 2 else "gradient") for i in range(N)]


def _run(weights_dir, frames, **kw):
    """The frames through a worker and a collecting sink -> (delivered frames, their .light, the worker's content_light)."""
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    w = HeadlessPipelineWorker(weights_dir, use_hg=False, proc_w=PW, proc_h=PH, **kw)
    assert w._load_model("FP16") is True
    got, light, done = [], [], threading.Event()

    def sink(payload):
        light.append(payload.light)
        got.append(payload.numpy().copy())
        payload.release()
        if len(got) == len(frames):
            done.set()

    w._start_hdr_feeder(sink)
    for i, f in enumerate(frames):
        w._process_frame(frame=f, frame_idx=i, mpv_w=True)
    assert done.wait(20.0)
    w._stop_hdr_feeder()
    cl = w.content_light
    w.close()
    return got, light, cl


@pytest.fixture(scope="module")
def rgb_run(weights_dir, frames):
    return _run(weights_dir, frames, light_stats=True)


def _check_accumulator(cl, records):
    from hdrtv_mi355x.lightlevel import ContentLightLevel
    want = ContentLightLevel()
    for r in records:
        want.update(r)
    assert cl is not None and cl.frames == len(records) == N
    assert cl.as_dict() == want.as_dict() and cl.max_cll > 0.0 and cl.max_fall > 0.0
    assert cl.x265_params() == want.x265_params()


def test_rgb48_frames_carry_their_record(rgb_run):
    got, light, cl = rgb_run
    assert len(got) == N
    for i in range(N):
        assert got[i].shape == (PH, PW, 3) and light[i] is not None and light[i].dtype == np.uint32
        assert np.array_equal(light[i], R.record(got[i])), i
    assert not np.array_equal(light[0], light[1])
    _check_accumulator(cl, [R.record(g) for g in got])


def test_feature_off_no_record_and_the_same_bytes(weights_dir, frames, rgb_run):
    got, light, cl = _run(weights_dir, frames)
    assert cl is None and all(v is None for v in light)
    for a, b in zip(got, rgb_run[0]):
        assert np.array_equal(a, b)


def test_yuv420p10le_records_equal_the_rgb48_run(weights_dir, frames, rgb_run):
    got, light, cl = _run(weights_dir, frames, light_stats=True, out_pix_fmt="yuv420p10le")
    assert got[0].shape == (PH * PW * 3 // 2,)
    for i in range(N):
        assert np.array_equal(light[i], rgb_run[1][i]), i
    assert cl.as_dict() == rgb_run[2].as_dict()
    # and measuring changes no delivered byte
    plain = _run(weights_dir, frames, out_pix_fmt="yuv420p10le")[0]
    for a, b in zip(got, plain):
        assert np.array_equal(a, b)


def test_scaled_output_is_measured_at_the_delivered_size(weights_dir, frames):
    ow, oh = 144, 96
    got, light, cl = _run(weights_dir, frames, light_stats=True, out_w=ow, out_h=oh)
    for i in range(N):
        assert got[i].shape == (oh, ow, 3)
        assert np.array_equal(light[i], R.record(got[i])), i
    _check_accumulator(cl, [R.record(g) for g in got])
    # Y'CbCr at the delivered size: the statistic reads the scaled RGB48 scratch, so the records are the scaled RGB48 run's
    _, light_y, cl_y = _run(weights_dir, frames, light_stats=True, out_w=ow, out_h=oh, out_pix_fmt="p010le")
    for i in range(N):
        assert np.array_equal(light_y[i], light[i]), i
    assert cl_y.as_dict() == cl.as_dict()


def test_light_rect_is_honoured(weights_dir, frames, rgb_run):
    from hdrtv_mi355x.worker import HeadlessPipelineWorker
    rect = (5, 8, 83, 48)                                         # odd x0, odd width, letterbox-like bars above and below
    got, light, cl = _run(weights_dir, frames, light_stats=True, light_rect=rect)
    for i in range(N):
        assert np.array_equal(got[i], rgb_run[0][i])
        assert np.array_equal(light[i], R.record(got[i], rect)) and light[i][4102] == 83 * 48
    _check_accumulator(cl, [R.record(g, rect) for g in got])
    with pytest.raises(ValueError):
        HeadlessPipelineWorker(weights_dir, use_hg=False, proc_w=PW, proc_h=PH, light_stats=True, light_rect=(90, 0, 10, 10))


def test_enqueue_frame_light_ptr_on_two_lanes(golden_dir, frames):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X

    def run(lanes):
        p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0, lanes=lanes)
        try:
            srcs = [torch.from_numpy(f).cuda() for f in frames]
            dsts = [torch.zeros((PH, PW, 3), dtype=torch.uint16, device="cuda") for _ in frames]
            recs = [torch.from_numpy(np.zeros(L.LIGHT_WORDS, dtype=np.uint32)).cuda() for _ in frames]
            torch.cuda.synchronize()
            for i in range(len(frames)):
                p.enqueue_frame(i % lanes, srcs[i].data_ptr(), PH, PW, dsts[i].data_ptr(), light_ptr=recs[i].data_ptr(),
                                light_rect=(1, 1, PW - 2, PH - 2) if i == 1 else None)
            torch.cuda.synchronize()
            return [d.cpu().numpy() for d in dsts], [r.cpu().numpy() for r in recs]
        finally:
            p.close()

    d1, r1 = run(1)
    d2, r2 = run(2)
    for i in range(len(frames)):
        assert np.array_equal(d1[i], d2[i]) and np.array_equal(r1[i], r2[i]), i
        assert np.array_equal(r1[i], R.record(d1[i], (1, 1, PW - 2, PH - 2) if i == 1 else None)), i
