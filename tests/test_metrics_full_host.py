"""The numpy rule of the full-reference metrics (tests/metrics_full_ref.py; include/hdrtv_mi355x.h R1 .. R6) against known answers,
and its measured distance from the reference's literal text, which takes float32 np.mean / np.std where the rule takes exact
histograms.  No GPU.

Measured distance over the evaluation pairs of tests/test_gpu_metrics_full.py (``literal_distance`` below; numpy 2.2.6 on x86-64):
the largest difference is 3.39e-5 dB in psnr_norm_db, 2.17e-7 in sssim_norm and 8.18e-5 in delta_e_itp_norm; 0.160 % of the
normalised codes differ (share 1.595e-3), each by one code.  The test asserts twice the measured values."""
import numpy as np
import pytest

import metrics_full_ref as R


# ------------------------------------------------------------------------------------------------------- area reduction
@pytest.mark.parametrize("hw,nhw", [((8, 12), (4, 6)), ((9, 12), (3, 4)), ((11, 13), (4, 5)), ((10, 12), (5, 5)), ((32, 64), (2, 4))])
def test_constant_frame_stays_constant_through_every_area_path(hw, nhw):
    for v in (0, 1, 777, 40000, 65535):                      # 65535 saturates and does not wrap
        src = np.full((*hw, 3), v, np.uint16)
        out = R.resize_area16(src, nhw[1], nhw[0])
        assert out.dtype == np.uint16 and out.shape == (*nhw, 3) and (out == v).all(), (hw, nhw, v, np.unique(out))


def test_area_2x2_and_3x3_known_answers():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 65536, (6, 8, 3), dtype=np.uint16)
    want = (src.astype(np.int64).reshape(3, 2, 4, 2, 3).sum(axis=(1, 3)) + 2) >> 2
    assert R.area_path(6, 8, 3, 4) == "2x2" and (R.resize_area16(src, 4, 3) == want).all()
    # a 3x3 block by hand: sum 45 -> 5; sum 9 * 65535 -> 65535; sum 65535 + 8 * 65534 = 589807 -> 65534.11 -> 65534;
    # sum 5 -> 0.5555 -> 1; sum 4 -> 0.4444 -> 0
    blocks = [np.arange(1, 10), np.full(9, 65535), np.array([65535] + [65534] * 8), np.array([5] + [0] * 8), np.array([4] + [0] * 8)]
    src = np.concatenate([np.repeat(b.reshape(3, 3, 1), 3, axis=2) for b in blocks], axis=1).astype(np.uint16)
    assert R.area_path(3, 15, 1, 5) == "int"
    assert R.resize_area16(src, 5, 1)[0, :, 0].tolist() == [5, 65535, 65534, 1, 0]


def test_area_table_path_weights_sum_to_one_and_match_a_float64_mean():
    rng = np.random.default_rng(2)
    src = rng.integers(0, 65536, (57, 83, 3), dtype=np.uint16)
    out = R.resize_area16(src, 24, 16)
    # against the exact area average in float64: the float32 table path stays within one code of it
    def w(n, m):
        a = np.zeros((m, n))
        for d in range(m):
            lo, hi = d * n / m, (d + 1) * n / m
            for s in range(n):
                a[d, s] = max(0.0, min(hi, s + 1) - max(lo, s)) / (n / m)
        return a
    exact = np.einsum("ys,xt,stc->yxc", w(57, 16), w(83, 24), src.astype(np.float64))
    assert np.abs(out.astype(np.float64) - exact).max() <= 1.0


def test_gpu_shapes_take_the_paths_they_are_listed_for():
    sizes = {}
    for h, w, max_side, bars, path in R.GPU_SHAPES:
        ch = h - 2 * bars
        nh, nw = R.eval_size(ch, w, max_side)
        assert R.area_path(ch, w, nh, nw) == path, (h, w, max_side, bars)
        sizes[(h, w)] = (nh, nw)
    assert sizes[(57, 83)] == (16, 24) and sizes[(51, 96)] == (26, 48) and sizes[(32, 512)] == (2, 32) and sizes[(64, 96)] == (32, 48)
    assert sizes[(96, 144)] == (32, 48) and sizes[(72, 96)] == (26, 48) and sizes[(75, 99)] == (22, 40)      # after the 10-row bars
    assert R.eval_size(1080, 1920) == (288, 512) and R.eval_size(2160, 3840) == (288, 512) and R.eval_size(288, 512) == (288, 512)
    with pytest.raises(ValueError):
        R.resize_area16(np.zeros((4, 34, 3), np.uint16), 2, 2)                  # 17x


# --------------------------------------------------------------------------------------------------------------- bounds
def _framed(h, w, top=0, bottom=0, left=0, right=0, seed=0):
    f = np.random.default_rng(seed).integers(2000, 60000, (h, w, 3), dtype=np.uint16)
    f[:top] = 0
    f[h - bottom:] = 0
    f[:, :left] = 0
    f[:, w - right:] = 0
    return f


def test_bounds_cases():
    h, w = 60, 80
    a, b = _framed(h, w, seed=1), _framed(h, w, seed=2)
    assert R.crop_rect(a, b) == ((0, h, 0, w), False)                                            # no bars
    a, b = _framed(h, w, 10, 10, seed=1), _framed(h, w, 12, 9, 0, 3, seed=2)
    assert R.crop_rect(a, b) == ((12, 50, 0, 77), True)                                          # bars in both: the intersection
    a, b = _framed(h, w, 10, 10, seed=1), _framed(h, w, seed=2)
    assert R.crop_rect(a, b) == ((10, 50, 0, w), True)                                           # bars in one frame only
    assert R.crop_rect(_framed(h, w, 7, 7, seed=1), _framed(h, w, 7, 7, seed=2)) == ((0, h, 0, w), False)      # 7 px: not cropped
    assert R.crop_rect(_framed(h, w, 8, 0, seed=1), _framed(h, w, 8, 0, seed=2)) == ((8, h, 0, w), True)       # 8 px: cropped
    z = np.zeros((h, w, 3), np.uint16)
    assert R.bounds_from_counts(*R.border_counts(z)) is None and R.crop_rect(z, z) == ((0, h, 0, w), False)    # all black: none
    assert R.crop_rect(z, _framed(h, w, 10, 10, seed=2)) == ((10, 50, 0, w), True)               # one "none": the other's bounds
    # the threshold: 131 is black, 132 is signal; a row needs max(4, round(0.01 * W)) signal pixels
    f = np.zeros((h, w, 3), np.uint16)
    f[20:40, 10:70, 1] = 131
    assert R.bounds_from_counts(*R.border_counts(f)) is None
    f[20:40, 10:70, 1] = 132
    assert R.bounds_from_counts(*R.border_counts(f)) == (20, 40, 10, 70)
    f[5, 0:3, 0] = 500                                                                           # three pixels: below the row minimum of 4
    assert R.bounds_from_counts(*R.border_counts(f)) == (20, 40, 10, 70)
    rec = R.counts_record(f, z)
    assert rec.shape == (2, h + w) and rec.dtype == np.uint32 and rec[0, 25] == 60 and rec[0, 5] == 3 and rec[0, h + 10] == 20 and not rec[1].any()


# ----------------------------------------------------------------------------------------------------------- statistics
def test_histogram_statistics_equal_float64_mean_and_std():
    pred, ref = R.ramp_pair(57, 83, 5)
    v = R.abs_of_code(1000.0).astype(np.float64)
    for frame in (pred, ref):
        h = R.channel_hist(frame)
        for c in range(3):
            codes = frame[:, :, c].astype(np.float64)
            for x, vals in ((np.arange(65536, dtype=np.float64), codes), (v, v[frame[:, :, c]])):
                mean, std = R.hist_mean_std(h[c], x)
                assert abs(mean - np.mean(vals)) <= 1e-12 * abs(np.mean(vals)) and abs(std - np.std(vals)) <= 1e-12 * np.std(vals)


def test_gain_is_one_on_a_flat_prediction_and_identity_on_equal_frames():
    _, ref = R.ramp_pair(24, 40, 3)
    flat = np.full_like(ref, 12345)
    g = R.grade_match(flat, ref)
    assert (g[0:3] == 1).all() and (g[6:9] == 1).all()
    for c in range(3):                                        # bias = mean_ref - mean_pred
        assert g[3 + c] == np.float32(np.mean(ref[:, :, c].astype(np.float64)) - 12345.0)
    g = R.grade_match(ref, ref)
    assert (g[[0, 1, 2, 6, 7, 8]] == 1).all() and (g[[3, 4, 5, 9, 10, 11]] == 0).all()
    assert (R.normalised_codes(ref, g) == ref).all()
    m = R.full_reference(ref, ref, max_side=512)
    assert m["psnr_db"] == 99.0 and m["psnr_norm_db"] == 99.0 and abs(m["sssim_norm"] - 1) < 1e-6 and abs(m["delta_e_itp_norm"] - 720e-6) < 1e-8


def test_normalised_codes_truncate_and_clip():
    p = np.array([[[0, 100, 65535]]], np.uint16)
    g = np.array([1.5, 0.999, 2.0, -10.0, 0.9, 0.0, 1, 1, 1, 0, 0, 0], np.float32)
    # 0 * 1.5 - 10 -> clipped to 0; 100 * 0.999 + 0.9 = 100.8 -> 100 (truncated, not rounded); 65535 * 2 -> clipped to 65535
    assert R.normalised_codes(p, g)[0, 0].tolist() == [0, 100, 65535]


def test_chain_note_rect_and_live_path():
    pred, ref = R.ramp_pair(72, 96, 72, bars=10)
    m = R.full_reference(pred, ref, max_side=48)
    assert m["crop_rect"] == (10, 62, 0, 96) and m["eval_size"] == (26, 48) and m["obj_note"].endswith("; shared black borders cropped)")
    live = R.full_reference(pred, ref, max_side=48, crop=False, normalized=False)
    assert live["crop_rect"] == (0, 72, 0, 96) and live["eval_size"] == (36, 48) and live["psnr_norm_db"] is None
    assert live["obj_note"].endswith("normalized pre-PQ)") and set(live) == set(m)


# ----------------------------------------------------------------------------- distance from the reference's literal text
# measured with literal_distance(), see the module docstring; the test's bound is twice these
MEASURED = {"psnr_norm_db": 3.39e-5, "sssim_norm": 2.17e-7, "delta_e_itp_norm": 8.18e-5, "share": 1.596e-3, "step": 1}


def literal_distance():
    """Over the evaluation pairs of the GPU test: the largest |rule - literal| of the three normalised metrics, the share of
    normalised codes that differ and the largest step between them."""
    worst = {"psnr_norm_db": 0.0, "sssim_norm": 0.0, "delta_e_itp_norm": 0.0}
    differ = total = step = 0
    for h, w, max_side, bars, _ in R.GPU_SHAPES:
        pred, ref = R.ramp_pair(h, w, h, bars=bars)
        p, q, _, _ = R.evaluation_pair(pred, ref, max_side)
        g, gl = R.grade_match(p, q), R.grade_match_literal(p, q)
        a, b = R.normalised_metrics(p, q, g), R.normalised_metrics(p, q, gl)
        for k, x, y in zip(worst, a, b):
            worst[k] = max(worst[k], abs(x - y))
        d = np.abs(R.normalised_codes(p, g).astype(np.int64) - R.normalised_codes(p, gl).astype(np.int64))
        differ, total, step = differ + int(np.count_nonzero(d)), total + d.size, max(step, int(d.max()))
    return worst, differ / total, step


def test_distance_from_the_literal_float32_statistics():
    worst, share, step = literal_distance()
    print("   literal distance:", worst, "share of codes", share, "largest step", step)
    # twice the measured values of the module docstring (the margin: numpy's summation order may change between versions)
    assert worst["psnr_norm_db"] <= 2 * MEASURED["psnr_norm_db"]
    assert worst["sssim_norm"] <= 2 * MEASURED["sssim_norm"]
    assert worst["delta_e_itp_norm"] <= 2 * MEASURED["delta_e_itp_norm"]
    assert share <= 2 * MEASURED["share"] and step <= 2 * MEASURED["step"]
