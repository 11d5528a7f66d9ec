"""The checker of tests/test_gpu_le_layers.py checked itself (CPU, no device): tests/le_layer_ref.py's stage table is the network,
its rounding model stays inside its own bound, the frames of the GPU test meet the input condition, and deliberate mistakes of
the kind a kernel can make break the bound."""
import os

import numpy as np
import pytest

import le_layer_ref as R

GOLDEN_FRAMES = ("hr_64x96_noise_s0", "hr_60x100_noise_s2", "hr_52x76_gradient_s5", "hr_32x96_gradient_s1_taps")


@pytest.fixture(scope="module")
def packed(hr_state):
    return R.pack(hr_state)


_TAPS = {}


def golden_taps(golden_dir, packed, name):
    """Every tensor of the graph on a golden frame's AGCM output, as exact f16 values (what the device hands out as taps)."""
    if name not in _TAPS:
        agcm = R.f16(R.as_t(np.load(os.path.join(golden_dir, name + ".npz"))["agcm_out"]))
        _TAPS[name] = R.taps_from_graph(R.full_graph(packed, agcm))
    return _TAPS[name]


def all_checks():
    """The per-layer form's checks and the composites of the default form (row kernels on), each once."""
    seen, out = set(), []
    for prof in (R.per_layer_profile(), R.fused_profile()):
        for c in R.plan(prof):
            if c.name not in seen:
                seen.add(c.name)
                out.append(c)
    return out


def test_the_stage_table_is_the_network(golden_dir, hr_state):
    """All stages assembled, in float64 on the unrounded checkpoint, are oracle.hdrtvnet_oracle.le (fp32) within 1e-5 -- at the
    output and at every tap the oracle has."""
    from oracle import hdrtvnet_oracle as O
    agcm = np.load(os.path.join(golden_dir, "hr_64x96_noise_s0.npz"))["agcm_out"]
    taps = {}
    want = O.le(hr_state, agcm, taps)
    env = R.full_graph(R.pack(hr_state, rounded=False), R.as_t(agcm))
    assert float((env["out"] - R.as_t(want)).abs().max()) <= 1e-5
    relu = lambda a: np.maximum(a, 0)
    same = {"cond": taps["LE.cond_first"], "cond1": taps["LE.CondNet1"], "cond2": taps["LE.CondNet2"], "cond3": taps["LE.CondNet3"],
            "cond4": taps["LE.CondNet4"], "f0a": relu(taps["LE.conv_first"]), "fea0": relu(taps["LE.HR_conv1"]),
            "fea1a": relu(taps["LE.down_conv1"]), "fea1": taps["LE.recon_trunk1"], "fea2a": relu(taps["LE.down_conv2"]),
            "fea2": taps["LE.recon_trunk2"], "fea3": relu(taps["LE.down_conv3"]), "t4": taps["LE.recon_trunk4"],
            "t5": taps["LE.recon_trunk5"], "t3y": taps["LE.recon_trunk3"] + relu(taps["LE.down_conv3"])}
    for k, a in same.items():
        assert float((env[k] - R.as_t(a)).abs().max()) <= 1e-5, k
    # every launch of the table is part of a check in both forms, and a launch nobody claims is an error
    for prof in (R.per_layer_profile(), R.fused_profile(), R.fused_profile(head=False, blocks=(), tail=False)):
        covered = {s.name for c in R.plan(prof) for s in c.stages}
        assert covered == {s.name for s in R.STAGES}
    with pytest.raises(AssertionError):
        R.plan(R.per_layer_profile() + [("LE.some_new_launch", "kernel")])


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_the_rounding_model_stays_inside_the_bound(golden_dir, packed, name):
    taps = golden_taps(golden_dir, packed, name)
    for c in all_checks():
        for t, r in R.evaluate(c, packed, taps).items():
            m = R.metrics(r, r["model"])
            assert m["violations"] == 0 and m["max_ratio"] <= 1.0, (c.name, t, m)
            ok, share, share_nz = R.input_condition(r)
            assert ok or c.extra, (c.name, t, share, share_nz)


@pytest.mark.parametrize("kind", ["noise", "gradient"])
@pytest.mark.parametrize("size", list(R.FRAMES))
def test_the_gpu_tests_frames_meet_the_input_condition(hr_state, packed, size, kind):
    """For every stage and size, on the CPU reference alone: at least 25 % of the output elements with |v| > 8 d (le_layer_ref.
    input_condition: its form for outputs a ReLU leaves mostly zero).  The inputs are the graph's own tensors on the oracle's
    AGCM output for the frame the GPU test uses."""
    from hdrtv_mi355x import weights as W
    from oracle import hdrtvnet_oracle as O
    f = W.synthetic_frame(*size, seed=R.FRAMES[size][kind == "gradient"], kind=kind)
    taps = R.taps_from_graph(R.full_graph(packed, R.f16(R.as_t(O.agcm(hr_state, *O.preprocess(f))))))
    for c in all_checks():
        if c.extra:
            continue
        for t, v in c.run(R.Bounded(), packed, taps).items():
            ok, share, share_nz = R.input_condition({"v": v[0], "d": v[1]})
            assert ok, (size, kind, c.name, t, share, share_nz)


# mutation -> the checks that must see it (frame hr_60x100_noise_s2: maps 30x50, 15x25, 8x13 -- up_conv1's 16x26 is cropped)
MUTATIONS = {
    "zero_tap": ("fea1a", "rt5a", "rt5b", "rt33a", "up1", "f0b", "out", "h2a", "x192"),
    "zero_weight": ("rt5a", "rt4a", "fea0", "fea2a"),
    "replicate_last_col": ("rt5a", "rt5b", "fea0", "up2", "out", "trunk"),
    "crop_from_end": ("up1",),
    "ps_swap": ("up1", "up2", "up3"),
    "slope02": ("x192", "h2a", "h2b", "trunk", "trunk1", "cond2", "rt5a", "fea0"),
    "no_plus1": ("fea0", "rt5a", "rt5b", "rt33a", "rt33b", "f0b"),
    "res_twice": ("rt5b", "rt4b", "rt33b", "up1", "up2", "up3", "out"),
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_a_mutated_model_violates_the_bound(golden_dir, packed, mut):
    """One 3x3 tap zeroed (and: the single largest weight), replicate instead of zero padding right of the last column, the
    _align_to crop taken from the bottom / right, PixelShuffle sub-positions (0, 1) and (1, 0) exchanged, LeakyReLU slope 0.2,
    the SFT's + 1 dropped, a residual added twice: each must leave the bound at many elements of every stage it applies to."""
    taps = golden_taps(golden_dir, packed, "hr_60x100_noise_s2")
    for stage in MUTATIONS[mut]:
        c = R.Check([stage])
        ref = R.evaluate(c, packed, taps)
        got = c.run(R.Rounded(mut), packed, taps)
        bad = sum(R.metrics(ref[t], got[t])["violations"] for t in c.outs)
        print(f"  {mut:20s} {stage:7s} violations {bad}")
        assert bad >= 8, (mut, stage, bad)


def test_an_fp16_accumulator_fails_the_precision_condition_only(golden_dir, packed):
    """A precision loss that is not a wrong result: the 3x3 conv's accumulator rounded to f16 after every 8 terms.  Behind an SFT
    layer it stays inside the hard bound (which has to allow for the SFT's own roundings, worst case) and falls outside
    mean|x - v| <= 2 mean|model - v|: the case the precision condition is there for.  At a plain conv launch the hard bound is one
    f16 rounding wide and the same mistake breaks it outright.  (Rounded every 32 terms, once per tap, it costs a factor 1.3 .. 1.5
    behind an SFT layer: printed -- that is below what the factor 2 can see.)"""
    taps = golden_taps(golden_dir, packed, "hr_60x100_noise_s2")
    for stage in ("rt5a", "rt4a", "rt33a", "fea0", "f0b"):
        c = R.Check([stage])
        ref = R.evaluate(c, packed, taps)
        for chunk in (32, 8):
            got = c.run(R.Rounded("acc16", chunk=chunk), packed, taps)
            m = R.metrics(ref[c.outs[0]], got[c.outs[0]])
            print(f"  acc16/{chunk:<2d} {stage:6s} max err/d {m['max_ratio']:.2f}  mean {m['mean_err']:.2e} = {m['mean_err'] / m['mean_model']:.2f} x model")
            assert m["violations"] == 0, (stage, chunk, m)
            assert chunk == 32 or m["mean_err"] > 2 * m["mean_model"], (stage, m)
    for stage in ("fea1a", "up2"):
        c = R.Check([stage])
        ref = R.evaluate(c, packed, taps)
        got = c.run(R.Rounded("acc16", chunk=8), packed, taps)
        assert R.metrics(ref[c.outs[0]], got[c.outs[0]])["violations"] > 0, stage
