"""The checker of tests/test_gpu_hg_layers.py checked itself (CPU, no device): tests/hg_layer_ref.py's stage table is the oracle's
head, its rounding model stays inside its own bound, the frames of the GPU test meet the input condition and have a mask that the
fp32 arithmetic cannot tip, and deliberate mistakes of the kind a kernel can make break the bound."""
import os
import re

import numpy as np
import pytest

import hg_layer_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))


_TAPS = {}


def frame_taps(hr_state, hg_state, size, kind):
    """(P, every tensor of the head as the device would hand it out) on the oracle's LE output of a frame of the GPU test."""
    if (size, kind) not in _TAPS:
        from hdrtv_mi355x import weights as W
        from oracle import hdrtvnet_oracle as O
        seed, r = H.FRAMES[size][kind == "gradient"]
        P = H.pack(hg_state, mask_r=r)
        base, _ = O.hr_forward(hr_state, *O.preprocess(W.synthetic_frame(*size, seed=seed, kind=kind)))
        _TAPS[(size, kind)] = (P, H.taps_from_graph(H.full_graph(P, H.f16(H.as_t(base)), H.HRounded())))
    return _TAPS[(size, kind)]


@pytest.mark.parametrize("name", ["hg_96x128_gradient_s3", "hg_80x112_gradient_s4"])
def test_the_stage_table_is_the_oracles_head(golden_dir, hg_state, name):
    """All stages assembled, in float64 without a rounding on the unrounded checkpoint, are oracle.hdrtvnet_oracle.hg_generator on
    the golden frame's LE output (reflect-padded and cropped as hg_composite does) within the golden test's own 1e-4 -- at the output
    and at every tap both have.  80 x 112 is padded to 96 x 128: the table's `prep` and the crop of `final` are the oracle's."""
    from oracle import hdrtvnet_oracle as O
    base = np.load(os.path.join(golden_dir, name + ".npz"))["tap:base"]
    _, h, w = base.shape
    mask = O.hg_mask(base)
    pad = ((0, 0), (0, -h % 32), (0, -w % 32))
    taps = {}
    want = O.hg_generator(hg_state, np.pad(base, pad, mode="reflect"), np.pad(mask, pad, mode="reflect"), taps)[:, :h, :w]
    env = H.full_graph(H.pack(hg_state, rounded=False), H.as_t(base))
    assert float((env["out"] - H.as_t(want)).abs().max()) <= 1e-4
    assert np.array_equal(env["mask"].numpy()[:, :h, :w], mask)
    for t in ("p1", "conv2", "conv3_2", "conv4_2", "conv5_2", "conv_code2", "conv6", "conv7", "conv8", "conv9"):
        assert float((env[t] - H.as_t(taps["hg." + t])).abs().max()) <= 1e-4, t
    # part + part2 + b10 is the oracle's conv10
    c10 = env["part"] + env["part2"] + H.as_t(hg_state["conv10.bias"])[:, None, None]
    assert float((c10 - H.as_t(taps["hg.conv10"])).abs().max()) <= 1e-4


def test_the_layer_table_is_the_librarys():
    """HG_LAYERS against hg_layers of csrc/api.h, field by field, and the plan: one check per launch, an unknown launch or a
    need-list launch is an error."""
    src = open(os.path.join(HERE, "..", "hdr-realtime-video-pipeline_amd", "csrc", "api.h")).read()
    body = src.split("inline constexpr HgLayer hg_layers[] = {", 1)[1].split("};", 1)[0]
    rows = re.findall(r'\{"(\w+)", (\d+), (\d+), (\d+), (\d), (\d+), ST_(\w+), ACT_(\w+), \d, "(\w+)", (nullptr|"\w+"), (nullptr|"\w+"), "([\w.]*)"', body)
    assert len(rows) == len(H.HG_LAYERS) == 18
    for got, (name, cout, cin, skip_cin, ks, ps, mode, relu, src_t, skip, dst, bn) in zip(rows, H.HG_LAYERS):
        want = (name, str(cout), str(cin), str(skip_cin), str(ks), str(ps), mode.upper(), "RELU" if relu else "NONE", src_t,
                f'"{skip}"' if skip else "nullptr", "nullptr" if name == "Up_conv5" else f'"{dst}"', bn)
        assert got == want, (got, want)
    checks = H.plan(H.dense_profile())
    assert [c.name for c in checks] == [s.name for s in H.STAGES] and len(checks) == 21          # hg_prep, conv1, the 18 table rows, hg_final
    with pytest.raises(AssertionError):
        H.plan(H.dense_profile() + [("hg.some_new_launch", "kernel")])
    with pytest.raises(AssertionError):
        H.plan(H.dense_profile() + [("hg_need", "hg_need")])


def test_no_listed_mask_r_leaves_a_pixel_to_the_fp32_arithmetic():
    """The number of pixels at which the device's mask may differ from the float64 one is 0 for every frame of the GPU test: no f16
    value in [0, 2] puts m within the fp32 evaluation's reach of the threshold.  The counter does count: with mask_r chosen so that
    m(0.5) is the threshold itself, the f16 value 0.5 is reported."""
    for size, frames in H.FRAMES.items():
        for _, r in frames:
            assert H.mask_uncertain_values(r) == 0, (size, r)
    assert H.mask_uncertain_values(0.75) == 0                   # the default
    r_hit = (0.5 - H.THRESH) / (1.0 - H.THRESH)                  # m(0.5) = thresh up to the rounding of r to fp32
    assert H.mask_uncertain_values(r_hit) >= 1


@pytest.mark.parametrize("kind", ["noise", "gradient"])
@pytest.mark.parametrize("size", list(H.FRAMES))
def test_model_inside_the_bound_and_input_condition_on_the_gpu_tests_frames(hr_state, hg_state, size, kind):
    """For every launch and frame of the GPU test, on the CPU alone: the rounding model stays inside the bound at every element, at
    least 25 % of every output stands clear of it (|v| > 8 d), and the oracle's mask at the listed mask_r is a 10 .. 90 % mixture."""
    P, taps = frame_taps(hr_state, hg_state, size, kind)
    frac = float(taps["mask"][:, :size[0], :size[1]].mean())
    assert 0.1 <= frac <= 0.9, frac
    low = 1.0
    for c in H.plan(H.dense_profile()):
        for t, r in H.evaluate(c, P, taps).items():
            m = H.metrics(r, r["model"])
            assert m["violations"] == 0 and m["max_ratio"] <= 1.0, (c.name, t, m)
            if t not in H.EXACT:
                ok, share, share_nz = H.input_condition(r)
                low = min(low, share)
                assert ok, (c.name, t, share, share_nz)
    print(f"  {size[0]}x{size[1]} {kind}: mask {frac:.3f}, smallest clear share {low:.2f}")


# mutation -> the launches that must see it (96 x 160 gradient, and 90 x 150 for the padding)
MUTATIONS = {
    "zero_tap": ((96, 160), ("conv1", "conv2", "conv3_1", "conv5_2", "Up_conv1", "Up_conv4", "Up_conv5")),
    "no_shift": ((96, 160), ("conv1", "conv2", "conv4_1", "conv_code2", "Up_conv2", "conv6", "conv9", "Up_conv5")),
    "pool_shift": ((96, 160), ("conv1", "conv3_1", "conv4_1", "conv5_1", "conv_code1")),
    "cat_swap": ((96, 160), ("conv6", "conv7", "conv8", "conv9")),
    "ps_swap": ((96, 160), ("Up_conv1", "Up_conv2", "Up_conv3", "Up_conv4", "Up_conv5")),
    "zero_pad": ((90, 150), ("prep",)),
    "lo_unscaled": ((96, 160), ("Up_conv5",)),
    "c10_f32": ((96, 160), ("final",)),
    "blend_all": ((96, 160), ("final",)),
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_a_mutated_model_violates_the_bound(hr_state, hg_state, mut):
    """A zeroed 3x3 tap, BatchNorm's shift (or the bias) dropped, the pool window shifted by one pixel, the skip concatenated in
    front of the input, PixelShuffle sub-positions exchanged, zero instead of reflect padding in prep, the lo half of the dot-product
    weights applied without its 2^-10, conv10 not rounded to f16 before conv_last, the blend applied at unmasked pixels: each leaves
    the hard bound on every launch it applies to.  Printed: the number of violations and the factor by which the worst one exceeds d.
    (The lo half DROPPED: test_a_dropped_lo_half_... below.)"""
    size, stages = MUTATIONS[mut]
    P, taps = frame_taps(hr_state, hg_state, size, "gradient")
    for stage in stages:
        c = H.Check([stage], by_name=H.BY_NAME, taps=H.TAPS)
        ref = H.evaluate(c, P, taps)
        got = c.run(H.HRounded(mut), P, taps)
        ms = [H.metrics(ref[t], got[t]) for t in c.outs]
        bad, worst = sum(m["violations"] for m in ms), max(m["max_ratio"] for m in ms)
        print(f"  {mut:11s} {stage:10s} violations {bad:7d}  worst err/d {worst:.3g}")
        assert bad >= 8, (mut, stage, bad)


def test_an_fp16_accumulator_fails_the_precision_condition(hr_state, hg_state):
    """A precision loss that is not a wrong result: the 3x3 conv's accumulator rounded to f16 after every 32 terms.  It misses
    mean|x - v| <= 2 mean|model - v| on every launch it applies to (the factor is printed)."""
    P, taps = frame_taps(hr_state, hg_state, (96, 160), "gradient")
    for stage in ("conv2", "conv3_1", "conv3_2", "Up_conv4", "Up_conv5"):
        c = H.Check([stage], by_name=H.BY_NAME, taps=H.TAPS)
        ref = H.evaluate(c, P, taps)
        got = c.run(H.HRounded("acc16", chunk=32), P, taps)
        t = c.outs[0]
        m = H.metrics(ref[t], got[t])
        print(f"  acc16/32 {stage:9s} max err/d {m['max_ratio']:.2f}  mean {m['mean_err']:.2e} = {m['mean_err'] / m['mean_model']:.2f} x model (condition: 2)")
        assert m["mean_err"] > 2 * m["mean_model"], (stage, m)


def test_a_dropped_lo_half_leaves_the_bound_where_the_operands_are_pinned(hr_state, hg_state):
    """conv_prw<ps_dot3> without the lo half of its weight pairs moves hg.part by sum (w - hi) x, about 2^-12 relative.  Up_conv5's
    f16 activations x never reach memory, so the bound has to allow each of them the other f16 neighbour wherever the worst-case
    fp32 accumulation error of the 3x3 conv (gamma_K over up to 576 nonzero products) reaches a rounding boundary -- on a frame's
    dense conv9 that is most of them, their 2^-11 steps outweigh the dropped term, and the mistake stays at err/d = 0.3 (printed,
    asserted < 1 so that nobody takes the frame cases for a test of it).  Where the operands ARE pinned the bound is the split term
    plus gamma_66 and the mistake leaves it: the same conv9 tap with two of every three rows and columns zeroed has at most 64
    nonzero products per output element, and HBounded.convbn counts them."""
    P, taps = frame_taps(hr_state, hg_state, (96, 160), "gradient")
    c = H.Check(["Up_conv5"], by_name=H.BY_NAME, taps=H.TAPS)
    m = H.metrics(H.evaluate(c, P, taps)["part"], c.run(H.HRounded("no_lo"), P, taps)["part"])
    print(f"  no_lo on the frame's conv9:   violations {m['violations']:6d} of {m['n']}  worst err/d {m['max_ratio']:.3g}")
    assert m["max_ratio"] < 1.0
    keep = np.zeros(tuple(taps["conv9"].shape[-2:]))
    keep[1::3, 1::3] = 1.0
    thin = dict(taps, conv9=taps["conv9"] * H.as_t(keep))
    ref = H.evaluate(c, P, thin)["part"]
    ok = H.metrics(ref, c.run(H.HRounded(), P, thin)["part"])
    m = H.metrics(ref, c.run(H.HRounded("no_lo"), P, thin)["part"])
    print(f"  no_lo on the thinned conv9:   violations {m['violations']:6d} of {m['n']}  worst err/d {m['max_ratio']:.3g}   (model: {ok['max_ratio']:.3f})")
    assert ok["violations"] == 0 and m["violations"] >= 0.25 * m["n"], m
