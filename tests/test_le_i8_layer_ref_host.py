"""The checker of tests/test_gpu_le_i8_layers.py checked itself (CPU, no device): tests/le_i8_layer_ref.py's stage table is the
fake-quant network, its folded border-class shifts are the network's zero padding, its model stays inside its own bound and inside
the marked-element cap on the GPU test's frames, and deliberate mistakes of the kind an int8 kernel can make leave the bound."""
import os

import numpy as np
import pytest
import torch

import le_i8_layer_ref as Q
import le_layer_ref as R

TOL = 1e-5          # the fp32 noise of the oracle, as in the other host tests
NOISE = 4e-6        # ... and what of it a quantiser INSIDE a compared segment may see on its input: the oracle's fp32 convs are within
                    # 1.9e-6 of float64 at every element no code flip reaches (printed below; largest at 1/8 resolution); twice that
_C = {}


def recipe(golden_dir, tag, rounded=True):
    key = (tag, rounded)
    if key not in _C:
        from hdrtv_mi355x import weights as W
        from oracle import hdrtvnet_oracle as O
        raw = W.load_pack(os.path.join(golden_dir, Q.RECIPES[tag]))
        _C[key] = (Q.pack(raw, rounded), O.w8a8_state(raw))
    return _C[key]


def frame_taps(golden_dir, tag, size, kind):
    """The model's own tensors on the oracle's AGCM output for a frame of the GPU test: inputs of the kind the device hands out."""
    key = (tag, size, kind)
    if key not in _C:
        from hdrtv_mi355x import weights as W
        from oracle import hdrtvnet_oracle as O
        P, sd = recipe(golden_dir, tag)
        f = W.synthetic_frame(*size, seed=R.FRAMES[size][kind == "gradient"], kind=kind)
        agcm = R.f16(R.as_t(O.agcm(sd, *O.preprocess(f))))
        taps = Q.taps_from_graph(P, Q.full_graph(P, agcm, Q.Rounded8()))
        if tag == "full":
            taps["img32"] = Q.full_graph(P, agcm, Q.Rounded8(), no_c3q8=True)["img32"]
        _C.clear() if len(_C) > 6 else None          # keep the cache small: two recipes, a few frames
        _C[key] = taps
    return _C[key]


def all_checks(P, tag):
    checks = Q.plan(Q.per_layer_profile(P), P)
    if tag == "full":
        checks += [c for c in Q.plan(Q.per_layer_profile(P, True), P, True) if c.name in ("img32", "f0a")]
    return checks


# the stages between two tensors the oracle taps (oracle.hdrtvnet_oracle.le), each evaluated on the ORACLE's inputs: end to end these
# graphs are chaotic in the small (tests/test_gpu_int8_hr.py), stage by stage they are not
SEGMENTS = (["trunk"], ["trunk1"], ["c234", "c2a", "cond2"], ["c234", "h2a", "cond3"], ["c234", "h2b", "cond4"], ["f0a"], ["fea0"], ["fea1a"],
            ["rt1a", "rt1b"], ["fea2a"], ["rt2a", "rt2b"], ["fea3"], ["rt30a", "rt30b", "rt31a", "rt31b", "rt32a", "rt32b", "rt33a", "rt33b"],
            ["up1", "rt4a", "rt4b"], ["up2", "rt5a", "rt5b"], ["up3", "f0b", "out"])


# Segments in which the flip allowance reaches (nearly) every output, so that `err <= TOL + dd` alone says little there: three chained
# convs, two of them 3x3 / stride 2 with a fan-in of 576 codes each, from `cond` -- the oracle taps neither CondNet{3,4}.0's nor .2's
# output (c3a / c4a, h2a / h2b), so the segment cannot restart nearer to the output.  What holds these two layers pairs is the packer
# test below (CondNet4.4 among its layers) and the per-launch model-inside-bound test on every frame.
# `t3y`: the four ResBlocks of recon_trunk3 -- eight SFT + conv launches with 24 quantisers in a row -- between two oracle taps (the oracle
# taps the trunk's output only); at 8x12 the allowance leaves 2 % of the elements free in the mixed recipe.
DEEP = ("cond3", "cond4", "t3y")


@pytest.mark.parametrize("tag", list(Q.RECIPES))
def test_the_stage_table_is_the_fake_quant_network(golden_dir, tag):
    """With the quantisers as they are, v of every stage is oracle.hdrtvnet_oracle on O.w8a8_state(...) within 1e-5 -- except where a
    code can flip: an element whose pre-rounding coordinate lies within the oracle's fp32 error (and 1e-5) of a rounding tie is one
    step apart in the two evaluations, and everything it reaches moves by |w| step.  Bounded8(ties = NOISE) carries exactly that
    allowance and no other term (no fp16, no fp32 rounding): d = 0 at every element no such code reaches, and there the two agree
    to 1e-5 (measured: 1.9e-6).  The allowance is a worst case over fan-ins of 64 .. 576 codes, so it is nonzero at a large share of a
    3x3 chain's outputs (printed per segment, with the share that really differs by more than 1e-5: those are the flips)."""
    from oracle import hdrtvnet_oracle as O
    P, sd = recipe(golden_dir, tag, rounded=False)
    d = np.load(os.path.join(golden_dir, f"int8_{tag}_qat_w8a8_64x96_gradient_s6.npz"))
    agcm = d["agcm_out"]
    ot = {}
    want = O.le(sd, agcm, ot)
    relu = lambda a: np.maximum(a, 0)          # noqa: E731
    have = {"agcm": agcm, "out": want, "cond": ot["LE.cond_first"], "cond1": ot["LE.CondNet1"], "cond2": ot["LE.CondNet2"],
            "cond3": ot["LE.CondNet3"], "cond4": ot["LE.CondNet4"], "f0a": relu(ot["LE.conv_first"]), "fea0": relu(ot["LE.HR_conv1"]),
            "fea1a": relu(ot["LE.down_conv1"]), "fea1": ot["LE.recon_trunk1"], "fea2a": relu(ot["LE.down_conv2"]), "fea2": ot["LE.recon_trunk2"],
            "fea3": relu(ot["LE.down_conv3"]), "t4": ot["LE.recon_trunk4"], "t5": ot["LE.recon_trunk5"],
            "t3y": ot["LE.recon_trunk3"] + relu(ot["LE.down_conv3"])}
    have = {k: R.as_t(v) for k, v in have.items()}
    by_name = {s.name: s for s in Q.stages(P)}
    covered = set()
    for seg in SEGMENTS:
        seg = [s for s in seg if s in by_name]
        covered.update(seg)
        c = Q.Check(seg, by_name=by_name, taps=have)
        assert set(c.ins) <= set(have), (seg, c.ins)
        got = c.run(Q.Bounded8(ties=NOISE), P, have)
        for t in c.outs:
            v, dd = got[t]
            err = (v - have[t]).abs()
            clear = float(err[dd == 0].max()) if bool((dd == 0).any()) else 0.0
            print(f"  {tag:5s} {c.name:16s} {t:6s} max |v - oracle| where no code can flip {clear:.2e}  allowance > 0 at "
                  f"{float((dd > 0).double().mean()):.2e}  differing by > 1e-5 at {float((err > TOL).double().mean()):.2e}")
            assert bool((err <= TOL + dd).all()), (tag, seg, t, float((err - dd).max()))
            # ... and the comparison must not quietly become empty: a tenth of the elements at least carries no allowance at all
            assert t in DEEP or float((dd == 0).double().mean()) >= 0.1, (tag, seg, t, float((dd == 0).double().mean()))
    assert covered == set(by_name)
    # the reference's own run (tests/golden/gen_golden_w8a8.py): the whole graph chained from its AGCM output, same allowance.  The file
    # has no tap to restart from, so the allowance composes: it is empty at `cond` of the mixed recipe, reaches 9 % / 54 % of the
    # elements at `cond` / `fea0` of the full one and every element behind the ResBlocks (printed) -- there this comparison says no
    # more than the end-to-end bars of tests/test_gpu_int8_hr.py do; the segments above are what holds the stage table
    o = Q.Bounded8(ties=NOISE)
    env = Q.full_graph(P, R.as_t(d["agcm_out"]), o)
    for t, a, step in (("cond", d["tap:LE.cond_first"], 8), ("fea0", relu(d["tap:LE.HR_conv1"]), 4), ("f0b", relu(d["tap:LE.HR_conv2"]), 4),
                       ("out", d["out"], 1)):          # the golden file keeps every 8th / 4th channel of a tap
        v, dd = env[t][0][::step], env[t][1][::step]
        err = (v - R.as_t(a)).abs()
        print(f"  {tag:5s} reference run {t:5s} max err where no code can flip {float(err[dd == 0].max()) if bool((dd == 0).any()) else 0.0:.2e}  allowance > 0 at {float((dd > 0).double().mean()):.2e}")
        assert bool((err <= TOL + dd).all()), (tag, t, float((err - dd).max()))
    # a launch nobody claims, a missing launch and a wrong kernel tag are errors
    Pr = recipe(golden_dir, tag)[0]
    prof = Q.per_layer_profile(Pr)
    assert {s.name for c in Q.plan(prof, Pr) for s in c.stages} == {s.name for s in Q.stages(Pr)}
    assert sorted(c.name for c in Q.plan(prof, Pr) if c.composite) == ["rt1a+rt1b", "rt2a+rt2b", "rt30a..rt32b"]
    assert Q.TAGS[tag] <= {k for _, k in prof}
    for bad in (prof + [("LE.some_new_launch", "kernel")], prof[:-1], [(l, "conv_q8<32,3,1>" if k == "conv_q8<32,3,2>" else k) for l, k in prof]):
        with pytest.raises(AssertionError):
            Q.plan(bad, Pr)


@pytest.mark.parametrize("layer,stride", [("LE.up_conv1.0", 1), ("LE.down_conv1", 2), ("LE.CondNet4.4", 2), ("LE.conv_first", 1)])
def test_the_folded_shift_is_the_networks_zero_padding_at_every_border_class(golden_dir, layer, stride):
    """The model's form -- out-of-image taps as int8 code 0, shift[class] with the in-image taps' weight sum folded in -- with no
    rounding at all equals the network form of v (zero padding after dequantisation) on maps small enough to enumerate: 3x3, 1x3,
    3x1 and 1x1 together show all 16 classes (on a one-row / one-column map both bits of an axis are set)."""
    P, _ = recipe(golden_dir, "full")
    L = P.q[layer]
    g = torch.Generator().manual_seed(5)
    seen = set()
    for h, w in ((3, 3), (1, 3), (3, 1), (1, 1), (4, 5), (5, 4)):
        seen |= set(Q.border_classes(h, w, 3, stride).reshape(-1).tolist()) if (h, w) in ((3, 3), (1, 3), (3, 1), (1, 1)) else set()
        x = R.f16(L.xz + L.xs * 255.0 * torch.rand((L.w8.shape[1], h, w), generator=g, dtype=torch.float64))
        b, m = Q.Bounded8(), Q.Rounded8(exact=True)
        v = b.qconv(b.quant((x, torch.zeros_like(x)), L), L, stride)[0]
        got = m.qconv(m.quant(x, L), L, stride)
        assert float((got - v).abs().max()) <= 1e-11 * max(1.0, float(v.abs().max())), (layer, h, w)
    assert (seen == set(range(16))) if stride == 1 else (seen >= {5, 13, 7, 15})


def _frames():
    return [pytest.param(tag, size, kind, id=f"{tag}-{size[0]}x{size[1]}-{kind}") for tag in Q.RECIPES for size in R.FRAMES for kind in ("noise", "gradient")]


@pytest.mark.parametrize("tag,size,kind", _frames())
def test_the_model_stays_inside_the_bound_and_the_cap_on_the_gpu_tests_frames(golden_dir, tag, size, kind):
    """On inputs made by the oracle for every frame of the GPU test: the model alone meets the hard condition at every output, the
    marked share of every capped quantiser is at most max(2 elements, 1e-3), and the input condition holds wherever the GPU test
    asks it."""
    P, _ = recipe(golden_dir, tag)
    taps = frame_taps(golden_dir, tag, size, kind)
    for c in all_checks(P, tag):
        res, marks = Q.evaluate(c, P, taps)
        ok, worst, _, wide_ok = Q.cap_ok(marks)
        assert ok, (c.name, [(l, m, n) for l, m, n, k, _e in marks if k and m > max(Q.CAP_MIN, Q.CAP_SHARE * n)])
        assert wide_ok, (c.name, [(l, m / n, e) for l, m, n, k, e in marks if not k])
        for t, r in res.items():
            m = R.metrics(r, r["model"])
            assert m["violations"] == 0 and m["max_ratio"] <= 1.0, (c.name, t, m)
            okin, share, asked = Q.input_ok(c, r)
            assert okin, (c.name, t, share, asked)


# mistake -> recipe -> the checks that must see it, on the GPU test's own 61x103 gradient frame (maps 31x52, 16x26, 8x13: odd maps at
# two levels, all 16 border classes at the first)
_EDGE = {"full": ("trunk", "c234", "h2a", "cond4", "f0a", "fea0", "fea1a", "up1", "rt5b", "out"), "mixed": ("c234", "h2a", "cond4", "fea1a", "rt33a", "up2")}
MISTAKES = {
    "cls_swap": _EDGE, "cls0": _EDGE, "pad128": _EDGE,
    "s2_last_pad": {"full": ("c234", "h2a", "h2b", "fea1a", "fea2a"), "mixed": ("c234", "h2a", "h2b", "fea1a", "fea2a")},
    "trunc": {"full": ("trunk", "trunk1", "c234", "f0a", "fea1a", "up1", "out", "img32"), "mixed": ("trunk1", "c234", "cond2", "fea1a", "up3")},
    "oq_fp32": {"full": ("c234", "h2a", "h2b"), "mixed": ("c234", "h2a", "h2b")},
    "wrap": {"full": (), "mixed": ("trunk1", "c234")},
    "no128": {"full": ("trunk", "c234", "f0a", "fea1a", "up1", "out", "img32"), "mixed": ("trunk1", "c234", "cond2", "fea1a", "up1")},
    "khalf_swap": {"full": ("fea0", "rt33a", "up1", "rt5b", "f0b", "out"), "mixed": ("rt33a", "up1", "rt4a", "up3")},
    "no_plus1": {"full": ("fea0", "rt33a", "rt4a", "rt5b", "f0b"), "mixed": ("fea0", "rt33a", "rt4b", "f0b")},
    "slope02": {"full": ("trunk", "trunk1", "cond2", "fea0", "rt33a"), "mixed": ("trunk", "cond2")},
    "other_zero": {"full": ("trunk", "c234", "f0a", "fea1a", "up1", "rt33a", "img32"), "mixed": ("trunk1", "c234", "fea1a", "up1")},
}


@pytest.mark.parametrize("tag", list(Q.RECIPES))
@pytest.mark.parametrize("mut", list(MISTAKES))
def test_a_mistaken_model_leaves_the_hard_condition(golden_dir, mut, tag):
    """Class row and column bits exchanged; class 0's shift everywhere (padding as int8 code 0 without the correction); padding as u8
    code 0 (int8 -128, i.e. the value x_zero) under the unchanged table; the last row / column of a stride-2 layer on an odd map read
    as padding; floor instead of round-to-nearest in the input quantiser; the output quantiser on the fp32 value instead of the f16-
    rounded one; codes that wrap at 255 instead of saturating; the u8 byte read as int8 without the - 128; the two channel halves of the
    32-channel K order exchanged (channel 8 qd + 4 lh + k); the SFT scale's + 1 dropped; LeakyReLU slope 0.2 in a re-quantised hidden
    layer (and in the fp16 chains); another layer's x_zero.  Each must leave the hard condition at >= 8 elements of every listed check.
    Out of reach: `wrap` on the full recipe -- on the GPU test's frames no input of its quantisers lies above code 255, so wrapping and
    saturating agree; the mixed recipe's CondNet1.4 and CondNet3.0 / 4.0 inputs do saturate and show it."""
    P, _ = recipe(golden_dir, tag)
    taps = frame_taps(golden_dir, tag, (61, 103), "gradient")
    names = sorted(P.q)
    other = {n: P.q[names[(i + 1) % len(names)]].xz for i, n in enumerate(names)}
    by = {}
    for c in all_checks(P, tag):
        by.setdefault(c.name, c)          # f0a: conv_c3_q8's form (quantise on load), not the generic one behind img32
    for stage in MISTAKES[mut][tag]:
        c = by[stage]
        ref, _ = Q.evaluate(c, P, taps)
        got = c.run(Q.Rounded8(mut, other=other), P, taps)
        bad = sum(R.metrics(ref[t], got[t])["violations"] for t in c.outs)
        print(f"  {tag:5s} {mut:12s} {stage:7s} violations {bad}")
        assert bad >= 8, (tag, mut, stage, bad)
