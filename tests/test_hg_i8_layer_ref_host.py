"""The checker of tests/test_gpu_hg_i8_layers.py checked itself (CPU, no device): tests/hg_i8_layer_ref.py's network form is the oracle's
fake-quant head and the reference's own W8A8 run, its folded border constants are the network's zero padding at all 16 classes, its model
stays inside its own conditions on every frame the GPU test uses, and deliberate mistakes of the kind an int8 kernel or its packer can
make leave the hard condition."""
import os
import re

import numpy as np
import pytest
import torch

import hg_i8_layer_ref as G
import hg_layer_ref as H
import le_i8_layer_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-5           # the oracle's fp32 convolutions against float64, absolute, at activations of 1 .. 10: measured 2.1e-6 at most (printed)
NOISE = 5e-6         # ... and what of it a quantiser INSIDE a compared segment may see on its input: twice the measured figure
ODD_SIZE = (90, 150)
_C = {}


def qstate(cal):
    if ("sd", cal) not in _C:
        from hdrtv_mi355x import weights as W
        sd = W.seeded_hg_w8a8_state(1234, integer_zero=cal != "minmax")
        if cal == "odd":          # tests/test_gpu_int8_hg.py::test_w8a8_checkpoint_file_and_loader_errors: Up_conv2.0's zero point moved by 0.4 steps
            sd = dict(sd)
            sd["Up_conv2.0.x_zero"] = np.array(float(sd["Up_conv2.0.x_zero"]) + 0.4 * float(sd["Up_conv2.0.x_scale"]), np.float32)
        _C[("sd", cal)] = sd
    return _C[("sd", cal)]


def packed(cal):
    if ("P", cal) not in _C:
        _C[("P", cal)] = G.pack(qstate(cal))
    return _C[("P", cal)]


def frame_taps(hr_state, cal, size, kind):
    """(P, every tensor of the head as the device would hand it out): the MODEL chained on the oracle's LE output of a GPU-test frame."""
    key = (cal, size, kind)
    if key not in _C:
        from hdrtv_mi355x import weights as W
        from oracle import hdrtvnet_oracle as O
        seed, r = G.FRAMES[size][kind == "gradient"]
        if ("base", size, kind) not in _C:
            _C[("base", size, kind)] = H.f16(H.as_t(O.hr_forward(hr_state, *O.preprocess(W.synthetic_frame(*size, seed=seed, kind=kind)))[0]))
        for k in [k for k in _C if len(k) == 3 and k[0] in ("integer", "minmax", "odd") and (k[1], k[2]) != (size, kind) and k[1] == (272, 480)]:
            del _C[k]             # keep the cache small
        _C[key] = (r, G.model_env(packed(cal).with_mask_r(r), _C[("base", size, kind)]))
    r, env = _C[key]
    return packed(cal).with_mask_r(r), env


def one(name):
    return G.Check([name], by_name=G.BY_NAME, taps=G.TAPS)


# ------------------------------------------------------------------------------------------------- against the oracle and the reference
def _net_segment(P, names, x_real, skips, noise):
    """The NETWORK form of the layers `names` chained on a real-valued input (the oracle's tap), float64 -> (y, dd): dd > 0 wherever a
    code of a quantiser inside can flip between this evaluation and an fp32 one (a coordinate within the fp32 error of a tie), carried
    on as |W| step |gain|."""
    y, dy = x_real, torch.zeros_like(x_real)
    for i, name in enumerate(names):
        L = P.L[name]
        if L.skip:
            y, dy = torch.cat((y, skips[name])), torch.cat((dy, torch.zeros_like(skips[name])))
        t = (y - L.q.xz) / L.q.xs
        code = torch.clamp(torch.round(t), 0, 255)
        # the oracle takes rint(fl(fl(x - z) / s)) in fp32: its coordinate is within 4 U32 (|t| + |z / s|) of this one
        reach = ((noise if i else 0.0) + dy) / L.q.xs + 4 * G.U32 * (t.abs() + abs(L.q.xz / L.q.xs))
        unc = ((t - torch.floor(t) - 0.5).abs() <= reach) & (t > -0.5 - reach) & (t < 255.5 + reach)
        W = (L.w8 * L.ws[:, None, None, None]).abs()
        y = G.network(L, code - 128.0)
        dy = H._conv(unc.double() * L.q.xs, W, 1) * L.gain().abs()[:, None, None]
        if L.relu:
            y = torch.clamp(y, min=0.0)
        if L.ps:
            y, dy = H._ps2(y), H._ps2(dy)
        if L.mode == "pool":
            y, dy = H._pool(y), H._pool(dy)
    return y, dy


SEGMENTS = ((("conv2",), "hg.p1", "hg.conv2"), (("conv3_1", "conv3_2"), "hg.conv2", "hg.conv3_2"), (("conv4_1", "conv4_2"), "hg.conv3_2", "hg.conv4_2"),
            (("conv5_1", "conv5_2"), "hg.conv4_2", "hg.conv5_2"), (("conv_code1", "conv_code2"), "hg.conv5_2", "hg.conv_code2"),
            (("Up_conv1", "conv6"), "hg.conv_code2", "hg.conv6"), (("Up_conv2", "conv7"), "hg.conv6", "hg.conv7"),
            (("Up_conv3", "conv8"), "hg.conv7", "hg.conv8"), (("Up_conv4", "conv9"), "hg.conv8", "hg.conv9"), (("Up_conv5",), "hg.conv9", "hg.up5"))
GOLDEN = {"integer": "hg_w8a8_96x128_gradient_s3.npz", "minmax": "hg_w8a8_floatzero_96x128_gradient_s3.npz"}


@pytest.mark.parametrize("cal", list(GOLDEN))
def test_the_network_form_is_the_oracles_fake_quant_head_and_the_references_run(golden_dir, cal):
    """v of every int8 stage, chained between two tensors the oracle taps and fed the ORACLE's input (end to end a re-quantised graph is
    chaotic in the small, segment by segment it is not), is oracle.hdrtvnet_oracle.hg_generator on O.w8a8_state(...) within TOL at
    every element no code flip reaches, and that is at least a tenth of every tensor (printed: the largest difference there, the share
    compared).  The reference's own run (tests/golden/gen_golden_hg_w8a8.py) keeps every 4th / 16th channel of seven taps: the oracle
    reproduces them on the file's base (asserted here to 1e-6 -- tests/test_oracle_golden.py pins it bit-exact), so the segments are
    compared with the FILE's values wherever it has them.  All 18 rows are inside a segment; prep, conv1 and final are H's stages,
    held to the oracle by tests/test_hg_layer_ref_host.py on the same fp16 weights."""
    from oracle import hdrtvnet_oracle as O
    sd = qstate(cal)
    P = packed(cal)
    d = np.load(os.path.join(golden_dir, GOLDEN[cal]))
    base = d["tap:base"]
    ot = {}
    O.use_backend("aten")          # ATen's convolutions under the oracle's graph: bit-exact against the reference's run (tests/test_oracle_golden.py)
    try:
        O.hg_generator(O.w8a8_state(sd), base, O.hg_mask(base), ot)
    finally:
        O.use_backend("c")
    have = {k: H.as_t(v) for k, v in ot.items()}
    for k in d.files:
        if k.startswith("tap:hg."):
            a, full = H.as_t(d[k]), have[k[4:]]
            step = full.shape[0] // a.shape[0]
            assert float((full[::step] - a).abs().max()) <= 1e-6, k
            have[k[4:]] = full.clone()
            have[k[4:]][::step] = a            # the reference's own numbers where the file keeps them
    covered = set()
    skip_of = {"conv6": "hg.conv5_2", "conv7": "hg.conv4_2", "conv8": "hg.conv3_2", "conv9": "hg.conv2"}
    for names, src, dst in SEGMENTS:
        covered.update(names)
        y, dd = _net_segment(P, names, have[src], {n: have[skip_of[n]] for n in names if n in skip_of}, NOISE)
        err = (y - have[dst]).abs()
        clear = dd == 0
        share = float(clear.double().mean())
        print(f"  {cal:8s} {'+'.join(names):22s} -> {dst:14s} max |v - oracle| where no code can flip {float(err[clear].max()):.2e} (tolerance {TOL:.0e})  "
              f"compared {share:.3f}  differing by more elsewhere {float((err > TOL).double().mean()):.2e}")
        assert bool((err[clear] <= TOL).all()), (names, float(err[clear].max()))
        assert share >= 0.1, (names, share)
    assert covered == set(P.L)


def test_the_consumer_column_and_the_plan_are_the_librarys():
    """CONSUMER against hg_layers' `consumer` column of csrc/api.h; one check per launch; an unknown launch, a missing one, a need-list
    launch and a kernel tag the layer cannot have are errors; the tag set is what Seq::c3 / Seq::conv8 can emit for this table."""
    src = open(os.path.join(HERE, "..", "hdr-realtime-video-pipeline_amd", "csrc", "api.h")).read()
    body = src.split("inline constexpr HgLayer hg_layers[] = {", 1)[1].split("};", 1)[0]
    rows = re.findall(r'\{"(\w+)", [^{}]*?, "[\w.]*", (nullptr|"[\w.]+"), (?:nullptr|"\w+")\}', body)
    assert len(rows) == 18
    for name, cons in rows:
        assert (G.CONSUMER[name] and f'"{G.CONSUMER[name]}"') == (None if cons == "nullptr" else cons), (name, cons)
    for prw in ("", "prw", "prw8"):
        checks = G.plan(G.dense_profile(prw))
        assert [c.name for c in checks] == [s.name for s in G.STAGES] and len(checks) == 21
    assert {k for _, k in G.dense_profile("prw")} | {k for _, k in G.dense_profile("prw8")} | {k for _, k in G.dense_profile()} == set(G.KERNEL_TAGS)
    assert len(G.KERNEL_TAGS) == 15 and "conv1x1_i8<f16>" not in G.KERNEL_TAGS
    prof = G.dense_profile()
    for bad in (prof + [("hg.some_new_launch", "kernel")], prof + [("hg_need", "hg_need")], prof[:-1],
                [(l, "conv_pglds_i8<nhwc>" if l == "hg.conv3_1" else k) for l, k in prof], [(l, "conv_glds1" if l == "hg.conv6" else k) for l, k in prof]):
        with pytest.raises(AssertionError):
            G.plan(bad)


@pytest.mark.parametrize("cal,name", [("integer", "conv3_2"), ("minmax", "conv3_2"), ("integer", "Up_conv3"), ("minmax", "Up_conv3"), ("odd", "Up_conv2"),
                                      ("integer", "Up_conv5"), ("minmax", "Up_conv5")])
def test_the_folded_constants_are_the_networks_zero_padding_at_every_border_class(cal, name):
    """With no rounding at all, acc * scale + shift + delta[cls] (out-of-image taps as int8 code 0) equals the network form (zero
    padding after dequantisation, BatchNorm, the reader's coordinate) on maps small enough to enumerate: 3x3, 1x3, 3x1 and 1x1 together
    show all 16 classes (on a one-row / one-column map both bits of an axis are set).  Integer zero points (k != 128: delta is still in
    use), float zero points (minmax: the readers of conv6 .. conv9's outputs) and the `odd` checkpoint; for Up_conv5 the same identity
    through delta_acc, exact for an integer zero point and within half an accumulator unit otherwise."""
    P = packed(cal)
    L = P.L[name]
    T = G.tables(L)
    assert T["need"] and (cal == "integer") == L.q.integer or name == "conv3_2", (name, L.q.kf)
    g = torch.Generator().manual_seed(11)
    seen = set()
    for h, w in ((3, 3), (1, 3), (3, 1), (1, 1), (4, 5)):
        c = torch.randint(-128, 128, (L.cin, h, w), generator=g).double()
        cls = G.classes(L, h, w)
        if (h, w) != (4, 5):
            seen |= set(cls.reshape(-1).tolist())
        acc = Q._pad_conv(c, L.w8, 1)
        y = G.network(L, c)
        if L.o:
            got = acc * T["x_sc"][:, None, None] + T["x_sh"][:, None, None] + 128.0 + T["x_delta"][cls].permute(2, 0, 1)
            want = (y - L.o.xz) / L.o.xs
            tol = 1e-9 * float(want.abs().max())
        else:
            got = (acc + T["dacc"][cls].permute(2, 0, 1)) * T["x_sc"][:, None, None] + T["x_sh"][:, None, None]
            want = y
            tol = 1e-9 * float(want.abs().max()) + (0.0 if L.q.integer else 0.5 * float(T["x_sc"].abs().max()))
            assert L.q.integer == (float(T["dacc_res"].max()) == 0.0)
        assert float((got - want).abs().max()) <= tol, (name, h, w, float((got - want).abs().max()), tol)
    assert seen == set(range(16))


# ------------------------------------------------------------------------------------------------- the model on the GPU test's frames
def _frames():
    out = [pytest.param(cal, size, kind, id=f"{cal}-{size[0]}x{size[1]}-{kind}") for cal in G.CALIBRATIONS for size in G.FRAMES for kind in ("noise", "gradient")]
    return out + [pytest.param("odd", ODD_SIZE, "gradient", id="odd-90x150-gradient")]


@pytest.mark.parametrize("cal,size,kind", _frames())
def test_the_model_stays_inside_its_own_conditions_on_the_gpu_tests_frames(hr_state, cal, size, kind):
    """For every launch, calibration, size and frame of the GPU test, on the CPU alone, chained from the oracle's LE output: the model
    meets the hard condition at every output, the folded form lies inside the network form's bound at every element, the marked share is
    at most max(2 elements, 1e-3), conv1's widened share is what its bound explains, every input condition holds and the mask is a
    10 .. 90 % mixture.  This fixes the seeds and mask_r of hg_layer_ref.FRAMES for the int8 head."""
    P, taps = frame_taps(hr_state, cal, size, kind)
    frac = float(taps["mask"][:, :size[0], :size[1]].mean())
    assert 0.1 <= frac <= 0.9, frac
    low = 1.0
    for c in G.plan(G.dense_profile()):
        res, marks = G.evaluate(c, P, taps)
        ok, worst, wide, wide_ok = G.cap_ok(marks)
        assert ok and wide_ok, (c.name, marks)
        for t, r in res.items():
            m = G.metrics(r, r["model"])
            assert m["violations"] == 0 and m["max_ratio"] <= 1.0 and r["fold"] == 0, (c.name, t, m, r["fold"])
            okin, share = G.input_ok(t, r)
            low = min(low, share)
            assert okin, (c.name, t, share)
    print(f"  {cal} {size[0]}x{size[1]} {kind}: mask {frac:.3f}, smallest clear / in-range share {low:.2f}")


# ------------------------------------------------------------------------------------------------- mistakes
# mistake -> (calibration, size) -> the launches that must see it, on the GPU test's own gradient frames.  17x68: level-5 map 1x3, level-4
# map 2x6 (both row bits set at level 5); 96x160: ordinary borders.
MISTAKES = {
    "cls_swap": {("minmax", (17, 68)): ("conv_code2", "Up_conv1", "Up_conv2", "Up_conv4"), ("integer", (96, 160)): ("conv3_2", "Up_conv4")},
    "cls_first": {("minmax", (17, 68)): ("conv_code2", "Up_conv1"), ("integer", (17, 68)): ("conv_code2", "Up_conv1")},
    "cls0": {("minmax", (96, 160)): ("conv2", "conv3_1", "conv5_2", "Up_conv1", "Up_conv3"), ("integer", (96, 160)): ("conv2", "conv4_2", "Up_conv2")},
    "pad128_nodelta": {("minmax", (96, 160)): ("conv2", "Up_conv3")},
    "pad_u8_0": {("minmax", (96, 160)): ("Up_conv2", "Up_conv3", "Up_conv4", "Up_conv5"), ("integer", (96, 160)): ("Up_conv2", "Up_conv4", "Up_conv5")},
    "delta_no_gain": {("minmax", (96, 160)): ("conv2", "conv3_2", "conv5_2"), ("integer", (96, 160)): ("conv2", "conv4_1")},
    "trunc": {("minmax", (96, 160)): ("conv2", "conv3_1", "Up_conv1", "conv6", "conv9"), ("integer", (96, 160)): ("conv2", "conv7", "Up_conv4")},
    "cat_swap": {("integer", (96, 160)): ("conv6", "conv7", "conv8", "conv9")},
    "ps_swap": {("integer", (96, 160)): ("Up_conv1", "Up_conv2", "Up_conv3", "Up_conv4", "Up_conv5")},
    "conv9_pad_real": {("integer", (96, 160)): ("conv9",)},
    "no_f16": {("integer", (96, 160)): ("Up_conv5",), ("minmax", (96, 160)): ("Up_conv5",)},
    "no_delta_acc": {("minmax", (96, 160)): ("Up_conv5",), ("integer", (96, 160)): ("Up_conv5",)},
    "c1_fp32": {("integer", (96, 160)): ("conv1",), ("minmax", (96, 160)): ("conv1",)},
    "other_zero": {("minmax", (96, 160)): ("conv2", "conv3_2", "Up_conv2", "conv6", "conv9", "Up_conv5"), ("integer", (96, 160)): ("conv2", "Up_conv3", "conv8")},
}


def _violations(c, P, taps, mut, other=None):
    ref, _ = G.evaluate(c, P, taps)
    got, _ = G.evaluate(c, P, taps, mut, other, model_only=True)
    return sum(G.metrics(ref[t], got[t]["model"])["violations"] for t in c.outs), ref, got


@pytest.mark.parametrize("mut", list(MISTAKES))
def test_a_mistaken_model_leaves_the_hard_condition(hr_state, mut):
    """Class row and column bits exchanged; a both-bits class (one-row map) taken as its first bit only; class 0 everywhere -- which is
    also `padding as code 128 without delta`: u8 128 is int8 0, the code the halo really holds, so the two mistakes are one computation
    and both names are kept; padding as u8 code 0 (int8 -128) under the unchanged tables; delta not scaled by the BatchNorm gain;
    truncation in place of round-to-nearest-even; skip and input concatenated in the wrong order; PixelShuffle positions exchanged;
    conv9's padded half tile stored and read as real channels; Up_conv5's f16 rounding dropped; delta_acc left out at border pixels;
    conv1's quantiser on the fp32 value where the kernel takes the f16 one; another layer's x_zero (the next one in name order that differs).
    Each leaves the hard condition at >= 8 elements of every listed launch (cls_first: >= 2 -- the level-5 map of 17x68 has three
    pixels) on the GPU test's own frames."""
    for (cal, size), names in MISTAKES[mut].items():
        P, taps = frame_taps(hr_state, cal, size, "gradient")
        qn = sorted(L.wname for L in P.L.values())
        for name in names:
            other = None
            if mut == "other_zero":
                i = qn.index(P.L[name].wname)          # the next quantiser in name order whose zero point is another one
                other = next(k for k in (G.ActQ(P.sd, qn[(i + j) % len(qn)]).kf for j in range(1, len(qn))) if k != P.L[name].q.kf)
            bad, _, _ = _violations(one(name), P, taps, mut, other)
            print(f"  {mut:15s} {cal:8s} {size[0]}x{size[1]} {name:10s} violations {bad}")
            assert bad >= (2 if mut == "cls_first" else 8), (mut, cal, size, name, bad)


def test_pool_after_rounding_with_the_clamp_first_is_the_same_tensor(hr_state):
    """The kernels take the 2x2 max of the unrounded values (conv3x3_pglds_i8.hip:323-325: "the 2x2 max of ST_POOL commutes with the
    monotone quantiser"): clamp, round, saturate and THEN pool gives the same codes, on every pooled layer of both calibrations."""
    for cal in G.CALIBRATIONS:
        P, taps = frame_taps(hr_state, cal, (96, 160), "gradient")
        for name in ("conv3_1", "conv4_1", "conv5_1", "conv_code1"):
            c = one(name)
            a, _ = G.evaluate(c, P, taps, model_only=True)
            b, _ = G.evaluate(c, P, taps, "pool_after_round", model_only=True)
            assert torch.equal(a[c.outs[0]]["model"], b[c.outs[0]]["model"]), (cal, name)


def test_wrap_in_place_of_saturation(hr_state):
    """Codes that wrap at 255 instead of saturating.  On the GPU test's frames the calibration table's ranges (measured on gradient
    frames at 288x480) are exceeded by the 96x160 gradient frame at the launches listed: there the model saturates (printed: how many
    elements -- conv4_2 and conv7, one element each) and a wrapping epilogue leaves the hard condition there; because that is one
    element, the same is shown at >= 8 elements of conv4_2 on a scaled input (its codes at twice their distance from the zero point)."""
    seen = 0
    for cal in G.CALIBRATIONS:
        P, taps = frame_taps(hr_state, cal, (96, 160), "gradient")
        # ... one element each, so also on a SCALED input: conv4_2's input codes at twice their distance from the zero point
        k = P.L["conv4_2"].q.kf - 128.0
        scaled = dict(taps, p4=torch.clamp(torch.round(2.0 * (taps["p4"] - k) + k), -128, 127))
        bad, ref, _ = _violations(one("conv4_2"), P, scaled, "wrap")
        print(f"  wrap {cal:8s} 96x160 gradient conv4_2 on doubled input codes: saturated {int((ref['conv4_2']['model'] == 127.0).sum())}  violations {bad}")
        assert bad >= 8
        for c in G.plan(G.dense_profile()):
            if c.name not in P.L or c.name == "Up_conv5":
                continue
            bad, ref, got = _violations(c, P, taps, "wrap")
            t = c.outs[0]
            sat = int((ref[t]["model"] == 127.0).sum())
            if bad:
                print(f"  wrap {cal:8s} 96x160 gradient {c.name:10s} saturated {sat:6d}  violations {bad}")
                seen += 1
            assert (bad > 0) == bool(((got[t]["model"] != ref[t]["model"]) & (ref[t]["d"] == 0)).any())
    assert seen >= 1, "no layer saturates on this frame: show it on a scaled one"


def test_a_dropped_lo_clamp_shows_where_the_reader_has_a_negative_zero_point(hr_state):
    """lo_clamp is -128 in every layer of the three checkpoints tested: behind a ReLU both calibrations give k = 0 (the range's minimum
    is 0.0), and conv6 .. conv9 have no ReLU.  So the mistake is shown on a checkpoint made for it: conv3_2's reader quantiser
    (conv4_1.0 and conv8 share it) with its zero point moved to x_zero = -7.3 x_scale, a float kf.  The model clamps at
    nearbyint(7.3) = 7, the network at 0.0 = coordinate 7.3; rounding makes them the same code, as the model-inside-its-conditions check
    below shows on the frame; the model without the clamp leaves the hard condition wherever the ReLU clips."""
    sd = dict(qstate("integer"))
    for k in ("conv4_1.0", "conv8"):
        sd[k + ".x_zero"] = np.array(-7.3 * float(sd[k + ".x_scale"]), np.float32)
    _, taps = frame_taps(hr_state, "integer", (96, 160), "gradient")
    P = G.pack(sd)
    assert G.tables(P.L["conv3_2"])["lo"] == 7.0 - 128.0 and not P.L["conv3_2"].o.integer
    c = one("conv3_2")
    res, marks = G.evaluate(c, P, taps)
    r = res["conv3_2"]
    assert G.metrics(r, r["model"])["violations"] == 0 and r["fold"] == 0 and G.cap_ok(marks)[0]
    assert int(((r["netq"] != r["model"]) & (r["d"] == 0)).sum()) <= 2          # v's own code: the same tensor but at ties within d
    bad, _, _ = _violations(c, P, taps, "no_lo_clamp")
    print(f"  no_lo_clamp conv3_2 (reader kf = 7.3): violations {bad}")
    assert bad >= 8


def test_a_dropped_lo_half_and_what_the_bound_sees_of_it(hr_state):
    """conv_pglds_i8<ps_dot3> without the lo half of its weight pairs moves hg.part by sum (w - hi) x, about 2^-12 relative.  Unlike the
    fp16 head (tests/test_hg_layer_ref_host.py: err/d = 0.3 on a frame), Up_conv5's operands are pinned here: the integer sum is
    exact, so the f16 activations are known but where the few-ulp fp32 epilogue error reaches an f16 rounding boundary.  What remains in d
    is gamma_66 of the fp32 dot products against the 2^-12 of the dropped term: the mistake leaves the bound on the frame itself
    (printed: violations and worst err/d), and it is asserted at >= 8 elements."""
    for cal in G.CALIBRATIONS:
        P, taps = frame_taps(hr_state, cal, (96, 160), "gradient")
        c = one("Up_conv5")
        ref, _ = G.evaluate(c, P, taps)
        got, _ = G.evaluate(c, P, taps, "no_lo", model_only=True)
        m = G.metrics(ref["part"], got["part"]["model"])
        print(f"  no_lo {cal:8s} violations {m['violations']:6d} of {m['n']}  worst err/d {m['max_ratio']:.3g}")
        assert m["violations"] >= 8, m
