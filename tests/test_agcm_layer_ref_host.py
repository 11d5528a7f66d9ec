"""The checker of tests/test_gpu_agcm_layers.py checked itself (CPU, no device): tests/agcm_layer_ref.py's stage table is the
network, its rounding model stays inside its own bound, the frames of the GPU test meet the input condition, and deliberate
mistakes of the kind these kernels can make break the hard bound."""
import os

import numpy as np
import pytest

import agcm_layer_ref as R

GOLDEN_FRAMES = ("hr_64x96_noise_s0", "hr_60x100_noise_s2", "hr_52x76_gradient_s5", "hr_32x96_gradient_s1_taps")


@pytest.fixture(scope="module")
def packed(hr_state):
    return R.pack(hr_state)


_TAPS = {}


def frame_taps(hr_state, packed, size, kind):
    """The taps of one GPU-test frame, synthesised from the rounding model on the oracle's preprocess of that frame (rounded to
    f16, as the device's preprocess tensors are)."""
    if (size, kind) not in _TAPS:
        from hdrtv_mi355x import weights as W
        from oracle import hdrtvnet_oracle as O
        f = W.synthetic_frame(*size, seed=R.FRAMES[size][kind == "gradient"], kind=kind)
        tensor, cond = O.preprocess(f)
        _TAPS[(size, kind)] = R.full_graph(packed, R.f16(R.as_t(tensor)), R.f16(R.as_t(cond)), R.Rounded())
    return _TAPS[(size, kind)]


def test_the_sizes_have_the_properties_they_are_there_for():
    """The map arithmetic the frames were chosen by, restated from shapes_for / cls_block_launch / agcm_mlp_launch."""
    for size in R.FRAMES:
        assert R.admits(*size)
        assert tuple(R.px_of(h * w) for h, w in R.maps_for(*size)[1:]) == R.FORMS[size], size
    # the smallest frame the classifier admits: nothing smaller in either dimension passes do_reserve's conditions
    assert not any(R.admits(h, w) for h in range(8, 68) for w in range(8, 68))
    assert R.admits(8, 68) and not R.admits(8, 67)
    assert R.maps_for(36, 72)[1:] == [(5, 9), (3, 5), (2, 3), (1, 2), (1, 1)]
    m = R.maps_for(61, 103)
    assert m[:5] == [(15, 25), (8, 13), (4, 7), (2, 4), (1, 2)] and (61 * 103) % 32 == 11 and (1 * 2) % 4 != 0
    assert all(h % 2 or w % 2 for h, w in R.maps_for(69, 133)[:5]) and (9 * 17) % 4 == 1 and (69 * 133) % 32 == 25
    m = R.maps_for(270, 486)
    assert m[1] == (34, 61) and R.nblk_of(34 * 61) == 519 > 256
    m = R.maps_for(520, 1016)
    assert m[0] == (130, 254) and m[1] == (65, 127) and 65 * 127 > 4096 and (65 * 127) % 16 == 15
    assert R.mlp_grid(520 * 1016) == (16510, 8192, 3) and 16510 % 8192 != 0
    m = R.maps_for(1036, 1076)
    assert m[1:4] == [(130, 135), (65, 68), (33, 34)] and (130 * 135) % 16 == 14 and 65 * 68 > 4096 and (65 * 68) % 16 == 4
    assert 33 * 34 <= 4096 and (1036 * 1076) % 32 == 16 and R.mlp_grid(1036 * 1076)[2] > 1


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_the_stage_table_is_the_network(golden_dir, hr_state, packed, name):
    """All stages assembled in float64 on a golden frame's tensor / cond are oracle.hdrtvnet_oracle.agcm and agcm_classifier
    (fp32) and the golden fea6 / agcm_out within 1e-5."""
    from oracle import hdrtvnet_oracle as O
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    e = R.full_graph(packed, R.as_t(z["tensor"]), R.as_t(z["cond"]))
    assert float((e["out"] - R.as_t(O.agcm(hr_state, z["tensor"], z["cond"]))).abs().max()) <= 1e-5
    assert float((e["fea6"] - R.as_t(O.agcm_classifier(hr_state, z["cond"]))).abs().max()) <= 1e-5
    assert float((e["out"] - R.as_t(z["agcm_out"])).abs().max()) <= 1e-5
    if "fea6" in z.files:
        assert float((e["fea6"] - R.as_t(z["fea6"])).abs().max()) <= 1e-5


def test_the_plan_claims_every_launch_and_nothing_else():
    prof = R.default_profile()
    assert [c.name for c in R.plan(prof)] == [s.name for s in R.STAGES]
    assert [c.launch for c in R.plan([("hdrtv_pre", "unpack")] + prof + [("LE.cond_trunk", "le_cond_trunk")])] == list(range(12))
    with pytest.raises(AssertionError):                     # an AGCM launch nobody knows
        R.plan(prof + [("agcm_something_new", "kernel")])
    with pytest.raises(AssertionError):                     # a known layer on an unknown kernel
        R.plan(prof[:-1] + [("agcm_mlp", "agcm_mlp_v2")])
    with pytest.raises(AssertionError):                     # a classifier in five launches: the statistics inside cls_block
        R.plan([r for r in prof if r[0] != "cls_stats"])
    with pytest.raises(AssertionError):
        R.plan([("cls_block", "cls_block+stats") if r[0] == "cls_block" else r for r in prof if r[0] != "cls_stats"])
    with pytest.raises(AssertionError):                     # one launch more than the table has
        R.plan(prof + [("cls_block", "cls_block")])
    with pytest.raises(AssertionError):                     # launches in another order than the data flow
        R.plan(prof[1:2] + prof[0:1] + prof[2:])
    for fq in (("cls_block", "cls_block<fq>"), ("agcm_fold", "agcm_fold<q8>"), ("agcm_mlp", "agcm_mlp<q8>")):
        with pytest.raises(AssertionError, match="W8A8"):
            R.plan([fq if r[0] == fq[0] else r for r in prof])


def test_the_fragment_layout_is_a_bijection():
    """Every element of the three padded operand matrices has exactly one slot; decode is scatter's inverse."""
    lay, row, col, used = R.frag_layout()
    for i, shape in enumerate(((64, 16), (64, 64), (32, 64))):
        sel = lay == i
        assert sorted(zip(row[sel].tolist(), col[sel].tolist())) == [(r, c) for r in range(shape[0]) for c in range(shape[1])]
    assert int(used.sum()) == 64 * 3 + 64 * 64 + 3 * 64
    assert sorted(R.acc_kperm16(p) for p in range(16)) == list(range(16)) and [R.acc_kperm16(p) for p in (0, 4, 8, 12)] == [0, 8, 4, 12]
    import torch
    g = torch.Generator().manual_seed(0)
    mats = [torch.rand(s, generator=g, dtype=torch.float64) + 1 for s in ((64, 3), (64, 64), (3, 64))]
    A1, A2, A3 = R.decode_frags(R.scatter_frags(mats))
    assert bool((A1[:, :3] == mats[0]).all()) and bool((A1[:, 3:] == 0).all()) and bool((A2 == mats[1]).all())
    assert bool((A3[:3] == mats[2]).all()) and bool((A3[3:] == 0).all())


@pytest.mark.parametrize("kind", ["noise", "gradient"])
@pytest.mark.parametrize("size", list(R.FRAMES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_model_stays_inside_the_bound_and_the_frames_meet_the_input_condition(hr_state, packed, size, kind):
    """On every frame the GPU test uses, with taps synthesised from the rounding model: the model violates no bound (so the GPU
    test cannot fail for the reference's sake), and EVERY output meets le_layer_ref.input_condition (so it cannot fail, or
    pass, for the frames' sake) -- the six-element fea6 and the statistics of the 1x2 and 1x1 maps included: no output had to
    be exempted."""
    taps = frame_taps(hr_state, packed, size, kind)
    for c in R.plan(R.default_profile()):
        for t, r in R.evaluate(c, packed, taps).items():
            m = R.metrics(r, r["model"])
            assert m["violations"] == 0 and m["max_ratio"] <= 1.0, (c.name, t, m)
            ok, share, share_nz = R.input_condition(r)
            assert ok, (c.name, t, share, share_nz)


CLS = ("cls1", "cls2", "cls3", "cls4", "cls5")
# mutation -> [(frame, the checks that must see it)]
MUTATIONS = {
    "pool_div_cnt": [((61, 103), CLS), ((1036, 1076), CLS[:2])],
    "bias_x9": [((61, 103), CLS), ((1036, 1076), CLS[:2])],
    "window_clamp": [((69, 133), CLS), ((520, 1016), ("cls2",)), ((1036, 1076), ("cls1", "cls3"))],
    "slope01": [((61, 103), CLS), ((1036, 1076), CLS[:2])],
    "wrong_gamma": [((61, 103), CLS[1:]), ((1036, 1076), ("cls2",))],
    "idle_lanes": [((69, 133), ("stats1",)), ((520, 1016), ("stats1",)), ((1036, 1076), ("stats1", "stats2"))],
    "drop_last_wg": [((61, 103), ("stats1", "stats2")), ((270, 486), ("stats1",)), ((520, 1016), ("stats1",)),
                     ((1036, 1076), ("stats1", "stats2"))],
    "no_eps": [((61, 103), ("stats1", "stats2", "stats3")), ((1036, 1076), ("stats1", "stats2"))],
    "unbiased": [((61, 103), ("stats1", "stats2", "stats3", "stats4")), ((1036, 1076), ("stats1", "stats2"))],
    "l2_natural_k": [((61, 103), ("fold",))],
    "l3_row_shift": [((61, 103), ("fold",))],
    "no_relu3": [((61, 103), ("mlp",))],
    "bias_after_store": [((270, 486), ("mlp",)), ((520, 1016), ("mlp",))],
    "tail_not_written": [((61, 103), ("mlp",)), ((69, 133), ("mlp",))],
    "pixel0_leak": [((61, 103), ("mlp",)), ((69, 133), ("mlp",))],
}


def test_every_mutation_is_listed():
    assert set(MUTATIONS) == set(R.Rounded.MUTATIONS)


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_a_mutated_model_violates_the_hard_bound(hr_state, packed, mut):
    """Each mistake, switched on in the rounding model on the GPU test's own frames, must leave the hard bound |x - v| <= d of
    every check listed for it.  All but one do so at many elements.  `bias_after_store` is a second f16 rounding of a value that
    is rounded anyway, about as large as the roundings the bound has to allow: it leaves the bound at a few elements in 10^5
    (7 of 393660 at 270x486, 2 of 1584960 at 520x1016) and at none of 61x103's 18849, so it is listed at the sizes that have
    the elements -- which the GPU test runs."""
    for size, names in MUTATIONS[mut]:
        taps = frame_taps(hr_state, packed, size, "noise")
        for name in names:
            c = R.Check(name)
            ref = R.evaluate(c, packed, taps)
            got = c.run(R.Rounded(mut), packed, taps)
            bad = {t: R.metrics(ref[t], got[t])["violations"] for t in c.outs}
            print(f"  {mut:18s} {size[0]}x{size[1]} {name:7s} violations {bad}")
            assert sum(bad.values()) > 0, (mut, size, name, bad)
