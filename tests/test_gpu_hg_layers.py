"""Every launch of the HG head's fp16 path held ALONE to a float64 reference of the same operation.

One frame runs on the device with profiling on; every HG workspace tensor is read back (`hdrtv_get_tap`; each has its own slot), and
each launch is evaluated in float64 on the device's OWN input taps (tests/hg_layer_ref.py, on tests/le_layer_ref.py's machinery) --
exact f16 / fp32 values, so the error of the layers in front does not enter.  Per launch, output tensor, size and form:

    hard        |device - v| <= d at every element, d the a-priori bound derived from the launch's arithmetic -- not from anything
                measured.  hg.img and hg.mask have d = 0: bit for bit (no mask_r of the frames leaves a pixel to the fp32 arithmetic,
                tests/test_hg_layer_ref_host.py);
    precision   mean|device - v| <= 2 mean|model - v|, `model` the same graph with the roundings applied in float64 (fp32
                accumulation for the two fp32 outputs hg.part and hg.part2);
    inputs      at least 25 % of the output stands clear of the bound, |v| > 8 d (le_layer_ref.input_condition); for `final`, between
                10 % and 90 % of the device's mask are ones (mask_r is set per frame, hg_layer_ref.FRAMES);
    coverage    an hg.* / hg_* launch in the profile that no check claims fails the case (hg_layer_ref.plan).

DENSE ONLY: every case sets hg_sparse = 0 and asserts that the profile holds no hg_need launch -- with need lists hdrtv_get_tap re-runs
the head densely before it returns an hg.* tensor, and what is read is then not the frame's own launch.  The list-walking forms are
covered by transitivity: tests/test_gpu_hg_sparse*.py hold sparse == dense bit for bit.

Forms are variant settings (restored afterwards): `default` (prw = 1), `prw16` (prw = 2: conv_prw<pool, nhwc, ps, ps_dot3>), `prw8`
(prw = 3: conv_prw8<pool, nhwc, ps>), `pglds0` / `pglds1` (prw = 0 with pglds_nt_slow = 0 / 1: conv_pglds<..> in both tile orders),
`glds1_old` (the non-persistent 1x1 kernel; it exists in the A/B library only), `few16` / `few8` / `fewp` (prw = 2 / 3 / 0 with
force_ncu = 8, the smallest grid the persistent kernels take: several tiles per workgroup, the only regime in which the next-tile
prefetch and the hand-counted waits run at all).

Each case prints one line per output tensor:  max err/d, mean error of the device and of the model, share of the elements that are
bit-equal to the model, share with |v| > 8 d  (profiles/hg_layer_bounds.txt is such a run).  What the hard bound cannot see on a
frame -- the lo half of conv_prw<ps_dot3>'s weight pairs dropped -- is stated in tests/test_hg_layer_ref_host.py.
"""
import hashlib
import os

import pytest

import hg_layer_ref as H

pytestmark = pytest.mark.gpu

BASE = {"hg_sparse": 0, "prw": 1, "pglds_nt_slow": 3, "force_ncu": 0}
FORMS = {
    "default": {},
    "prw16": {"prw": 2},
    "prw8": {"prw": 3},
    "pglds0": {"prw": 0, "pglds_nt_slow": 0},
    "pglds1": {"prw": 0, "pglds_nt_slow": 1},
    "glds1_old": {"glds1_old": 1},
    "few16": {"prw": 2, "force_ncu": 8},
    "few8": {"prw": 3, "force_ncu": 8},
    "fewp": {"prw": 0, "force_ncu": 8},
}
PARTS = {(272, 480): 3}          # the float64 work of the largest size, split so that every case stays at a few seconds
SEEN = set()                     # kernel tags of every frame that ran


def _cases():
    out = []
    for size in H.FRAMES:
        for kind in ("noise", "gradient"):
            for form in FORMS:          # innermost: the forms of one frame share its float64 references (equal inputs, one evaluation)
                n = PARTS.get(size, 1)
                for part in range(n):
                    out.append(pytest.param(size, kind, form, part, n, id=f"{size[0]}x{size[1]}-{kind}-{form}" + (f"-{part + 1}of{n}" if n > 1 else "")))
    return out


class _Ctx:
    def __init__(self, golden_dir, hg_state):
        import torch
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
        self.golden_dir, self.hg_state = golden_dir, hg_state
        self.procs, self.saved = {}, {}
        self.key, self.frame = None, None
        self.refs_key, self.refs = None, {}

    def proc(self, ab):
        if ab not in self.procs:
            from hdrtv_mi355x.processor import HDRTVNetMI355X
            p = HDRTVNetMI355X(os.path.join(self.golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0,
                               _ab_library=ab)
            self.procs[ab] = p
            self.saved[ab] = {k: p.get_variant(k) for k in list(BASE) + ["glds1_old"]}
            assert all(self.saved[ab][k] == v for k, v in BASE.items() if k != "hg_sparse"), self.saved[ab]     # "untouched" is what BASE says
        return self.procs[ab]

    def close(self):
        for ab, p in self.procs.items():
            for k, v in self.saved[ab].items():
                p.set_variant(k, v)
            p.set_hg_mask_r(0.75)
            p.close()

    def run(self, size, kind, form):
        """One frame in one form -> (profile records, {logical tensor: float64 [C, H, W]}, mask_r); kept for the parts of a case."""
        if self.key != (size, kind, form):
            from hdrtv_mi355x import weights as W
            ab = "glds1_old" in FORMS[form]
            p = self.proc(ab)
            seed, r = H.FRAMES[size][kind == "gradient"]
            try:
                for k, v in {**BASE, **FORMS[form]}.items():
                    p.set_variant(k, v)
                p.set_hg_mask_r(r)
                p.profile_enable(True)
                try:
                    out, _ = p.infer(p.preprocess(W.synthetic_frame(*size, seed=seed, kind=kind)))
                    prof = p.profile_read()
                finally:
                    p.profile_enable(False)
                taps = {"out": out.float().cpu()[0].double()}
                for t, name in H.TAPS.items():
                    a = p.tap(name)
                    if t in ("part", "part2"):                   # [Hp][Wp][4] fp32, handed out as a flat [4, Hp, Wp] view
                        _, hp, wp = a.shape
                        a = a.reshape(hp, wp, 4).permute(2, 0, 1)[:3].contiguous()
                    taps[t] = a.double()
            finally:
                for k, v in self.saved[ab].items():
                    p.set_variant(k, v)
                p.set_hg_mask_r(0.75)
            SEEN.update(k for l, k, *_ in prof if l.startswith(("hg.", "hg_")))
            self.key, self.frame = (size, kind, form), (prof, taps, r)
        return self.frame

    def reference(self, size, kind, check, taps, r):
        """v / d / model of one launch on these input taps: computed once per distinct input (the forms of a frame mostly agree bit
        for bit in every tensor) and never changed."""
        if self.refs_key != (size, kind):
            self.refs_key, self.refs = (size, kind), {}
        h = hashlib.blake2b(digest_size=16)
        for t in check.ins:
            h.update(taps[t].numpy().tobytes())
        key = (check.name, h.hexdigest())
        if key not in self.refs:
            self.refs[key] = H.evaluate(check, H.pack(self.hg_state, mask_r=r), taps)
        return self.refs[key]


@pytest.fixture(scope="module")
def ctx(golden_dir, hg_state):
    c = _Ctx(golden_dir, hg_state)
    yield c
    c.close()


def _kernels(prof):
    return {l[3:]: k for l, k, *_ in prof if l.startswith("hg.")}


def _pins(form, prof):
    """The kernels a form is there for did run."""
    k = _kernels(prof)
    v = {**BASE, **FORMS[form]}
    big = [n for n, cout, _, _, ks, *_ in H.HG_LAYERS if ks == 3 and cout % 256 == 0]
    assert k["conv1"] == "conv_c3<64,dot3>" and all(k[n] == "conv_glds1" for n in ("conv6", "conv7", "conv8", "conv9")), k
    assert k["conv2"] == "conv_pglds<nhwc>", k
    if v["prw"] == 0:
        assert all(k[n].startswith("conv_pglds<") for n in big), k
    elif v["prw"] == 2:
        assert all(k[n].startswith("conv_prw<") for n in big), k
    elif v["prw"] == 3:
        assert all(k[n].startswith("conv_prw8<") for n in big if n != "Up_conv5") and k["Up_conv5"] == "conv_prw<ps_dot3>", k


@pytest.mark.parametrize("size,kind,form,part,nparts", _cases())
def test_every_hg_launch_against_its_float64_reference(ctx, size, kind, form, part, nparts):
    prof, taps, r = ctx.run(size, kind, form)
    assert not any(l == "hg_need" for l, *_ in prof)
    checks = H.plan(prof)                                        # coverage: every HG launch is claimed, none is a need-list launch
    assert len(checks) == len(H.STAGES)
    _pins(form, prof)
    on = float(taps["mask"][:, :size[0], :size[1]].mean())
    assert 0.1 <= on <= 0.9, ("the mask is no mixture", on)
    checks = H.split(checks, lambda t: taps[t].numel(), nparts)[part]
    failures = []
    for c in checks:
        for t, ref in ctx.reference(size, kind, c, taps, r).items():
            m = H.metrics(ref, taps[t])
            ok, share, _ = H.input_condition(ref)
            print(f"  {size[0]}x{size[1]} {kind:8s} {form:9s} {c.name:10s} {t:10s} n {m['n']:8d}  max err/d {m['max_ratio']:.3f}  "
                  f"mean dev {m['mean_err']:.3e} model {m['mean_model']:.3e}  bit-equal {m['bit_equal']:.4f}  clear {share:.2f}")
            if m["violations"]:
                failures.append((c.name, t, "hard", m["violations"], m["max_ratio"]))
            if m["mean_err"] > 2 * m["mean_model"]:
                failures.append((c.name, t, "precision", m["mean_err"], m["mean_model"]))
            if not ok and t not in H.EXACT:
                failures.append((c.name, t, "inputs", share))
    assert not failures, failures


def test_the_cases_cover_every_fp16_hg_kernel(ctx):
    """The union of the kernel tags over the forms holds every tag Seq::c3 and Seq::conv can emit for an fp16 head, and no other.
    (One 96 x 160 frame per form here, so that the test does not depend on which cases ran before it; the tags of those join in.)"""
    for form in FORMS:
        ctx.run((96, 160), "noise", form)
    print("\n  " + ", ".join(sorted(SEEN)))
    assert SEEN == set(H.KERNEL_TAGS), sorted(SEEN ^ set(H.KERNEL_TAGS))


@pytest.mark.parametrize("size", H.REFUSED)
def test_frames_the_reflect_padding_cannot_take_are_refused(ctx, size):
    """8 x 68 and 68 x 8 (the smallest frames without the head): padding to 32 rows needs 24 >= 8 rows of reflection, which F.pad
    refuses in the reference too -- HDRTV_EINVAL, and the context goes on working.  The smallest frames with a one-row / one-column
    level-5 map that the head does take, 17 x 68 and 68 x 17, are cases above."""
    import numpy as np
    from hdrtv_mi355x import lib as L
    p = ctx.proc(False)
    with pytest.raises(L.HdrtvError) as e:
        p.infer(p.preprocess(np.zeros(size + (3,), np.uint8)))
    assert f"({L.EINVAL})" in str(e.value) and "HG head's reflect padding" in str(e.value), str(e.value)
    ctx.key = None                                                # a frame of its own, not a kept one
    prof, _, _ = ctx.run((17, 68), "noise", "default")
    assert len(H.plan(prof)) == len(H.STAGES)
