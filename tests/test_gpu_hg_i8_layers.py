"""Every launch of the HG head's W8A8 path (BASELINE.json configs[4]) held ALONE to a float64 reference of the same operation.

One frame runs on the device with profiling on; every HG workspace tensor is read back (`hdrtv_get_tap`: the int8 code tensors are the
hg8.* taps, hg.part / hg.part2 fp32; each has its own slot), and each of the 21 launches is evaluated on the device's OWN input taps
(tests/hg_i8_layer_ref.py: read its docstring first) -- exact codes, so the integer sum of a layer is known exactly.  Per launch, output
tensor, calibration, size and form:

    hard        f16 / fp32 output (hg.img, hg.mask, hg.part2, hg.part, the output): |device - v| <= d at every element, d derived from
                the launch's arithmetic.  Code output: device code = model code EVERYWHERE, within 1 only at elements marked because the
                fp32 epilogue's span (contracted / uncontracted form) rounds to two codes; marked elements at most max(2, 1e-3 n); the
                folded form inside the network form's bound at every element (`fold`).  hg8.p1, the one quantiser behind f16 arithmetic
                of its own launch: the code between the codes of the two f16 values conv1's fp32 bound allows, the share of elements
                where these differ at most twice what that bound explains, plus 1e-3 (Q.cap_ok: wide_ok);
    precision   mean|device - v| <= 2 mean|model - v| (code tensors: in code units against v's float64 coordinate);
    inputs      f16 / fp32: |v| > 8 d at 25 % (H.input_condition); code tensor: 25 % of the codes strictly between the clamp and 255;
                final: the device's mask 10 .. 90 % ones;
    coverage    an hg.* / hg_* launch no check claims, a need-list launch or a kernel tag the layer cannot have fails (G.plan).

Calibrations: seeded-w8a8:1234 (integer zero points; delta is still used wherever k != 128), seeded-w8a8-minmax:1234 (float zero points
at the readers of conv6 .. conv9), and once, at 90x150 in the default form, the `odd` checkpoint of tests/test_gpu_int8_hg.py (Up_conv2.0's
x_zero moved by 0.4 steps: conv6 writes with the float rule into a tensor whose neighbours sit on the integer rule).
Sizes: hg_layer_ref.FRAMES with its seeds and mask_r -- 17x68 / 68x17 (level-5 maps 1x3 / 3x1: both bits of a class axis set, the 8-row
and 16-row tiles almost empty), 90x150 (reflect padding, crop, W & 3 != 0), 96x160, 272x480 (default and few-workgroup forms, in parts).
Forms (variants, restored afterwards): `default` (prw = 1, prw_i8 = 1), `prw16` (prw = 2, prw_i8 = 2), `prw8` (prw = 3, prw_i8 = 2),
`pglds` (prw = 0), and the last three with force_ncu = 8 (`few16`, `few8`, `fewp`: several tiles per workgroup).  prw = 2 / 3 force the
16-row / 8-row tiles at every size; in the `default` form prw_i8 = 1 never takes 16-row tiles by construction and takes the 8-row ones
only where Seq::prw_rows prefers them (pinned below: which layers did is printed by the coverage test).  Forms of one frame share their
references, keyed by a hash of the input taps.

Each case prints one line per output tensor: max err/d, mean error of the device and of the model, bit-equal share, marked (or, hg8.p1,
widened) share, clear / in-range share, fold violations (profiles/hg_i8_layer_bounds.txt is such a run).
"""
import hashlib
import os

import numpy as np
import pytest

import hg_i8_layer_ref as G

pytestmark = pytest.mark.gpu

BASE = {"hg_sparse": 0, "prw": 1, "prw_i8": 1, "force_ncu": 0}
FORMS = {
    "default": {},
    "prw16": {"prw": 2, "prw_i8": 2},
    "prw8": {"prw": 3, "prw_i8": 2},
    "pglds": {"prw": 0},
    "few16": {"prw": 2, "prw_i8": 2, "force_ncu": 8},
    "few8": {"prw": 3, "prw_i8": 2, "force_ncu": 8},
    "fewp": {"prw": 0, "force_ncu": 8},
}
BIG = (272, 480)
BIG_FORMS = ("default", "few16", "few8", "fewp")
PARTS = {BIG: 4}                 # the float64 work of the largest size, split so that every case stays at a few seconds
ODD = ("odd", (90, 150), "gradient", "default")
SEEN = {}                        # calibration -> kernel tags of every frame that ran


def _cases():
    out = []
    for cal in G.CALIBRATIONS:
        for size in G.FRAMES:
            for kind in ("noise", "gradient"):
                for form in (BIG_FORMS if size == BIG else FORMS):          # innermost: the forms of one frame share its references
                    n = PARTS.get(size, 1)
                    for part in range(n):
                        out.append(pytest.param(cal, size, kind, form, part, n,
                                                id=f"{cal}-{size[0]}x{size[1]}-{kind}-{form}" + (f"-{part + 1}of{n}" if n > 1 else "")))
    out.append(pytest.param(*ODD, 0, 1, id="odd-90x150-gradient-default"))
    return out


def _qstate(cal):
    from hdrtv_mi355x import weights as W
    sd = W.seeded_hg_w8a8_state(1234, integer_zero=cal != "minmax")
    if cal == "odd":
        sd = dict(sd)
        sd["Up_conv2.0.x_zero"] = np.array(float(sd["Up_conv2.0.x_zero"]) + 0.4 * float(sd["Up_conv2.0.x_scale"]), np.float32)
    return sd


class _Ctx:
    def __init__(self, golden_dir, cal):
        import torch
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
        from hdrtv_mi355x.processor import HDRTVNetMI355X
        self.cal = cal
        sd = _qstate(cal)
        self.p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights=G.CALIBRATIONS.get(cal, sd), warmup_passes=0)
        assert self.p._hg_int8
        self.saved = {k: self.p.get_variant(k) for k in BASE}
        assert all(self.saved[k] == v for k, v in BASE.items() if k != "hg_sparse"), self.saved          # "untouched" is what BASE says
        self.P = G.pack(sd)
        self.key, self.frame = None, None
        self.refs_key, self.refs = None, {}

    def close(self):
        for k, v in self.saved.items():
            self.p.set_variant(k, v)
        self.p.set_hg_mask_r(0.75)
        self.p.close()

    def run(self, size, kind, form):
        """One frame in one form -> (profile records, {logical tensor: float64 [C, H, W]}, mask_r); kept for the parts of a case."""
        if self.key != (size, kind, form):
            from hdrtv_mi355x import weights as W
            p = self.p
            seed, r = G.FRAMES[size][kind == "gradient"]
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
                for t, name in G.TAPS.items():
                    a = p.tap(name)
                    if t in ("part", "part2"):                   # [Hp][Wp][4] fp32, handed out as a flat [4, Hp, Wp] view
                        _, hp, wp = a.shape
                        a = a.reshape(hp, wp, 4).permute(2, 0, 1)[:3].contiguous()
                    taps[t] = a.double()
            finally:
                for k, v in self.saved.items():
                    p.set_variant(k, v)
                p.set_hg_mask_r(0.75)
            SEEN.setdefault(self.cal, set()).update(k for l, k, *_ in prof if l.startswith(("hg.", "hg_")))
            self.key, self.frame = (size, kind, form), (prof, taps, r)
        return self.frame

    def reference(self, size, kind, check, taps, r):
        """The results of one launch on these input taps: computed once per distinct input (the forms of a frame agree bit for bit in
        every tensor unless something is wrong) and never changed."""
        if self.refs_key != (size, kind):
            self.refs_key, self.refs = (size, kind), {}
        h = hashlib.blake2b(digest_size=16)
        for t in check.ins:
            h.update(taps[t].numpy().tobytes())
        key = (check.name, h.hexdigest())
        if key not in self.refs:
            self.refs[key] = G.evaluate(check, self.P.with_mask_r(r), taps)
        return self.refs[key]


_CTX = {}


@pytest.fixture(scope="module")
def ctxs(golden_dir):
    def get(cal):
        if cal not in _CTX:
            _CTX[cal] = _Ctx(golden_dir, cal)
        return _CTX[cal]
    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _kernels(prof):
    return {l[3:]: k for l, k, *_ in prof if l.startswith("hg.")}


def _pins(form, prof):
    """The kernels a form is there for did run."""
    k = _kernels(prof)
    v = {**BASE, **FORMS[form]}
    assert k["conv1"] == "conv_c3<64,dot3>" and all(k[n] == "conv1x1_i8" for n in ("conv6", "conv7", "conv8", "conv9")), k
    assert k["conv2"] == "conv_pglds_i8<nhwc,c64>" and k["Up_conv5"] == "conv_pglds_i8<ps_dot3,c64>", k
    if v["prw"] == 0:
        assert all(k[n].startswith("conv_pglds_i8<") for n in G.PRW_LAYERS), k
    elif v["prw"] == 2:
        assert all(k[n].startswith("conv_prw_i8<") for n in G.PRW_LAYERS), k
    elif v["prw"] == 3:
        assert all(k[n].startswith("conv_prw8_i8<") for n in G.PRW_LAYERS), k
    else:                        # prw_i8 = 1: the 8-row tiles where Seq::prw_rows prefers them, never the 16-row ones
        assert not any(k[n].startswith("conv_prw_i8<") for n in G.PRW_LAYERS), k


@pytest.mark.parametrize("cal,size,kind,form,part,nparts", _cases())
def test_every_w8a8_hg_launch_against_its_float64_reference(ctxs, cal, size, kind, form, part, nparts):
    ctx = ctxs(cal)
    prof, taps, r = ctx.run(size, kind, form)
    assert not any(l == "hg_need" for l, *_ in prof)
    checks = G.plan(prof)                                        # coverage: every HG launch is claimed, every tag is one the layer can have
    assert len(checks) == len(G.STAGES) == 21
    _pins(form, prof)
    on = float(taps["mask"][:, :size[0], :size[1]].mean())
    assert 0.1 <= on <= 0.9, ("the mask is no mixture", on)
    checks = G.split(checks, lambda t: taps[t].numel(), nparts)[part]
    failures = []
    for c in checks:
        res, marks = ctx.reference(size, kind, c, taps, r)
        cap, worst, wide, wide_ok = G.cap_ok(marks)
        if not cap:
            failures.append((c.name, "marked", marks))
        if not wide_ok:
            failures.append((c.name, "wide", marks))
        for t, ref in res.items():
            m = G.metrics(ref, taps[t])
            ok, share = G.input_ok(t, ref)
            print(f"  {cal:7s} {size[0]}x{size[1]} {kind:8s} {form:7s} {c.name:10s} {t:10s} {'codes' if ref['codes'] else 'float'} n {m['n']:8d}  "
                  f"max err/d {m['max_ratio']:.3f}  mean dev {m['mean_err']:.3e} model {m['mean_model']:.3e}  bit-equal {m['bit_equal']:.5f}  "
                  f"marked {worst:.1e}  wide {wide:.1e}  clear {share:.2f}  fold {ref['fold']}")
            if m["violations"]:
                failures.append((c.name, t, "hard", m["violations"], m["max_ratio"]))
            if ref["fold"]:
                failures.append((c.name, t, "fold", ref["fold"]))
            if m["mean_err"] > 2 * m["mean_model"]:
                failures.append((c.name, t, "precision", m["mean_err"], m["mean_model"]))
            if not ok:
                failures.append((c.name, t, "inputs", share))
    assert not failures, failures


def test_the_cases_cover_every_w8a8_hg_kernel_and_the_both_bits_classes(ctxs):
    """The union of the kernel tags over the forms is every tag Seq::c3 and Seq::conv8 can emit for this head's table, and no other, in
    BOTH calibrations (conv1x1_i8<f16> is not among them: every 1x1 layer has an int8 reader, G's docstring); and the both-bits border classes (one-row and one-column level-5 maps) ran in both, in every form.  (One frame
    per form and small size here, so that the test does not depend on which cases ran before it; their tags join in.)  Printed: the
    layers the `default` form gave 8-row tiles at each size."""
    for cal in G.CALIBRATIONS:
        ctx = ctxs(cal)
        for size in ((17, 68), (68, 17)):
            hp, wp = -(-size[0] // 32), -(-size[1] // 32)
            assert 1 in (hp, wp) and {c for c in G.border_classes(hp, wp, 3, 1).reshape(-1).tolist()} & {3, 7, 11, 12, 13, 14, 15}
            for form in FORMS:
                prof, _, _ = ctx.run(size, "noise", form)
                _pins(form, prof)
        for size in ((17, 68), (96, 160)):
            k = _kernels(ctx.run(size, "noise", "default")[0])
            print(f"\n  {cal} {size[0]}x{size[1]} default: 8-row tiles at {[n for n in G.PRW_LAYERS if k[n].startswith('conv_prw8_i8<')]}")
        for form in FORMS:
            ctx.run((96, 160), "noise", form)
        print("  " + ", ".join(sorted(SEEN[cal])))
        assert SEEN[cal] == set(G.KERNEL_TAGS), (cal, sorted(SEEN[cal] ^ set(G.KERNEL_TAGS)))


@pytest.mark.parametrize("size", G.REFUSED)
def test_frames_the_reflect_padding_cannot_take_are_refused_by_an_int8_context(ctxs, size):
    """8 x 68 and 68 x 8: padding to 32 rows needs 24 >= 8 rows of reflection -- HDRTV_EINVAL from a W8A8 context too, and the context
    then runs 17 x 68."""
    from hdrtv_mi355x import lib as L
    ctx = ctxs("integer")
    with pytest.raises(L.HdrtvError) as e:
        ctx.p.infer(ctx.p.preprocess(np.zeros(size + (3,), np.uint8)))
    assert f"({L.EINVAL})" in str(e.value) and "HG head's reflect padding" in str(e.value), str(e.value)
    ctx.key = None                                                # a frame of its own, not a kept one
    prof, _, _ = ctx.run((17, 68), "noise", "default")
    assert len(G.plan(prof)) == len(G.STAGES)
