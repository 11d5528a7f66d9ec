"""Every launch of the LE network's W8A8 path held ALONE to a float64 reference of the same operation (tests/le_i8_layer_ref.py).

One frame per case runs on the device with the shipped QAT checkpoints kept quantised (precision = "int8-<recipe>", predequantize
off); every workspace tensor is read back (`hdrtv_get_tap`; int8 code tensors are the le8.* taps) and each launch is evaluated on
the device's OWN input taps.  Per launch and output tensor:

    hard        f16 output: |device - v| <= d at every element, d the a-priori bound (a few fp32 ulps + half an f16 ulp per f16
                rounding + |w| step for every input code that is not determined); code output: device code = model code everywhere,
                within 1 at marked elements only;
    precision   mean|device - v| <= 2 mean|model - v| (for a code tensor: in code units, against the float64 coordinate);
    inputs      le_layer_ref.input_condition as it is -- but at the four launches le_i8_layer_ref.WAIVED names, each with its reason, where
                it is asked at factor 1 instead of 8, and at R's own exemption, the six-launch composite; the marked share of every capped
                quantiser at most max(2 elements, 1e-3) per tensor; the widened share of every uncapped one at most twice what its d
                explains (le_i8_layer_ref.cap_ok).

Forms: `layers` -- le_rows = le_rows_i8 = le_rows_fq = cond2_fused = cond3_fused = 0, no_c3fuse = 1: every launch alone but where the
frame overwrites its intermediate; for the full recipe once more with no_c3q8 = 1 (planar3_to_q8 + the generic conv_q8 for conv_first).
`default` (variants untouched) and `short` (le_rows_min = 1, at the three even sizes) of the full recipe are not a second reference:
every tap both forms write must be torch.equal to the `layers` run, which carries the per-launch result to le_head_rows<i8>,
le_rb_rows<i8> and le_tail_rows<i8> where they run.

Each case prints one line per output tensor: max err/d, mean error of the device and of the model, share bit-equal to the model,
share clear of the bound (|v| > 8 d), worst marked share of a capped quantiser, worst share of a widened uncapped one
(profiles/le_i8_layer_bounds.txt is such a run).
"""
import os

import pytest
import torch

import le_i8_layer_ref as Q
import le_layer_ref as R

pytestmark = pytest.mark.gpu

LAYERS = {"le_rows": 0, "le_rows_i8": 0, "le_rows_fq": 0, "cond2_fused": 0, "cond3_fused": 0, "no_c3fuse": 1, "no_c3q8": 0, "le_rows_min": 8}
DEFAULT = {"le_rows": 1, "le_rows_i8": 1, "le_rows_fq": 1, "cond2_fused": 1, "cond3_fused": 1, "no_c3fuse": 0, "no_c3q8": 0, "le_rows_min": 8}
# short: le_rows_min = 1 takes the row kernels to these small sizes (tests/test_gpu_le_layers.py's form of the same name)
FORMS = {"layers": LAYERS, "c3generic": dict(LAYERS, no_c3q8=1), "default": DEFAULT, "short": dict(DEFAULT, le_rows_min=1)}
PARTS = {(270, 486): 6}          # the float64 work of the largest size, split so that every case stays at a few seconds


def _cases():
    out = []
    for recipe in Q.RECIPES:
        for size in R.FRAMES:
            for kind in ("noise", "gradient"):
                n = PARTS.get(size, 1)
                for part in range(n):
                    out.append(pytest.param(recipe, size, kind, "layers", part, n,
                                            id=f"{recipe}-{size[0]}x{size[1]}-{kind}-layers" + (f"-{part + 1}of{n}" if n > 1 else "")))
    out.append(pytest.param("full", (61, 103), "gradient", "c3generic", 0, 1, id="full-61x103-gradient-c3generic"))
    return out


class _Ctx:
    def __init__(self, golden_dir, recipe):
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
        from hdrtv_mi355x import weights as W
        from hdrtv_mi355x.processor import HDRTVNetMI355X
        path = os.path.join(golden_dir, Q.RECIPES[recipe])
        self.p = HDRTVNetMI355X(path, precision=f"int8-{recipe}", predequantize="off", use_hg=False, warmup_passes=0)
        for k, v in DEFAULT.items():
            assert self.p.get_variant(k) == v, (k, self.p.get_variant(k))         # "variants untouched" is what DEFAULT says it is
        self.P = Q.pack(W.load_pack(path))
        self.T = Q.taps_of(self.P)
        self.key, self.frame = None, None

    def run(self, size, kind, form):
        """One frame in one form -> (profile records, {logical tensor: float64 [C, H, W]}, {tap: raw tensor}); kept for the parts."""
        if self.key != (size, kind, form):
            from hdrtv_mi355x import weights as W
            p = self.p
            for k, v in FORMS[form].items():
                p.set_variant(k, v)
            f = W.synthetic_frame(*size, seed=R.FRAMES[size][kind == "gradient"], kind=kind)
            p.profile_enable(True)
            out, agcm = p.infer(p.preprocess(f))
            prof = p.profile_read()
            p.profile_enable(False)
            raw = {"agcm": agcm.float().cpu()[0], "out": out.float().cpu()[0]}
            taps = {"agcm": raw["agcm"].double(), "out": raw["out"].double()}
            for t, (name, ch) in self.T.items():
                if name not in raw:
                    raw[name] = p.tap(name)
                a = raw[name].double()
                taps[t] = a if ch is None else a[ch[0]:ch[1]].contiguous()
            self.key, self.frame = (size, kind, form), (prof, taps, raw)
        return self.frame


_CTX = {}


@pytest.fixture(scope="module")
def ctxs(golden_dir):
    def get(recipe):
        if recipe not in _CTX:
            _CTX[recipe] = _Ctx(golden_dir, recipe)
        return _CTX[recipe]
    yield get
    for c in _CTX.values():
        c.p.close()
    _CTX.clear()


@pytest.mark.parametrize("recipe,size,kind,form,part,nparts", _cases())
def test_every_w8a8_le_launch_against_its_float64_reference(ctxs, recipe, size, kind, form, part, nparts):
    ctx = ctxs(recipe)
    prof, taps, _ = ctx.run(size, kind, form)
    kernels = {k for l, k, *_ in prof if l.startswith(("LE.", "le."))}
    assert not {k for k in kernels if "rows" in k or "+tail" in k or "c3+" in k}, kernels
    want = set(Q.TAGS[recipe])
    if form == "c3generic":
        want = (want - {"conv_c3_q8"}) | {"planar3_to_q8", "conv_q8<32,3,1>"}
    assert want <= kernels, sorted(want - kernels)
    checks = Q.plan(prof, ctx.P, no_c3q8=form == "c3generic")
    assert sorted(c.name for c in checks if c.composite) == ["rt1a+rt1b", "rt2a+rt2b", "rt30a..rt32b"]
    if form == "c3generic":          # the rest of the frame is the `layers` case's
        checks = [c for c in checks if c.name in ("img32", "f0a")]
    checks = R.split(checks, lambda t: taps[t].numel(), nparts)[part]
    failures = []
    for c in checks:
        res, marks = Q.evaluate(c, ctx.P, taps)
        cap, worst, wide, wide_ok = Q.cap_ok(marks)
        if not cap:
            failures.append((c.name, "marked", [(l, m, n) for l, m, n, k, _ in marks if k and m > max(Q.CAP_MIN, Q.CAP_SHARE * n)]))
        if not wide_ok:
            failures.append((c.name, "wide", [(l, m / n, e) for l, m, n, k, e in marks if not k]))
        for t, r in res.items():
            m = R.metrics(r, taps[t])
            ok, share, asked = Q.input_ok(c, r)
            print(f"  {recipe:5s} {size[0]}x{size[1]} {kind:8s} {form:9s} {c.name:14s} {t:6s} {'codes' if r['codes'] else 'f16  '} n {m['n']:8d}  "
                  f"max err/d {m['max_ratio']:.3f}  mean dev {m['mean_err']:.3e} model {m['mean_model']:.3e}  bit-equal {m['bit_equal']:.5f}  "
                  f"clear {share:.2f}  marked {worst:.1e}  wide {wide:.1e}")
            if m["violations"]:
                failures.append((c.name, t, "hard", m["violations"], m["max_ratio"]))
            if m["mean_err"] > 2 * m["mean_model"]:
                failures.append((c.name, t, "precision", m["mean_err"], m["mean_model"]))
            if not ok:
                failures.append((c.name, t, "inputs", share, asked))
    assert not failures, failures


def _identity_cases():
    return [pytest.param(size, kind, form, id=f"{size[0]}x{size[1]}-{kind}-{form}") for size in R.FRAMES for form in ("default", "short")
            if form == "default" or size in R.SHORT for kind in ("noise", "gradient")]


def _written(P, prof):
    """The taps a frame's launches write, from its profile: a per-layer launch writes its stage's outputs (le_i8_layer_ref.stages), a row
    kernel the tensors that leave its LDS rings.  A launch the table does not know fails."""
    by_key = {}
    for st in Q.stages(P):
        by_key.setdefault(st.key, []).extend(st.outs)
    fused = {"LE.head": ["fea0", "fea1a"], "LE.tail": ["out"]}
    for st in Q.stages(P):
        if st.key.endswith(".conv2") and ".recon_trunk" in st.key:
            fused[st.key[:-len(".conv2")]] = list(st.outs)          # le_rb_rows: the block's output only
    T, names = Q.taps_of(P), set()
    for l, *_ in prof:
        if not l.startswith(("LE.", "le.")):
            continue
        assert l in by_key or l in fused, ("a launch this test does not know", l)
        for t in (fused[l] if l in fused else by_key[l]):
            if t == "out":
                names.add("out")
            elif t in T:
                names.add(T[t][0])
    return names


@pytest.mark.parametrize("size,kind,form", _identity_cases())
def test_the_shipped_forms_are_the_per_layer_form_bit_for_bit(ctxs, size, kind, form):
    """Full recipe, `default` (variants untouched) and `short` (le_rows_min = 1): every tap the form's own launches write (read off its
    profile, so a tap that merely still holds the per-layer run's bytes is not compared) is torch.equal to the per-layer run the test
    above holds launch by launch, and the int8 row kernels ran exactly where they should -- this carries the per-launch result to
    le_head_rows<i8>, le_rb_rows<i8> and le_tail_rows<i8>.  (The fused CondNet tails are fp16 forms: cond2_fused and
    cond3_fused never engage for this recipe, api_graph.hip `!c->tail_q8` / `!isq8`.)"""
    ctx = ctxs("full")
    prof_l, _, raw_l = ctx.run(size, kind, "layers")
    prof, _, raw_d = ctx.run(size, kind, form)
    kernels = {k for l, k, *_ in prof if l.startswith(("LE.", "le."))}
    rows = {"le_head_rows<i8>", "le_rb_rows<i8>", "le_tail_rows<i8>"}
    if form == "short":
        assert rows <= kernels, kernels
    elif size == (270, 486):         # le_rows_min = 8: the full-resolution head and tail (10 rows per segment), no ResBlock (3 rows)
        assert rows & kernels == {"le_head_rows<i8>", "le_tail_rows<i8>"}, kernels
    else:                            # odd, narrower than one strip, or one or two rows per segment: no row kernel at le_rows_min = 8
        assert not (rows & kernels), kernels
    assert not {k for k in kernels if "<fq>" in k or "+tail" in k}, kernels
    written = _written(ctx.P, prof)
    every = _written(ctx.P, prof_l)
    assert written <= every == (set(raw_l) - {"agcm", "le8.img32"}), (sorted(every ^ set(raw_l)), sorted(written - every))
    assert {"le.cond", "le.cond1", "le.cond2", "le.cond3", "le.cond4", "le.fea0", "le.fea1a", "le.fea1", "le.fea2", "le.fea3", "le.t3y", "le.t4",
            "le.t5", "out"} <= written, sorted(written)
    if not (rows & kernels):
        assert written == every
    for name in sorted(written):
        assert torch.equal(raw_l[name], raw_d[name]), (form, name, float((raw_l[name] - raw_d[name]).abs().max()))
