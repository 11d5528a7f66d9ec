"""Every launch of the LE network's fp16 path held ALONE to a float64 reference of the same operation.

One frame runs on the device; every workspace tensor is read back (`hdrtv_get_tap`), and each launch is evaluated in float64 on the
device's OWN input taps (tests/le_layer_ref.py) -- exact f16 values, so the error of the layers in front does not enter.  Per
launch, output tensor and size:

    hard        |device - v| <= d at every element, d the a-priori bound derived from the launch's arithmetic (fp16 roundings where
                the kernel performs them, fp32 accumulation) -- not from anything measured;
    precision   mean|device - v| <= 2 mean|model - v|, `model` the same graph with the fp16 roundings applied in float64: the device
                and the model round at the same points and differ in accumulation order only;
    inputs      enough of the output stands clear of the bound for the comparison to mean something (le_layer_ref.input_condition).

Forms: `layers` -- every fusion off (le_rows = 0, cond2_fused = 0, cond3_fused = 0, no_c3fuse = 1): each launch's input and output
exist, every launch is checked alone (le_layer_ref's docstring lists them and the few that cannot be); `default` -- the variants
untouched; `short` -- le_rows_min = 1, which takes the row kernels to these small sizes.  A fused launch is checked as the longer
primitive list of the launches it replaces; which launches ran is read off the frame's profile, and a launch that no check claims
fails the test (le_layer_ref.plan).  tests/test_le_layer_ref_host.py shows what these comparisons catch.

Each case prints one line per output tensor:  max err/d, mean error of the device and of the model, share of the elements that are
bit-equal to the model, share with |v| > 8 d  (profiles/le_layer_bounds.txt is such a run).
"""
import os

import pytest

import le_layer_ref as R

pytestmark = pytest.mark.gpu

FORMS = {
    "layers": {"le_rows": 0, "cond2_fused": 0, "cond3_fused": 0, "no_c3fuse": 1, "le_rows_min": 8},
    "default": {"le_rows": 1, "cond2_fused": 1, "cond3_fused": 1, "no_c3fuse": 0, "le_rows_min": 8},
    "short": {"le_rows": 1, "cond2_fused": 1, "cond3_fused": 1, "no_c3fuse": 0, "le_rows_min": 1},
}
PARTS = {(270, 486): 3}          # the float64 work of the largest size, split so that every case stays at a few seconds


def _cases():
    out = []
    for size in R.FRAMES:
        for form in FORMS:
            if form == "short" and size not in R.SHORT:
                continue
            for kind in ("noise", "gradient"):
                n = PARTS.get(size, 1)
                for part in range(n):
                    out.append(pytest.param(size, kind, form, part, n, id=f"{size[0]}x{size[1]}-{kind}-{form}" + (f"-{part + 1}of{n}" if n > 1 else "")))
    return out


class _Ctx:
    def __init__(self, golden_dir, hr_state):
        import torch
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
        from hdrtv_mi355x.processor import HDRTVNetMI355X
        self.p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
        for k, v in FORMS["default"].items():
            assert self.p.get_variant(k) == v, (k, self.p.get_variant(k))         # "variants untouched" is what FORMS says it is
        self.P = R.pack(hr_state)
        self.key, self.frame = None, None

    def run(self, size, kind, form):
        """One frame in one form -> (profile records, {logical tensor: float64 [C, H, W]}); kept for the parts of a case."""
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
            taps = {"agcm": agcm.float().cpu()[0].double(), "out": out.float().cpu()[0].double()}
            raw = {}
            for t, (name, ch) in R.TAPS.items():
                if name not in raw:
                    raw[name] = p.tap(name).double()
                taps[t] = raw[name] if ch is None else raw[name][ch[0]:ch[1]].contiguous()
            self.key, self.frame = (size, kind, form), (prof, taps)
        return self.frame


@pytest.fixture(scope="module")
def ctx(golden_dir, hr_state):
    c = _Ctx(golden_dir, hr_state)
    yield c
    c.p.close()


@pytest.mark.parametrize("size,kind,form,part,nparts", _cases())
def test_every_le_launch_against_its_float64_reference(ctx, size, kind, form, part, nparts):
    prof, taps = ctx.run(size, kind, form)
    kernels = {k for l, k, *_ in prof if l.startswith(("LE.", "le."))}
    fused = {k for k in kernels if "rows" in k or "+tail" in k or "c3+" in k}
    if form == "layers":
        assert not fused, fused
    else:
        assert {"conv3x3s2_preg<192>+tail", "conv3x3s2_preg<64>+tail"} <= kernels, kernels
    if form == "short":
        assert {"le_head_rows", "le_rb_rows", "le_tail_rows"} <= kernels, kernels
    checks = R.plan(prof)
    if form == "layers":          # every launch alone, but where the frame overwrites its intermediate
        assert sorted(c.name for c in checks if c.composite) == ["rt1a+rt1b", "rt2a+rt2b", "rt30a..rt32b"]
    checks = R.split(checks, lambda t: taps[t].numel(), nparts)[part]
    failures = []
    for c in checks:
        for t, r in R.evaluate(c, ctx.P, taps).items():
            m = R.metrics(r, taps[t])
            ok, share, _ = R.input_condition(r)
            print(f"  {size[0]}x{size[1]} {kind:8s} {form:7s} {c.name:16s} {t:6s} n {m['n']:8d}  max err/d {m['max_ratio']:.3f}  "
                  f"mean dev {m['mean_err']:.3e} model {m['mean_model']:.3e}  bit-equal {m['bit_equal']:.4f}  clear {share:.2f}")
            if m["violations"]:
                failures.append((c.name, t, "hard", m["violations"], m["max_ratio"]))
            if m["mean_err"] > 2 * m["mean_model"]:
                failures.append((c.name, t, "precision", m["mean_err"], m["mean_model"]))
            if not ok and not c.extra:
                failures.append((c.name, t, "inputs", share))
    assert not failures, failures
