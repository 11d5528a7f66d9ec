"""Every launch of the AGCM front end's fp16 path held ALONE to a float64 reference of the same operation.

One frame runs on the device with profiling on; every AGCM workspace tensor is read back (`hdrtv_get_tap`: agcm.u1..5, mean1..5,
rstd1..5, part, frags as raw f16 bits, bias; the preprocess tensors and agcm_out), and each of the twelve launches (5 x cls_block,
5 x cls_stats, agcm_fold, agcm_mlp) is evaluated in float64 on the device's OWN input bits (tests/agcm_layer_ref.py), so the error
of the launches in front does not enter.  Per launch and output tensor:

    hard        |device - v| <= d at every element, d the a-priori bound derived from the launch's arithmetic -- not from anything
                measured; d = 0 (device == v exactly) at the fragment slots and bias rows the layout leaves empty;
    precision   mean|device - v| <= 2 mean|model - v|, `model` the same launch with roundings where the kernel rounds (plain
                equality where the model reproduces v exactly);
    inputs      enough of the output stands clear of the bound for the comparison to mean something (le_layer_ref.input_condition,
                asked of every output: none is exempted).

Which launches ran is read off the frame's profile; an AGCM launch that no check claims fails the test (agcm_layer_ref.plan).  The
profile names only `cls_block`, so the kernel form each case is there for (PX = 16 above 4096 output pixels, f16 input for block 1
and f32 with InstanceNorm on load behind it) is asserted from the sizes of the maps the device hands back and the launcher's rule.
The sizes and what each is for: agcm_layer_ref.FRAMES.  The MLP is evaluated at ALL pixels (share 1.0) at every size; at the two
large ones the pixels are split over the parts of a case (PARTS).
tests/test_agcm_layer_ref_host.py shows what these comparisons catch.

Each case prints one line per output tensor:  max err/d, mean error of the device and of the model, share of the elements that are
bit-equal to the model, share with |v| > 8 d  (profiles/agcm_layer_bounds.txt is such a run).
"""
import os

import pytest

import agcm_layer_ref as R

pytestmark = pytest.mark.gpu


# The float64 work of the MLP at the two large sizes, split over the pixels so that every case stays at a few seconds: part k of n
# evaluates pixels [k N / n, (k + 1) N / n) -- the parts together ALL pixels, the final partial group included -- and part 0 the
# eleven launches in front of the MLP as well.
PARTS = {(520, 1016): 2, (1036, 1076): 3}


def _cases():
    out = []
    for size in R.FRAMES:
        for kind in ("noise", "gradient"):
            n = PARTS.get(size, 1)
            for part in range(n):
                out.append(pytest.param(size, kind, False, part, n, id=f"{size[0]}x{size[1]}-{kind}" + (f"-{part + 1}of{n}" if n > 1 else "")))
    # run_agcm is shared with the HG build, whose workspace is laid out differently around it
    return out + [pytest.param(R.HG_FRAME, kind, True, 0, 1, id=f"{R.HG_FRAME[0]}x{R.HG_FRAME[1]}-{kind}-hg") for kind in ("noise", "gradient")]


class _Ctx:
    def __init__(self, golden_dir, hr_state):
        import torch
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
        self.golden_dir, self.procs = golden_dir, {}
        self.P = R.pack(hr_state)
        self.key, self.frame = None, None

    def proc(self, hg):
        if hg not in self.procs:
            from hdrtv_mi355x.processor import HDRTVNetMI355X
            kw = {"use_hg": True, "hg_weights": "seeded:1234"} if hg else {"use_hg": False}
            self.procs[hg] = HDRTVNetMI355X(os.path.join(self.golden_dir, "hr_weights.hdrw"), warmup_passes=0, **kw)
        return self.procs[hg]

    def run(self, size, kind, hg):
        """One frame -> (profile records, {logical tensor: float64}); kept for the parts of a case."""
        if self.key != (size, kind, hg):
            self.key, self.frame = (size, kind, hg), self._run(size, kind, hg)
        return self.frame

    def _run(self, size, kind, hg):
        import torch
        from hdrtv_mi355x import weights as W
        p = self.proc(hg)
        f = W.synthetic_frame(*size, seed=R.FRAMES[size][kind == "gradient"], kind=kind)
        p.profile_enable(True)
        tensor, cond = p.preprocess(f)
        _, agcm = p.infer((tensor, cond))
        prof = p.profile_read()
        p.profile_enable(False)
        d = lambda t: t.float().cpu().double()
        taps = {"rgb": d(tensor)[0], "cond": d(cond)[0], "out": d(agcm)[0]}
        for i in range(1, 6):
            taps[f"u{i}"] = p.tap(f"agcm.u{i}").double()
            taps[f"mean{i}"] = p.tap(f"agcm.mean{i}").double().reshape(-1)
            taps[f"rstd{i}"] = p.tap(f"agcm.rstd{i}").double().reshape(-1)
        n5 = taps["u5"].shape[1] * taps["u5"].shape[2]
        # block 5's partials, read with the launcher's nblk: [co][nblk] float2
        taps["part5"] = p.tap("agcm.part").double().reshape(-1)[:2 * 128 * R.nblk_of(n5)].reshape(128, R.nblk_of(n5), 2)
        # f16 elements in an f32-sized slot: the raw bits
        taps["frags"] = p._tap_device("agcm.frags").view(torch.float16).float().cpu().double().reshape(R.NFRAG, 64, 8)
        bias = p.tap("agcm.bias").double().reshape(-1)
        taps["bias"], taps["fea6"] = bias[:160].contiguous(), bias[160:166].contiguous()
        return prof, taps


@pytest.fixture(scope="module")
def ctx(golden_dir, hr_state):
    c = _Ctx(golden_dir, hr_state)
    yield c
    for p in c.procs.values():
        p.close()


@pytest.mark.parametrize("size,kind,hg,part,nparts", _cases())
def test_every_agcm_launch_against_its_float64_reference(ctx, size, kind, hg, part, nparts):
    prof, taps = ctx.run(size, kind, hg)
    # the case ran the kernel forms it is there for: the maps the device hands back are shapes_for's, and the launcher's rule on them
    maps = R.maps_for(*size)
    assert tuple(taps["cond"].shape[1:]) == maps[0] and tuple(taps["rgb"].shape[1:]) == size
    assert [tuple(taps[f"u{i}"].shape) for i in range(1, 6)] == [(R.CLS_CO[i - 1],) + maps[i] for i in range(1, 6)]
    assert tuple(R.px_of(h * w) for h, w in maps[1:]) == R.FORMS[size]
    agcm = [(l, k) for l, k, *_ in prof if l.startswith(("cls", "agcm")) or k.startswith(("cls", "agcm"))]
    assert agcm == [("cls_block", "cls_block"), ("cls_stats", "cls_stats")] * 5 + [("agcm_fold", "agcm_fold"), ("agcm_mlp", "agcm_mlp")], agcm
    checks = R.plan(prof)
    assert sorted(c.launch for c in checks) == list(range(12))
    tag = f"{size[0]}x{size[1]} {kind:8s}" + (" hg" if hg else "") + (f" {part + 1}/{nparts}" if nparts > 1 else "")
    if nparts > 1:
        npix = size[0] * size[1]
        a, b = part * npix // nparts, (part + 1) * npix // nparts
        taps = dict(taps, rgb=taps["rgb"].reshape(3, 1, -1)[:, :, a:b], out=taps["out"].reshape(3, 1, -1)[:, :, a:b])
        checks = [c for c in checks if c.name == "mlp" or part == 0]
    failures = []
    for c in checks:
        for t, r in R.evaluate(c, ctx.P, taps).items():
            m = R.metrics(r, taps[t])
            ok, share, _ = R.input_condition(r)
            print(f"  {tag} {c.name:6s} {t:6s} n {m['n']:8d}  max err/d {m['max_ratio']:.3f}  "
                  f"mean dev {m['mean_err']:.3e} model {m['mean_model']:.3e}  bit-equal {m['bit_equal']:.4f}  clear {share:.2f}")
            if m["violations"]:
                failures.append((c.name, t, "hard", m["violations"], m["max_ratio"]))
            if m["mean_err"] > 2 * m["mean_model"]:
                failures.append((c.name, t, "precision", m["mean_err"], m["mean_model"]))
            if not ok:
                failures.append((c.name, t, "inputs", share))
    assert not failures, failures
