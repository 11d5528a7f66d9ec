#!/usr/bin/env python3
"""Times hdrtv_light_stats and hdrtv_rgb48_light_stats next to hdrtv_post_rgb48 (the yardstick: existing code that reads the same
tensor and writes 12 bytes per pixel more) with HIP events at 3840x2160, on three inputs: a noise frame, a constant black frame
and the model's output for the synthetic source.  The three calls alternate inside every round, so they share the machine's state.

    python tools/light_stats_timing.py [--size 3840x2160] [--calls 40] [--rounds 7] [--out profiles/light_stats_timing.txt]

A call's time is the event time around `--calls` back-to-back launches divided by their number (the record's hipMemsetAsync is part
of a light-level call); the figure reported is the median over the rounds, with the fastest and slowest round beside it.  The same
buffers are read again and again, so all three kernels read from whatever the caches keep of a frame -- equally.  The tensor entry
point is also timed with the grid capped at 1, 2, 4 and 8 workgroups per CU (variant light_wgs)."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "hdr-realtime-video-pipeline_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    w, h = (int(v) for v in a.size.lower().split("x", 1))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("light_stats_timing needs a GPU")
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.lightlevel import FrameLight
    from hdrtv_mi355x.processor import HDRTVNetMI355X

    hr = W.load_pack(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"))
    p = HDRTVNetMI355X(hr, device="cuda:0", use_hg=True, hg_weights=W.seeded_hg_state(1234), warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    out, _ = p.infer(p.preprocess(W.synthetic_frame(h, w, seed=3, kind="gradient")))
    model = out[0].clone()
    dt = L.F32 if model.dtype == torch.float32 else L.F16
    gen = torch.Generator(device="cuda").manual_seed(1234)
    inputs = [("noise", torch.rand((3, h, w), generator=gen, device="cuda", dtype=torch.float32).to(model.dtype)),
              ("black", torch.zeros_like(model)), ("model", model)]
    codes = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    rec = torch.empty(L.LIGHT_WORDS, dtype=torch.uint32, device="cuda")
    st = p._stream()
    full = (0, 0, w, h)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.calls          # microseconds per call

    lines = [f"light_stats_timing: {torch.cuda.get_device_name(0)}, {w}x{h}, tensor dtype {str(model.dtype).split('.')[-1]}, "
             f"{a.calls} calls x {a.rounds} rounds, build {L.build_id()}",
             "us per call: median [fastest .. slowest round]; ratio = median / hdrtv_post_rgb48's median on the same input"]
    for name, t in inputs:
        calls = {
            "hdrtv_post_rgb48": lambda: p._chk(lib.hdrtv_post_rgb48(ctx, st, t.data_ptr(), dt, h, w, codes.data_ptr()), "post_rgb48"),
            "hdrtv_light_stats": lambda: p._chk(lib.hdrtv_light_stats(ctx, st, t.data_ptr(), dt, h, w, 0, 0.0, *full, rec.data_ptr()), "light_stats"),
            "hdrtv_rgb48_light_stats": lambda: p._chk(lib.hdrtv_rgb48_light_stats(ctx, st, codes.data_ptr(), h, w, *full, rec.data_ptr()), "rgb48_light_stats"),
        }
        for fn in calls.values():                                # warm-up: code objects, and `codes` holds this input's frame
            fn()
        torch.cuda.synchronize()
        calls["hdrtv_light_stats"]()
        r_tensor = rec.cpu().numpy().copy()
        calls["hdrtv_rgb48_light_stats"]()
        r_codes = rec.cpu().numpy().copy()
        f = FrameLight.from_record(r_tensor)
        same = bool(np.array_equal(r_tensor, r_codes))
        times = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        base = statistics.median(times["hdrtv_post_rgb48"])
        lines.append(f"[{name}] max code {f.max_code}, CLL {f.cll:.1f} nits, FALL {f.fall:.2f} nits, non-zero bins "
                     f"{int((f.hist > 0).sum())}, tensor and RGB48 records equal: {same}")
        for k, v in times.items():
            med = statistics.median(v)
            lines.append(f"  {k:26s} {med:8.1f} [{min(v):8.1f} .. {max(v):8.1f}]  ratio {med / base:5.2f}")
        sweep, default = [], p.get_variant("light_wgs")
        for wgs in (1, 2, 4, 8):
            p.set_variant("light_wgs", wgs)
            calls["hdrtv_light_stats"]()
            torch.cuda.synchronize()
            assert np.array_equal(rec.cpu().numpy(), r_tensor), "the record depends on the grid"
            v = [timed(calls["hdrtv_light_stats"]) for _ in range(a.rounds)]
            sweep.append(f"{wgs}: {statistics.median(v):.1f}")
        p.set_variant("light_wgs", default)
        lines.append(f"  hdrtv_light_stats by light_wgs (workgroups per CU; the figures above: {default})  " + "  ".join(sweep))
    p.close()
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(report)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
