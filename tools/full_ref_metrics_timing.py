#!/usr/bin/env python3
"""Times hdrtv_full_reference_metrics at 3840x2160 -> 512x288 -- the stream-ordered launches with HIP events, the calls that bring
numbers back to the host by the wall clock -- and, beside them in the same session, hdrtv_metrics on a 3840x2160 fp16 pair (what the
playback CSV's psnr_db cost before).  A measurement, not a target: no ratio is asserted.

    python tools/full_ref_metrics_timing.py [--size 3840x2160] [--calls 20] [--rounds 7] [--out profiles/full_ref_metrics_timing.txt]

The frames are seeded noise on a smooth ramp with 140-row black bars (the reference's letterboxed 2.39:1 case), so the crop, the
table path of the area reduction (1880 rows -> 251) and the grade match all have work to do.  A figure is the median over the rounds
of the time per call, with the fastest and slowest round beside it."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    w, h = (int(v) for v in a.size.lower().split("x", 1))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("full_ref_metrics_timing needs a GPU")
    import metrics_full_ref as R
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X

    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), device="cuda:0", use_hg=False, warmup_passes=0)
    bars = h * 140 // 2160
    pred_np, ref_np = R.ramp_pair(h, w, 1, bars=bars)
    pred, ref = torch.from_numpy(pred_np).cuda(), torch.from_numpy(ref_np).cuda()
    ta = (pred.permute(2, 0, 1).float() / 65535.0).half().contiguous()
    tb = (ref.permute(2, 0, 1).float() / 65535.0).half().contiguous()
    flat = torch.full_like(pred, 12345)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.calls

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.calls

    full = p.full_reference_metrics(pred, ref)
    rect, (eh, ew) = full["crop_rect"], full["eval_size"]
    ep = p.rgb48_area_reduce(pred, ew, eh, rect=rect)
    er = p.rgb48_area_reduce(ref, ew, eh, rect=rect)
    eflat = p.rgb48_area_reduce(flat, ew, eh, rect=rect)
    rows = [
        ("launch: hdrtv_rgb48_border_counts (both frames)", events, lambda: p.rgb48_border_counts(pred, ref)),
        ("launch: hdrtv_rgb48_area_reduce (one frame; the chain: both in one launch)", events, lambda: p.rgb48_area_reduce(pred, ew, eh, rect=rect)),
        (f"call:   hdrtv_rgb48_grade_match at {ew}x{eh} (histograms, 1.5 MiB to the host, statistics)", wall, lambda: p.rgb48_grade_match(ep, er)),
        (f"call:   hdrtv_rgb48_grade_match at {ew}x{eh}, flat prediction (one bin)", wall, lambda: p.rgb48_grade_match(eflat, er)),
        (f"call:   metrics on the {ew}x{eh} evaluation frames alone (one metric launch + partial sums)", wall,
         lambda: p.full_reference_metrics(ep, er, crop=False, normalized=False)),
        ("call:   live path (crop=False, normalized=False)", wall, lambda: p.full_reference_metrics(pred, ref, crop=False, normalized=False)),
        ("call:   crop only", wall, lambda: p.full_reference_metrics(pred, ref, normalized=False)),
        ("call:   normalized only", wall, lambda: p.full_reference_metrics(pred, ref, crop=False)),
        ("call:   hdrtv_full_reference_metrics, whole (crop + normalized)", wall, lambda: p.full_reference_metrics(pred, ref)),
        (f"call:   hdrtv_metrics on the {w}x{h} fp16 pair (objective_metrics)", wall, lambda: p.objective_metrics(ta, tb)),
    ]
    for _, _, fn in rows:                                        # warm-up: code objects, scratch, tables
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in rows]
    for _ in range(a.rounds):
        for i, (_, how, fn) in enumerate(rows):
            times[i].append(how(fn))
    lines = [f"full_ref_metrics_timing: {torch.cuda.get_device_name(0)}, {w}x{h} -> crop {rect} -> {ew}x{eh}, "
             f"{a.calls} calls x {a.rounds} rounds, build {L.build_id()}",
             "us per call: median [fastest .. slowest round]; launches by HIP events, calls by the wall clock (they synchronise)",
             f"result: { {k: (round(v, 6) if isinstance(v, float) else v) for k, v in full.items() if k != 'obj_note'} }"]
    for (name, _, _), v in zip(rows, times):
        lines.append(f"  {statistics.median(v):9.1f} [{min(v):9.1f} .. {max(v):9.1f}]  {name}")
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
