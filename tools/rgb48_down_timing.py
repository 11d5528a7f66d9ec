"""Device time of hdrtv_post_rgb48_down (the shrink of the RGB48 output) without and with its SSimDownscaler stage, beside the floor
for reading the same tensor: the unscaled hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 at the processing size (csrc/prepost.hip, which the
shrink does not touch), in the same session: HIP events around every call, warmed, the calls alternated round by round so that
clocks and cache state are shared.  f32 / f16 input, plain / PQ, every --out-size.

Each figure: median and p10 / p90 of the per-call times; then per form the ratios to the unscaled call.  There is no pass mark.
Run it under a time limit of its own (the whole run is one GPU step of a few seconds):

  timeout -k 10 300 python tools/rgb48_down_timing.py [--size 3840x2160] [--out-size 2560x1440 --out-size 1920x1080] [--antiring 51] [--calls 50] [--warmup 10] [--out file.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--out-size", action="append", help="may be given more than once (default: 2560x1440 and 1920x1080)")
    ap.add_argument("--antiring", type=int, default=51, help="the strength code, 0 .. 256 (51 = the reference's 0.20)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--peak-nits", type=float, default=1000.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    w, h = (int(v) for v in a.size.lower().split("x"))
    outs = [tuple(int(v) for v in s.lower().split("x")) for s in (a.out_size or ["2560x1440", "1920x1080"])]
    for ow, oh in outs:
        L.check_down_size(w, h, ow, oh)
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    big32 = torch.from_numpy(rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)).cuda()
    big16 = big32.half()
    dst = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    d, pk, ar = dst.data_ptr(), a.peak_nits, a.antiring
    forms = {"f32 plain": (big32, L.F32, 0), "f16 plain": (big16, L.F16, 0), "f32 pq": (big32, L.F32, 1), "f16 pq": (big16, L.F16, 1)}
    cases = {}
    for f, (t, dt, pq) in forms.items():
        if pq:
            cases[f"unscaled {w}x{h} {f}"] = (lambda t=t, dt=dt: lib.hdrtv_post_pq_rgb48(ctx, st, t.data_ptr(), dt, h, w, pk, d))
        else:
            cases[f"unscaled {w}x{h} {f}"] = (lambda t=t, dt=dt: lib.hdrtv_post_rgb48(ctx, st, t.data_ptr(), dt, h, w, d))
        for ow, oh in outs:
            base = (ctx, st, t.data_ptr(), dt, h, w, pq, pk, d, oh, ow)
            cases[f"mitchell {ow}x{oh} {f}"] = (lambda b=base, t=t: lib.hdrtv_post_rgb48_down(*b, ar, 0))
            cases[f"ssim     {ow}x{oh} {f}"] = (lambda b=base, t=t: lib.hdrtv_post_rgb48_down(*b, ar, 1))
    for fn in cases.values():
        for _ in range(a.warmup):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {c: [] for c in cases}
    for _ in range(a.calls):
        for c, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn() == 0
            e1.record()
            e1.synchronize()
            times[c].append(e0.elapsed_time(e1) * 1e3)
    lines = [f"{torch.cuda.get_device_name(0)}; {lib.hdrtv_version().decode()}",
             f"{w}x{h} -> {', '.join('%dx%d' % o for o in outs)}, antiring = {ar} (of 256); {a.calls} rounds after {a.warmup} warm-up calls each, "
             "HIP events, calls alternated round by round; unscaled = hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 at the processing size",
             f"{'call':34s} {'median us':>10s} {'p10':>8s} {'p90':>8s}"]
    med = {}
    for c in cases:
        t = np.array(times[c])
        med[c] = float(np.median(t))
        lines.append(f"{c:34s} {med[c]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f}")
    for f in forms:
        floor = med[f"unscaled {w}x{h} {f}"]
        for ow, oh in outs:
            mit, ss = med[f"mitchell {ow}x{oh} {f}"], med[f"ssim     {ow}x{oh} {f}"]
            lines.append(f"{f} -> {ow}x{oh}: mitchell / unscaled = {mit / floor:.2f} ({mit - floor:+.1f} us); ssim / unscaled = {ss / floor:.2f} "
                         f"({ss - floor:+.1f} us); the ssim stage adds {ss - mit:.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
