"""Device time of hdrtv_post_rgb48_ssimsr (the spline36 / SSimSuperRes upscale of the RGB48 output) with its shader stage off and
on, beside the other two upscalers of the reference's display chain in the same session: hdrtv_post_rgb48_fsr with RCAS, and the
Lanczos chain hdrtv_post_rgb48_scaled_cas with the CAS code 3605 and the strength code 26 (its 0.16 / 0.10 at 1080p).  HIP events
around every call, warmed, the calls alternated round by round so that clocks and cache state are shared.  f32 / f16 input,
plain / PQ.

Each figure: median and p10 / p90 of the per-call times; then per form the ratios of the new calls to FSR and to the Lanczos chain.
There is no pass mark.  Run it under a time limit of its own (the whole run is one GPU step of a few seconds):

  timeout -k 10 300 python tools/rgb48_ssimsr_timing.py [--size 1920x1080] [--out-size 3840x2160] [--calls 50] [--warmup 10] [--out file.txt]
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
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out-size", default="3840x2160")
    ap.add_argument("--sharpness", type=float, default=0.2, help="the RCAS sharpness of the FSR row, 0 .. 2")
    ap.add_argument("--cas", type=int, default=3605, help="the CAS code of the Lanczos chain, 1032 .. 4096")
    ap.add_argument("--antiring", type=int, default=26, help="its strength code, 1 .. 256")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--peak-nits", type=float, default=1000.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    w, h = (int(v) for v in a.size.lower().split("x"))
    ow, oh = (int(v) for v in a.out_size.lower().split("x"))
    L.check_ssimsr_size(w, h, ow, oh)
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    small32 = torch.from_numpy(rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)).cuda()
    small16 = small32.half()
    dst = torch.empty((oh, ow, 3), dtype=torch.uint16, device="cuda")
    d, pk, ar, k, sh = dst.data_ptr(), a.peak_nits, a.antiring, a.cas, a.sharpness
    forms = {"f32 plain": (small32, L.F32, 0), "f16 plain": (small16, L.F16, 0), "f32 pq": (small32, L.F32, 1), "f16 pq": (small16, L.F16, 1)}
    names = ("spline36      ", "spline36+ssim ", "fsr easu+rcas ", "scaled_cas+ar ")
    cases = {}
    for f, (t, dt, pq) in forms.items():
        base = (ctx, st, t.data_ptr(), dt, h, w, pq, pk, d, oh, ow)
        cases[names[0] + f] = (lambda b=base, t=t: lib.hdrtv_post_rgb48_ssimsr(*b, 0))
        cases[names[1] + f] = (lambda b=base, t=t: lib.hdrtv_post_rgb48_ssimsr(*b, 1))
        cases[names[2] + f] = (lambda b=base, t=t: lib.hdrtv_post_rgb48_fsr(*b, 1, sh))
        cases[names[3] + f] = (lambda b=base, t=t: lib.hdrtv_post_rgb48_scaled_cas(*b, ar, k))
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
             f"{w}x{h} -> {ow}x{oh}; FSR: sharpness = {sh}; the Lanczos chain: cas = {k} (code), antiring = {ar} (of 256); {a.calls} rounds "
             f"after {a.warmup} warm-up calls each, HIP events, calls alternated round by round",
             f"{'call':28s} {'median us':>10s} {'p10':>8s} {'p90':>8s}"]
    med = {}
    for c in cases:
        t = np.array(times[c])
        med[c] = float(np.median(t))
        lines.append(f"{c:28s} {med[c]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f}")
    for f in forms:
        sp, both, fsr, lan = (med[n + f] for n in names)
        lines.append(f"{f}: spline36 / fsr = {sp / fsr:.2f}, / scaled_cas+ar = {sp / lan:.2f}; spline36+ssim / fsr = {both / fsr:.2f}, "
                     f"/ scaled_cas+ar = {both / lan:.2f}; the shader's stage adds {both - sp:.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
