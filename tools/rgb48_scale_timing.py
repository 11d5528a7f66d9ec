"""Device time of hdrtv_post_rgb48_scaled (RGB48 at the display size, one kernel) against the unscaled post kernels at the output
size, HIP events around every call, warmed, the calls alternated round by round so that clocks and cache state are shared:

  hdrtv_post_rgb48_scaled  HxW -> dHxdW   f32 / f16 input, plain / PQ     reads 3 planes of HxW, writes 6 B per output pixel
  hdrtv_post_rgb48 / hdrtv_post_pq_rgb48 at dHxdW (f32)                   the yardstick: reads 12 B, writes 6 B per output pixel

Each figure: median and p10 / p90 of the per-call times, and the algorithmic bytes / time against 8 TB/s.

  python tools/rgb48_scale_timing.py [--size 1920x1080] [--out-size 3840x2160] [--calls 50] [--warmup 10] [--out file.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out-size", default="3840x2160")
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
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    small32 = torch.from_numpy(rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)).cuda()
    small16 = small32.half()
    big32 = torch.from_numpy(rng.uniform(-0.1, 1.1, (3, oh, ow)).astype(np.float32)).cuda()
    dst = torch.empty((oh, ow, 3), dtype=torch.uint16, device="cuda")
    d, pk = dst.data_ptr(), a.peak_nits
    out_b = oh * ow * 6
    cases = {
        "scaled f32 plain": (lambda: lib.hdrtv_post_rgb48_scaled(ctx, st, small32.data_ptr(), L.F32, h, w, 0, 0.0, d, oh, ow), h * w * 12 + out_b),
        "scaled f16 plain": (lambda: lib.hdrtv_post_rgb48_scaled(ctx, st, small16.data_ptr(), L.F16, h, w, 0, 0.0, d, oh, ow), h * w * 6 + out_b),
        "scaled f32 pq": (lambda: lib.hdrtv_post_rgb48_scaled(ctx, st, small32.data_ptr(), L.F32, h, w, 1, pk, d, oh, ow), h * w * 12 + out_b),
        "scaled f16 pq": (lambda: lib.hdrtv_post_rgb48_scaled(ctx, st, small16.data_ptr(), L.F16, h, w, 1, pk, d, oh, ow), h * w * 6 + out_b),
        "post_rgb48 f32 at the output size": (lambda: lib.hdrtv_post_rgb48(ctx, st, big32.data_ptr(), L.F32, oh, ow, d), oh * ow * 12 + out_b),
        "post_pq_rgb48 f32 at the output size": (lambda: lib.hdrtv_post_pq_rgb48(ctx, st, big32.data_ptr(), L.F32, oh, ow, pk, d), oh * ow * 12 + out_b),
    }
    for fn, _ in cases.values():
        for _ in range(a.warmup):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.calls):
        for k, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn() == 0
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    lines = [f"{torch.cuda.get_device_name(0)}; {lib.hdrtv_version().decode()}",
             f"{w}x{h} -> {ow}x{oh}, {a.calls} rounds after {a.warmup} warm-up calls each, HIP events, calls alternated round by round",
             f"{'call':40s} {'median us':>10s} {'p10':>8s} {'p90':>8s} {'MB':>7s} {'TB/s':>6s} {'of 8 TB/s':>9s}"]
    med = {}
    for k, (_, nbytes) in cases.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        lines.append(f"{k:40s} {med[k]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f} {nbytes / 1e6:7.1f} "
                     f"{nbytes / med[k] / 1e6:6.2f} {nbytes / med[k] * 1e6 / HBM_PEAK:9.2f}")
    y0, y1 = med["post_rgb48 f32 at the output size"], med["post_pq_rgb48 f32 at the output size"]
    for k in ("scaled f32 plain", "scaled f16 plain"):
        lines.append(f"{k}: {med[k] / y0:.2f} x post_rgb48 at the output size (aim: <= 1.5)")
    for k in ("scaled f32 pq", "scaled f16 pq"):
        lines.append(f"{k}: {med[k] / y1:.2f} x post_pq_rgb48 at the output size (aim: < 1)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
