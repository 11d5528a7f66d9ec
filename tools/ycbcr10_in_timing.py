"""Device time of the 10-bit Y'CbCr input preprocess against the 8-bit forms at the same size, HIP events around every call, warmed,
the calls alternated round by round so that clocks and cache state are shared (the method of tools/ycbcr10_timing.py):

  hdrtv_preprocess_ycbcr10    p010le / yuv420p10le / yuv422p10le   pre_fused<Ycc10Src>: reads 3 / 3 / 4 B per pixel
  hdrtv_preprocess_yuv420     I420                                  the yardstick: pre_fused<Yuv420Src>, reads 1.5 B per pixel
  hdrtv_preprocess            bgr24                                 pre_fused<PfBgr>, reads 3 B per pixel
  hdrtv_ycbcr10_to_rgb10      the rule on its own, for reference (reads the planes, writes 6 B per pixel)

Every preprocess writes the 6 B per pixel fp16 tensor and the 0.375 B per pixel condition map.  Byte model of the ratio to the I420
form: (3 + 6.375) / (1.5 + 6.375) = 1.19 for 10-bit 4:2:0 and (4 + 6.375) / 7.875 = 1.32 for 4:2:2.  Each figure: median and
p10 / p90 of the per-call times, and the algorithmic bytes / time against 8 TB/s.

  python tools/ycbcr10_in_timing.py [--sizes 1920x1080,3840x2160] [--calls 50] [--warmup 10] [--out file.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"))
HBM_PEAK = 8.0e12
MODEL = {"p010le": (3 + 6.375) / 7.875, "yuv420p10le": (3 + 6.375) / 7.875, "yuv422p10le": (4 + 6.375) / 7.875}


def measure(p, h, w, calls, warmup):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.lib import input_format
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.hdrtv_reserve(ctx, h, w) == 0, lib.hdrtv_last_error(ctx)
    rng = np.random.default_rng(0)
    px = h * w
    out = torch.empty((3, h, w), dtype=torch.float16, device="cuda")
    cond = torch.empty((3, h // 4, w // 4), dtype=torch.float16, device="cuda")
    codes = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    wr = px * 6 + 3 * (h // 4) * (w // 4) * 2
    bgr = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    i420 = torch.from_numpy(rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)).cuda()
    cases = {
        "preprocess bgr24": (lambda: lib.hdrtv_preprocess(ctx, st, bgr.data_ptr(), h, w, out.data_ptr(), cond.data_ptr()), px * 3 + wr),
        "preprocess_yuv420 i420": (lambda a=input_format("i420").planes(i420.data_ptr(), h, w):
                                   lib.hdrtv_preprocess_yuv420(ctx, st, *a, h, w, out.data_ptr(), cond.data_ptr()), px * 3 // 2 + wr),
    }
    keep = [bgr, i420]
    for fmt in L.YCBCR10_IN_FORMATS:
        shape = L.ycbcr10_frame_shape(fmt, h, w)
        v = rng.integers(0, 1024, shape, dtype=np.uint16)
        f = torch.from_numpy((v << 6) if fmt == "p010le" else v).cuda()
        keep.append(f)
        a = input_format(fmt).planes(f.data_ptr(), h, w)
        rd = shape[0] * shape[1] * 2
        cases[f"preprocess_ycbcr10 {fmt}"] = (lambda a=a: lib.hdrtv_preprocess_ycbcr10(ctx, st, *a, h, w, out.data_ptr(), cond.data_ptr()),
                                              rd + wr)
        cases[f"ycbcr10_to_rgb10 {fmt}"] = (lambda a=a: lib.hdrtv_ycbcr10_to_rgb10(ctx, st, *a, h, w, codes.data_ptr()), rd + px * 6)
    for fn, _ in cases.values():
        for _ in range(warmup):
            assert fn() == 0, lib.hdrtv_last_error(ctx)
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(calls):
        for k, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn() == 0
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    lines = [f"{w}x{h}, {calls} rounds after {warmup} warm-up calls each, HIP events, calls alternated round by round",
             f"{'call':34s} {'median us':>10s} {'p10':>8s} {'p90':>8s} {'MB':>7s} {'TB/s':>6s} {'of 8 TB/s':>9s}"]
    med = {}
    for k, (_, nbytes) in cases.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        lines.append(f"{k:34s} {med[k]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f} {nbytes / 1e6:7.1f} "
                     f"{nbytes / med[k] / 1e6:6.2f} {nbytes / med[k] * 1e6 / HBM_PEAK:9.2f}")
    for fmt in L.YCBCR10_IN_FORMATS:
        m = med[f"preprocess_ycbcr10 {fmt}"]
        lines.append(f"preprocess_ycbcr10 {fmt}: {m / med['preprocess_yuv420 i420']:.2f} x preprocess_yuv420 (byte model {MODEL[fmt]:.2f}), "
                     f"{m / med['preprocess bgr24']:.2f} x preprocess bgr24")
    del keep
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lines = [f"ycbcr10_in_timing: {torch.cuda.get_device_name(0)}; {p._lib.hdrtv_version().decode()}"]
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.lower().split("x"))
        lines += measure(p, h, w, a.calls, a.warmup)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
