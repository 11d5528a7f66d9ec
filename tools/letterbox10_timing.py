"""Device time of the 10-bit letterbox against the 8-bit route at the same sizes, HIP events around every call, warmed, the calls
alternated round by round so that clocks and cache state are shared (the method of tools/ycbcr10_in_timing.py):

  hdrtv_letterbox_ycbcr10                 p010le / yuv420p10le / yuv422p10le   the codes: planes at the source size in, 6 B per
                                                                               destination pixel out, one launch
  hdrtv_preprocess_ycbcr10_letterboxed    the same three                       the fp16 tensor (6 B per destination pixel) in that one
                                                                               launch, then the condition map from the tensor
  8-bit route                             I420                                 hdrtv_yuv420_to_bgr_u8 at the source size, hdrtv_letterbox_u8,
                                                                               hdrtv_preprocess: three launches (preprocess_yuv420_letterboxed)
  hdrtv_preprocess_ycbcr10                the three, at the DESTINATION size   what a frame decoded at the processing size costs
  hdrtv_letterbox_u8                      BGR                                  the second launch of the 8-bit route on its own

Three geometries, source -> destination: 3840x2160 -> 1920x1080 (2x2 box), 3840x2160 -> 2560x1440 (fractional area),
1920x1080 -> 3840x2160 (cubic).  MB: the algorithmic bytes of the call (every plane, intermediate and output once).  Each figure:
median and p10 / p90 of the per-call times.  No test asserts a time.

  python tools/letterbox10_timing.py [--calls 50] [--warmup 10] [--out file.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"))
GEOMETRIES = [((3840, 2160), (1920, 1080), "2x2 box"), ((3840, 2160), (2560, 1440), "fractional area"), ((1920, 1080), (3840, 2160), "cubic")]


def measure(p, src_wh, dst_wh, kind, calls, warmup):
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.lib import input_format
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    (sw, sh), (w, h) = src_wh, dst_wh
    assert lib.hdrtv_reserve(ctx, h, w) == 0, lib.hdrtv_last_error(ctx)
    rng = np.random.default_rng(0)
    spx, px = sh * sw, h * w
    out = torch.empty((3, h, w), dtype=torch.float16, device="cuda")
    cond = torch.empty((3, h // 4, w // 4), dtype=torch.float16, device="cuda")
    codes = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    cond_b = 3 * (h // 4) * (w // 4) * 2
    i420 = torch.from_numpy(rng.integers(0, 256, (sh * 3 // 2, sw), dtype=np.uint8)).cuda()
    bgr_src = torch.empty((sh, sw, 3), dtype=torch.uint8, device="cuda")
    bgr_dst = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    a8 = input_format("i420").planes(i420.data_ptr(), sh, sw)

    def route8():
        rc = lib.hdrtv_yuv420_to_bgr_u8(ctx, st, *a8, sh, sw, bgr_src.data_ptr())
        rc = rc or lib.hdrtv_letterbox_u8(ctx, st, bgr_src.data_ptr(), sh, sw, bgr_dst.data_ptr(), h, w)
        return rc or lib.hdrtv_preprocess(ctx, st, bgr_dst.data_ptr(), h, w, out.data_ptr(), cond.data_ptr())

    # planes in, BGR out and in again at the source size, BGR out and in again at the destination size, tensor and map out
    cases = {"8-bit route i420 (3 launches)": (route8, spx * 3 // 2 + 2 * spx * 3 + 2 * px * 3 + px * 6 + cond_b)}
    # the u8 letterbox on its own (route8's second launch; its source is the frame route8's first launch left)
    cases["letterbox_u8 alone"] = (lambda: lib.hdrtv_letterbox_u8(ctx, st, bgr_src.data_ptr(), sh, sw, bgr_dst.data_ptr(), h, w), spx * 3 + px * 3)
    keep = [i420, bgr_src, bgr_dst]
    for fmt in L.YCBCR10_IN_FORMATS:
        def frame(hh, ww):
            v = rng.integers(0, 1024, L.ycbcr10_frame_shape(fmt, hh, ww), dtype=np.uint16)
            f = torch.from_numpy((v << 6) if fmt == "p010le" else v).cuda()
            keep.append(f)
            return f
        fs, fd = frame(sh, sw), frame(h, w)
        a = input_format(fmt).planes(fs.data_ptr(), sh, sw)
        ad = input_format(fmt).planes(fd.data_ptr(), h, w)
        rd, rdd = fs.numel() * 2, fd.numel() * 2
        cases[f"letterbox_ycbcr10 {fmt}"] = (lambda a=a: lib.hdrtv_letterbox_ycbcr10(ctx, st, *a, sh, sw, codes.data_ptr(), h, w), rd + px * 6)
        cases[f"preprocess_ycbcr10_letterboxed {fmt}"] = (
            lambda a=a: lib.hdrtv_preprocess_ycbcr10_letterboxed(ctx, st, *a, sh, sw, h, w, out.data_ptr(), cond.data_ptr()),
            rd + px * 6 + px * 6 + cond_b)                  # the tensor is written, then read for the condition map
        cases[f"preprocess_ycbcr10 {fmt} at {w}x{h}"] = (
            lambda ad=ad: lib.hdrtv_preprocess_ycbcr10(ctx, st, *ad, h, w, out.data_ptr(), cond.data_ptr()), rdd + px * 6 + cond_b)
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
    lines = [f"{sw}x{sh} -> {w}x{h} ({kind}), {calls} rounds after {warmup} warm-up calls each, HIP events, calls alternated round by round",
             f"{'call':50s} {'median us':>10s} {'p10':>8s} {'p90':>8s} {'MB':>7s} {'TB/s':>6s}"]
    med = {}
    for k, (_, nbytes) in cases.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        lines.append(f"{k:50s} {med[k]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f} {nbytes / 1e6:7.1f} {nbytes / med[k] / 1e6:6.2f}")
    for fmt in L.YCBCR10_IN_FORMATS:
        m = med[f"preprocess_ycbcr10_letterboxed {fmt}"]
        lines.append(f"preprocess_ycbcr10_letterboxed {fmt}: {m / med['8-bit route i420 (3 launches)']:.2f} x the 8-bit route, "
                     f"{m / med[f'preprocess_ycbcr10 {fmt} at {w}x{h}']:.2f} x preprocess_ycbcr10 at the destination size")
    del keep
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lines = [f"letterbox10_timing: {torch.cuda.get_device_name(0)}; {p._lib.hdrtv_version().decode()}"]
    for src_wh, dst_wh, kind in GEOMETRIES:
        lines += measure(p, src_wh, dst_wh, kind, a.calls, a.warmup)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
