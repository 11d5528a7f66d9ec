"""Device time of the 4:2:0 input kernels against the BGR preprocess at one size (default 3840x2160), HIP events, warmed,
the four calls alternated round by round so that clocks and cache state are shared:

  hdrtv_preprocess (BGR)         3 B in + 6 B f16 planes + cond per pixel
  hdrtv_preprocess_yuv420 I420   1.5 B in + the same outputs
  hdrtv_preprocess_yuv420 NV12   1.5 B in + the same outputs
  hdrtv_yuv420_to_bgr_u8 (I420)  1.5 B in + 3 B out

Each figure: median and p10 / p90 of the per-call times, and the algorithmic bytes / time against 8 TB/s.

  python tools/yuv420_timing.py [--size 3840x2160] [--calls 300] [--out file.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    w, h = (int(v) for v in a.size.lower().split("x"))
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    p._ensure_buffers(h, w)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    bgr = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    yuv = torch.from_numpy(rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)).cuda()
    conv = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    rgb, cond = p._gpu_input, p._gpu_cond
    y, c = yuv.data_ptr(), yuv.data_ptr() + h * w
    i420 = (y, w, c, c + (h // 2) * (w // 2), w // 2, L.YUV_I420, 709, 0)
    nv12 = (y, w, c, None, w, L.YUV_NV12, 709, 0)
    out_b = h * w * 3 * 2 + 3 * (h // 4) * (w // 4) * 2
    cases = {
        "preprocess_bgr": (lambda: lib.hdrtv_preprocess(ctx, st, bgr.data_ptr(), h, w, rgb.data_ptr(), cond.data_ptr()), h * w * 3 + out_b),
        "preprocess_yuv420_i420": (lambda: lib.hdrtv_preprocess_yuv420(ctx, st, *i420, h, w, rgb.data_ptr(), cond.data_ptr()),
                                   h * w * 3 // 2 + out_b),
        "preprocess_yuv420_nv12": (lambda: lib.hdrtv_preprocess_yuv420(ctx, st, *nv12, h, w, rgb.data_ptr(), cond.data_ptr()),
                                   h * w * 3 // 2 + out_b),
        "yuv420_to_bgr_u8_i420": (lambda: lib.hdrtv_yuv420_to_bgr_u8(ctx, st, *i420, h, w, conv.data_ptr()), h * w * 3 // 2 + h * w * 3),
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
            times[k].append((e0, e1))
        torch.cuda.synchronize()
    res = {"size": f"{w}x{h}", "calls_each": a.calls, "warmup_each": a.warmup, "device": torch.cuda.get_device_name(0),
           "library": lib.hdrtv_version().decode(), "hbm_peak_bytes_per_s": HBM_PEAK, "kernels": {}}
    for k, (_, nbytes) in cases.items():
        us = np.array([s.elapsed_time(e) * 1e3 for s, e in times[k]])
        med = float(np.median(us))
        res["kernels"][k] = {"median_us": round(med, 2), "p10_us": round(float(np.percentile(us, 10)), 2),
                             "p90_us": round(float(np.percentile(us, 90)), 2), "algorithmic_bytes": int(nbytes),
                             "algorithmic_tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3),
                             "frac_of_8tbs": round(nbytes / (med * 1e-6) / HBM_PEAK, 3)}
    p.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
