"""Device time of the Floyd-Steinberg error diffusion at the given frame sizes and output formats, HIP events around
every call, warmed, the calls alternated round by round so that clocks and cache state are shared (the method of
tools/cleanup_timing.py):

  hdrtv_rgb48_to_ycbcr10_fs, fs_passes = 1     the samples launch alone (fully parallel: reads 6 B, writes 4 B per sample)
  hdrtv_rgb48_to_ycbcr10_fs, fs_passes = 2     the diffusion launch alone (one workgroup per plane, a wavefront of 256 rows)
  hdrtv_rgb48_to_ycbcr10_fs                    the whole call from RGB48 codes
  hdrtv_post_ycbcr10_fs f16                    the whole call from the model's tensor
  hdrtv_rgb48_to_ycbcr10_ex dither 1           the ordered-dither conversion of the same frame
  hdrtv_rgb48_to_ycbcr10                       the undithered conversion of the same frame

next to two figures that are computed, not measured: the serial floor of the rule, (W + 2 H) steps of the luma chain at
--step-cycles cycles (what one step of fs_diffuse_kernel issues: 25 wave instructions at 4 cycles each plus one LDS read and one
LDS write, read from the ISA) and --clock-ghz, and the steps the kernel's schedule takes for the luma plane,
ceil(H / 256) row groups x (W + 604) steps.

  python tools/fs_dither_timing.py [--sizes 1920x1080,3840x2160] [--pix-fmts yuv422p10le,p010le] [--calls 20] [--warmup 3] [--out file.txt]
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
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--pix-fmts", default="yuv422p10le,p010le")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-cycles", type=float, default=110.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"{torch.cuda.get_device_name(0)}; {lib.hdrtv_version().decode()}",
             f"{a.calls} rounds after {a.warmup} warm-up calls each, HIP events, calls alternated round by round; one session",
             f"serial floor: (W + 2 H) steps x {a.step_cycles:.0f} cycles at {a.clock_ghz} GHz; schedule: ceil(H / {L.FS_ROWS}) x (W + 604) luma steps"]
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.lower().split("x"))
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        ramp = (xx / w * 0.6 + yy / h * 0.3)[None] + np.random.default_rng(0).uniform(0.0, 0.004, (3, h, w)).astype(np.float32)
        t16 = torch.from_numpy(ramp).cuda().half()
        rgb = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
        assert lib.hdrtv_post_rgb48(ctx, st, t16.data_ptr(), L.F16, h, w, rgb.data_ptr()) == 0
        d = rgb.data_ptr()
        for fmt in a.pix_fmts.split(","):
            ycc = torch.empty((L.out_frame_bytes(fmt, h, w) // 2,), dtype=torch.uint16, device="cuda")
            planes = L.ycbcr10_planes(ycc.data_ptr(), h, w, fmt, "left")
            scratch = torch.empty((lib.hdrtv_ycbcr10_fs_scratch_bytes(L.YCC_FORMATS[fmt], h, w),), dtype=torch.uint8, device="cuda")
            sc = scratch.data_ptr()

            def fs(passes):
                p.set_variant("fs_passes", passes)
                rc = lib.hdrtv_rgb48_to_ycbcr10_fs(ctx, st, d, h, w, *planes, sc)
                p.set_variant("fs_passes", 3)
                return rc

            cases = {"fs samples launch (from codes)": lambda: fs(1),
                     "fs diffusion launch": lambda: fs(2),
                     "fs whole call from codes": lambda: fs(3),
                     "fs whole call from the f16 tensor": lambda: lib.hdrtv_post_ycbcr10_fs(ctx, st, t16.data_ptr(), L.F16, h, w, 0, 0.0, *planes, sc),
                     "ordered dither from codes": lambda: lib.hdrtv_rgb48_to_ycbcr10_ex(ctx, st, d, h, w, *planes, 1),
                     "no dither from codes": lambda: lib.hdrtv_rgb48_to_ycbcr10(ctx, st, d, h, w, *planes)}
            for fn in cases.values():
                for _ in range(a.warmup):
                    assert fn() == 0
            torch.cuda.synchronize()
            times = {k: [] for k in cases}
            for _ in range(a.calls):
                for k, fn in cases.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    assert fn() == 0
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3)
            ch = h if fmt == "yuv422p10le" else h // 2
            floor_us = (w + 2 * h) * a.step_cycles / (a.clock_ghz * 1e3)
            steps = -(-h // L.FS_ROWS) * (w + 604)
            lines.append(f"{w}x{h} {fmt} (chroma planes {w // 2}x{ch}); scratch {scratch.numel() / 1e6:.1f} MB")
            lines.append(f"  {'call':36s} {'median us':>10s} {'p10':>9s} {'p90':>9s}")
            for k in cases:
                t = np.array(times[k])
                lines.append(f"  {k:36s} {np.median(t):10.1f} {np.percentile(t, 10):9.1f} {np.percentile(t, 90):9.1f}")
            dif = float(np.median(times["fs diffusion launch"]))
            lines.append(f"  serial floor (W + 2 H = {w + 2 * h} steps): {floor_us:.0f} us; the schedule's {steps} luma steps at that rate: "
                         f"{steps * a.step_cycles / (a.clock_ghz * 1e3):.0f} us; measured diffusion / luma steps = {dif * 1e3 / steps:.1f} ns per step")
            lines.append(f"  whole call / ordered dither = {np.median(times['fs whole call from codes']) / np.median(times['ordered dither from codes']):.0f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
