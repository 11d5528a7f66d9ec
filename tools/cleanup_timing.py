"""Device time of the output cleanup at one frame size, HIP events around every call, warmed, the calls alternated
round by round so that clocks and cache state are shared (the method of tools/ycbcr10_timing.py):

  hdrtv_rgb48_deband                                           the deband kernel alone: reads 6 B per pixel (+ halo), writes 6 B
  hdrtv_post_ycbcr10_ex  dither 0 | 1, f16 / f32, plain / PQ   each dithered fused conversion next to its undithered twin
  hdrtv_rgb48_to_ycbcr10_ex  dither 0 | 1                      the same for the RGB48-codes source
  post_rgb48 + deband + rgb48_to_ycbcr10_ex(1)                 the whole deband + dither route of _post_out (three launches) ...
  hdrtv_post_ycbcr10 f16                                       ... next to the one-launch P010 of a frame without cleanup

Each figure: median and p10 / p90 of the per-call times, and the algorithmic bytes / time against 8 TB/s.

  python tools/cleanup_timing.py [--size 3840x2160] [--pix-fmt p010le] [--siting left] [--calls 50] [--warmup 10] [--out file.txt]
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
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--pix-fmt", default="p010le")
    ap.add_argument("--siting", default="left")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--peak-nits", type=float, default=1000.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    w, h = (int(v) for v in a.size.lower().split("x"))
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # a picture deband has work on: a smooth ramp (so most pixels pass the threshold and are averaged) with a little noise
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ramp = (xx / w * 0.6 + yy / h * 0.3)[None] + np.random.default_rng(0).uniform(0.0, 0.004, (3, h, w)).astype(np.float32)
    t32 = torch.from_numpy(ramp.astype(np.float32)).cuda()
    t16 = t32.half()
    raw = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    rgb = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    ycc_b = L.out_frame_bytes(a.pix_fmt, h, w)
    ycc = torch.empty((ycc_b // 2,), dtype=torch.uint16, device="cuda")
    planes = L.ycbcr10_planes(ycc.data_ptr(), h, w, a.pix_fmt, a.siting)
    r, d, pk, px = raw.data_ptr(), rgb.data_ptr(), a.peak_nits, h * w
    assert lib.hdrtv_post_rgb48(ctx, st, t16.data_ptr(), L.F16, h, w, r) == 0

    def route():
        rc = lib.hdrtv_post_rgb48(ctx, st, t16.data_ptr(), L.F16, h, w, r)
        rc = rc or lib.hdrtv_rgb48_deband(ctx, st, r, h, w, L.DEBAND_RANGE, L.DEBAND_THRESHOLD, 0, d)
        return rc or lib.hdrtv_rgb48_to_ycbcr10_ex(ctx, st, d, h, w, *planes, 1)

    cases = {"deband R=16 T=1311": (lambda: lib.hdrtv_rgb48_deband(ctx, st, r, h, w, 16, 1311, 0, d), px * 12),
             "deband R=1 T=1311": (lambda: lib.hdrtv_rgb48_deband(ctx, st, r, h, w, 1, 1311, 0, d), px * 12)}
    for name, t, dt, nin in (("f16", t16, L.F16, 6), ("f32", t32, L.F32, 12)):
        for pq in (0, 1):
            for dither in (0, 1):
                cases[f"fused {name} {'pq' if pq else 'plain'} dither {dither}"] = (
                    lambda t=t, dt=dt, pq=pq, dither=dither: lib.hdrtv_post_ycbcr10_ex(ctx, st, t.data_ptr(), dt, h, w, pq, pk, *planes, dither),
                    px * nin + ycc_b)
    for dither in (0, 1):
        cases[f"from codes dither {dither}"] = (lambda dither=dither: lib.hdrtv_rgb48_to_ycbcr10_ex(ctx, st, d, h, w, *planes, dither),
                                               px * 6 + ycc_b)
    cases["route: post_rgb48 + deband + ex(1)"] = (route, px * 6 + px * 6 + px * 12 + px * 6 + ycc_b)
    cases["today: post_ycbcr10 f16"] = (lambda: lib.hdrtv_post_ycbcr10(ctx, st, t16.data_ptr(), L.F16, h, w, 0, 0.0, *planes), px * 6 + ycc_b)
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
    assert lib.hdrtv_rgb48_deband(ctx, st, r, h, w, 16, 1311, 0, d) == 0
    torch.cuda.synchronize()
    changed = float((raw.cpu().numpy() != rgb.cpu().numpy()).any(axis=2).mean())
    lines = [f"{torch.cuda.get_device_name(0)}; {lib.hdrtv_version().decode()}",
             f"{w}x{h} {a.pix_fmt} siting {a.siting}, {a.calls} rounds after {a.warmup} warm-up calls each, HIP events, calls alternated round by round",
             f"deband input: a ramp with noise; R = 16, T = 1311 changes {100 * changed:.1f} % of its pixels",
             f"{'call':36s} {'median us':>10s} {'p10':>8s} {'p90':>8s} {'MB':>7s} {'TB/s':>6s} {'of 8 TB/s':>9s}"]
    med = {}
    for k, (_, nbytes) in cases.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        lines.append(f"{k:36s} {med[k]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f} {nbytes / 1e6:7.1f} "
                     f"{nbytes / med[k] / 1e6:6.2f} {nbytes / med[k] * 1e6 / HBM_PEAK:9.2f}")
    for name in ("f16", "f32"):
        for kind in ("plain", "pq"):
            lines.append(f"fused {name} {kind}: dithered / undithered = {med[f'fused {name} {kind} dither 1'] / med[f'fused {name} {kind} dither 0']:.3f}")
    lines.append(f"from codes: dithered / undithered = {med['from codes dither 1'] / med['from codes dither 0']:.3f}")
    lines.append(f"deband + dither route: {med['route: post_rgb48 + deband + ex(1)']:.1f} us against {med['today: post_ycbcr10 f16']:.1f} us "
                 f"for today's one-launch {a.pix_fmt} (+{med['route: post_rgb48 + deband + ex(1)'] - med['today: post_ycbcr10 f16']:.1f} us per frame)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
