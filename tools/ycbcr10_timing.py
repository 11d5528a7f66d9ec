"""Device time of the 10-bit Y'CbCr output kernels against the RGB48 post kernels at the same size, HIP events around every call,
warmed, the calls alternated round by round so that clocks and cache state are shared (the method of tools/rgb48_scale_timing.py):

  hdrtv_post_ycbcr10          f32 / f16 input, plain / PQ      one kernel: reads 3 planes, writes 3 B per pixel (4:2:0)
  hdrtv_post_rgb48 / hdrtv_post_pq_rgb48                      the yardsticks: read 3 planes, write 6 B per pixel
  ... the same two from --parent-lib                           the library built from the parent commit, loaded beside this one
  post_rgb48 + hdrtv_rgb48_to_ycbcr10                          the two-launch form: writes 6 B, re-reads them, writes 3 B per pixel

Each figure: median and p10 / p90 of the per-call times, and the algorithmic bytes / time against 8 TB/s.

  python tools/ycbcr10_timing.py [--size 3840x2160] [--pix-fmt p010le] [--siting left] [--calls 50] [--warmup 10]
                                 [--parent-lib path/to/libhdrtv_mi355x.so] [--out file.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hdr-realtime-video-pipeline_amd"))
HBM_PEAK = 8.0e12


def parent_calls(path, st, t32, dst, h, w, peak):
    """post_rgb48 / post_pq_rgb48 of another build of the library (its own context on the same device)."""
    so = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    so.hdrtv_create.restype = i
    so.hdrtv_create.argtypes = [vp, C.c_size_t, vp, C.c_size_t, i, C.POINTER(vp)]
    so.hdrtv_post_rgb48.restype = so.hdrtv_post_pq_rgb48.restype = i
    so.hdrtv_post_rgb48.argtypes = [vp, vp, vp, i, i, i, vp]
    so.hdrtv_post_pq_rgb48.argtypes = [vp, vp, vp, i, i, i, C.c_float, vp]
    so.hdrtv_version.restype = C.c_char_p
    blob = open(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), "rb").read()
    ctx = vp()
    rc = so.hdrtv_create(blob, len(blob), None, 0, 0, C.byref(ctx))
    if rc != 0:
        raise RuntimeError(f"hdrtv_create of {path} failed ({rc})")
    return so.hdrtv_version().decode(), {
        "parent post_rgb48 f32": (lambda: so.hdrtv_post_rgb48(ctx, st, t32.data_ptr(), 1, h, w, dst), h * w * 18),
        "parent post_pq_rgb48 f32": (lambda: so.hdrtv_post_pq_rgb48(ctx, st, t32.data_ptr(), 1, h, w, peak, dst), h * w * 18),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--pix-fmt", default="p010le")
    ap.add_argument("--siting", default="left")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--peak-nits", type=float, default=1000.0)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    w, h = (int(v) for v in a.size.lower().split("x"))
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t32 = torch.from_numpy(np.random.default_rng(0).uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)).cuda()
    t16 = t32.half()
    rgb = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    ycc_b = L.out_frame_bytes(a.pix_fmt, h, w)
    ycc = torch.empty((ycc_b // 2,), dtype=torch.uint16, device="cuda")
    planes = L.ycbcr10_planes(ycc.data_ptr(), h, w, a.pix_fmt, a.siting)
    d, pk, px = rgb.data_ptr(), a.peak_nits, h * w

    def two(pq):
        rc = lib.hdrtv_post_pq_rgb48(ctx, st, t32.data_ptr(), L.F32, h, w, pk, d) if pq else lib.hdrtv_post_rgb48(ctx, st, t32.data_ptr(), L.F32, h, w, d)
        return rc or lib.hdrtv_rgb48_to_ycbcr10(ctx, st, d, h, w, *planes)

    cases = {
        "fused f32 plain": (lambda: lib.hdrtv_post_ycbcr10(ctx, st, t32.data_ptr(), L.F32, h, w, 0, 0.0, *planes), px * 12 + ycc_b),
        "fused f16 plain": (lambda: lib.hdrtv_post_ycbcr10(ctx, st, t16.data_ptr(), L.F16, h, w, 0, 0.0, *planes), px * 6 + ycc_b),
        "fused f32 pq": (lambda: lib.hdrtv_post_ycbcr10(ctx, st, t32.data_ptr(), L.F32, h, w, 1, pk, *planes), px * 12 + ycc_b),
        "fused f16 pq": (lambda: lib.hdrtv_post_ycbcr10(ctx, st, t16.data_ptr(), L.F16, h, w, 1, pk, *planes), px * 6 + ycc_b),
        "post_rgb48 f32": (lambda: lib.hdrtv_post_rgb48(ctx, st, t32.data_ptr(), L.F32, h, w, d), px * 18),
        "post_pq_rgb48 f32": (lambda: lib.hdrtv_post_pq_rgb48(ctx, st, t32.data_ptr(), L.F32, h, w, pk, d), px * 18),
        "rgb48_to_ycbcr10 alone": (lambda: lib.hdrtv_rgb48_to_ycbcr10(ctx, st, d, h, w, *planes), px * 6 + ycc_b),
        "two launches f32 plain": (lambda: two(0), px * 24 + ycc_b),
        "two launches f32 pq": (lambda: two(1), px * 24 + ycc_b),
    }
    parent = None
    if a.parent_lib:
        parent, extra = parent_calls(a.parent_lib, st, t32, d, h, w, pk)
        cases.update(extra)
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
    lines = [f"{torch.cuda.get_device_name(0)}; {lib.hdrtv_version().decode()}"]
    if parent:
        lines.append(f"parent library, loaded beside it in the same process: {parent}")
    lines += [f"{w}x{h} {a.pix_fmt} siting {a.siting}, {a.calls} rounds after {a.warmup} warm-up calls each, HIP events, calls alternated round by round",
              f"{'call':28s} {'median us':>10s} {'p10':>8s} {'p90':>8s} {'MB':>7s} {'TB/s':>6s} {'of 8 TB/s':>9s}"]
    med = {}
    for k, (_, nbytes) in cases.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        lines.append(f"{k:28s} {med[k]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f} {nbytes / 1e6:7.1f} "
                     f"{nbytes / med[k] / 1e6:6.2f} {nbytes / med[k] * 1e6 / HBM_PEAK:9.2f}")
    ref = "parent " if parent else ""
    lines.append(f"fused f32 plain: {med['fused f32 plain'] / med['two launches f32 plain']:.2f} x the two-launch form, "
                 f"{med['fused f32 plain'] / med[ref + 'post_rgb48 f32']:.2f} x {ref}post_rgb48")
    lines.append(f"fused f32 pq: {med['fused f32 pq'] / med['two launches f32 pq']:.2f} x the two-launch form, "
                 f"{med['fused f32 pq'] / med[ref + 'post_pq_rgb48 f32']:.2f} x {ref}post_pq_rgb48")
    lines.append(f"D2H bytes per frame: rgb48le {px * 6} -> {a.pix_fmt} {ycc_b}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
