"""Device time of the tone map's entry points beside their unchanged twins, in one session: hdrtv_rgb48_tonemap alone, the fused
hdrtv_post_rgb48_tonemap from f16 and from f32 (plain and PQ), and beside them hdrtv_post_rgb48 (the plain twin) and
hdrtv_post_pq_rgb48 -- which does the same three table walks per pixel and so is the yardstick for what the walks cost.  Two sizes
(3840x2160, 1920x1080) and two contents: uniform random values, the worst case for the three 256 KiB tables (every gather and every
walk lands on another cache line), and a smooth picture (a diagonal ramp with a little noise), where neighbouring pixels share
lines as they do in video.  HIP events around every call, warmed, the calls alternated round by round so that clocks and cache
state are shared.

Each figure: median and p10 / p90 of the per-call times; then the fused form against its twin followed by the standalone launch.

  python tools/tonemap_timing.py [--sizes 3840x2160,1920x1080] [--curve spline] [--target-peak 600] [--calls 50] [--warmup 10] [--out file.txt]
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
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--curve", default="spline")
    ap.add_argument("--target-peak", type=float, default=600.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--peak-nits", type=float, default=1000.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import lib as L
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    lib, ctx = p._lib, p._ctx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tone = L.tone_mapping(a.curve, a.target_peak)
    gain = p._tone_gain(tone)
    rng = np.random.default_rng(0)
    pk = a.peak_nits
    cases, keep = {}, []
    sizes = [tuple(int(v) for v in s.lower().split("x")) for s in a.sizes.split(",")]
    for w, h in sizes:
        ramp = (np.add.outer(np.arange(h), np.arange(w)) / float(h + w)).astype(np.float32)
        contents = {"random": rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32),
                    "smooth": (ramp[None] * np.array([1.0, 0.8, 0.6], np.float32)[:, None, None]
                               + rng.normal(0.0, 0.002, (3, h, w)).astype(np.float32))}
        for cn, x in contents.items():
            t32 = torch.from_numpy(x).cuda()
            t16 = t32.half()
            dst = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
            codes = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
            assert lib.hdrtv_post_rgb48(ctx, st, t32.data_ptr(), L.F32, h, w, codes.data_ptr()) == 0
            keep += [t32, t16, dst, codes]
            tag, d = "%dx%d %s" % (w, h, cn), dst.data_ptr()
            cases["tonemap            " + tag] = (lambda c=codes.data_ptr(), h=h, w=w, d=d: lib.hdrtv_rgb48_tonemap(ctx, st, c, h, w, gain, d))
            for f, t, dt in (("f32", t32, L.F32), ("f16", t16, L.F16)):
                b = (ctx, st, t.data_ptr(), dt, h, w)
                cases["rgb48 %s          " % f + tag] = (lambda b=b, d=d: lib.hdrtv_post_rgb48(*b, d))
                cases["rgb48_tonemap %s  " % f + tag] = (lambda b=b, d=d: lib.hdrtv_post_rgb48_tonemap(*b, 0, pk, gain, d))
                cases["pq_rgb48 %s       " % f + tag] = (lambda b=b, d=d: lib.hdrtv_post_pq_rgb48(*b, pk, d))
                cases["pq_rgb48_tonemap %s " % f[:3] + tag] = (lambda b=b, d=d: lib.hdrtv_post_rgb48_tonemap(*b, 1, pk, gain, d))
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
             f"curve {tone.kind} {tone.source_peak:g} -> {tone.target_peak:g} nits; {a.calls} rounds after {a.warmup} warm-up calls each, HIP events, "
             f"calls alternated round by round",
             f"{'call':44s} {'median us':>10s} {'p10':>8s} {'p90':>8s}"]
    med = {}
    for c in cases:
        t = np.array(times[c])
        med[c] = float(np.median(t))
        lines.append(f"{c:44s} {med[c]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f}")
    for w, h in sizes:
        for cn in ("random", "smooth"):
            tag = "%dx%d %s" % (w, h, cn)
            alone = med["tonemap            " + tag]
            npx = w * h
            lines.append(f"{tag}: tonemap alone {npx * 12 / alone / 1e3:.0f} GB/s of codes read + written ({npx * 12 / 1e6:.1f} MB), "
                         f"{npx / alone / 1e3:.1f} Gpixel/s")
            for f in ("f32", "f16"):
                tw, fu = med["rgb48 %s          " % f + tag], med["rgb48_tonemap %s  " % f + tag]
                ptw, pfu = med["pq_rgb48 %s       " % f + tag], med["pq_rgb48_tonemap %s " % f + tag]
                lines.append(f"  {f}: plain twin + tonemap launch {tw + alone:.1f} us, fused {fu:.1f} ({fu - tw:+.1f} over the twin); "
                             f"pq twin + tonemap launch {ptw + alone:.1f} us, fused {pfu:.1f} ({pfu - ptw:+.1f} over the twin)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
