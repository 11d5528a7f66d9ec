"""Device time of the film grain's entry points beside their twins without grain, in one session: hdrtv_post_rgb48 /
hdrtv_post_pq_rgb48 against hdrtv_post_rgb48_grain at the delivered size, hdrtv_post_rgb48_scaled_cas (plain passes without CAS, and
the reference's CAS code 3605 with anti-ringing 26 at 1080p) against hdrtv_post_rgb48_scaled_grain, hdrtv_post_rgb48_fsr (RCAS at 0.2)
against hdrtv_post_rgb48_fsr_grain, and hdrtv_rgb48_film_grain alone at both sizes.  HIP events around every call, warmed, the calls
alternated round by round so that clocks and cache state are shared.  f32 / f16 input, plain / PQ.

Each figure: median and p10 / p90 of the per-call times; then per form the cost of the grain in each fused kernel, and the fused
kernel against its twin followed by the standalone launch where that route exists (the delivered-size forms).

  python tools/film_grain_timing.py [--size 1920x1080] [--out-size 3840x2160] [--intensity 0.01] [--calls 50] [--warmup 10] [--out file.txt]
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
    ap.add_argument("--intensity", type=float, default=0.01)
    ap.add_argument("--cas", type=int, default=3605, help="the CAS code of the sharpened Lanczos pair, 1032 .. 4096")
    ap.add_argument("--antiring", type=int, default=26, help="its strength code, 0 .. 256")
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
    big32 = torch.from_numpy(rng.uniform(-0.1, 1.1, (3, oh, ow)).astype(np.float32)).cuda()
    small16, big16 = small32.half(), big32.half()
    dst = torch.empty((oh, ow, 3), dtype=torch.uint16, device="cuda")
    codes = torch.from_numpy(rng.integers(0, 65536, (oh, ow, 3), dtype=np.uint16)).cuda()
    d, pk, ar, k, inten, seed = dst.data_ptr(), a.peak_nits, a.antiring, a.cas, a.intensity, L.film_grain_seed(0, 1)
    forms = {"f32 plain": (small32, big32, L.F32, 0), "f16 plain": (small16, big16, L.F16, 0), "f32 pq": (small32, big32, L.F32, 1),
             "f16 pq": (small16, big16, L.F16, 1)}
    cases = {}
    cases["film_grain %dx%d" % (ow, oh)] = lambda: lib.hdrtv_rgb48_film_grain(ctx, st, codes.data_ptr(), oh, ow, inten, seed, d)
    cases["film_grain %dx%d" % (w, h)] = lambda: lib.hdrtv_rgb48_film_grain(ctx, st, codes.data_ptr(), h, w, inten, seed, d)
    for f, (ts, tb, dt, pq) in forms.items():
        full = (ctx, st, tb.data_ptr(), dt, oh, ow)
        base = (ctx, st, ts.data_ptr(), dt, h, w, pq, pk, d, oh, ow)
        if pq:
            cases["rgb48         " + f] = (lambda b=full: lib.hdrtv_post_pq_rgb48(*b, pk, d))
        else:
            cases["rgb48         " + f] = (lambda b=full: lib.hdrtv_post_rgb48(*b, d))
        cases["rgb48_grain   " + f] = (lambda b=full, pq=pq: lib.hdrtv_post_rgb48_grain(*b, pq, pk, d, inten, seed))
        cases["scaled        " + f] = (lambda b=base: lib.hdrtv_post_rgb48_scaled_cas(*b, 0, 0))
        cases["scaled_grain  " + f] = (lambda b=base: lib.hdrtv_post_rgb48_scaled_grain(*b, 0, 0, inten, seed))
        cases["cas+ar        " + f] = (lambda b=base: lib.hdrtv_post_rgb48_scaled_cas(*b, ar, k))
        cases["cas+ar_grain  " + f] = (lambda b=base: lib.hdrtv_post_rgb48_scaled_grain(*b, ar, k, inten, seed))
        cases["fsr           " + f] = (lambda b=base: lib.hdrtv_post_rgb48_fsr(*b, 1, 0.2))
        cases["fsr_grain     " + f] = (lambda b=base: lib.hdrtv_post_rgb48_fsr_grain(*b, 1, 0.2, inten, seed))
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
             f"unscaled pairs at {ow}x{oh}; scaled pairs {w}x{h} -> {ow}x{oh} (cas+ar: cas = {k} (code), antiring = {ar} (of 256); fsr: RCAS at 0.2); "
             f"intensity {inten}, {a.calls} rounds after {a.warmup} warm-up calls each, HIP events, calls alternated round by round",
             f"{'call':28s} {'median us':>10s} {'p10':>8s} {'p90':>8s}"]
    med = {}
    for c in cases:
        t = np.array(times[c])
        med[c] = float(np.median(t))
        lines.append(f"{c:28s} {med[c]:10.1f} {np.percentile(t, 10):8.1f} {np.percentile(t, 90):8.1f}")
    alone = med["film_grain %dx%d" % (ow, oh)]
    npx = ow * oh
    lines.append(f"film_grain {ow}x{oh}: {npx * 12 / alone / 1e3:.0f} GB/s of codes read + written ({npx * 12 / 1e6:.1f} MB), {npx / alone / 1e3:.0f} Gpixel/s")
    for f in forms:
        m = {n.strip(): med[n + f] for n in ("rgb48         ", "rgb48_grain   ", "scaled        ", "scaled_grain  ", "cas+ar        ", "cas+ar_grain  ",
                                             "fsr           ", "fsr_grain     ")}
        lines.append(f"{f}: rgb48_grain - rgb48 = {m['rgb48_grain'] - m['rgb48']:+.1f} us (twin + film_grain launch: {m['rgb48'] + alone:.1f} us, fused "
                     f"{m['rgb48_grain']:.1f}); scaled_grain - scaled = {m['scaled_grain'] - m['scaled']:+.1f} us; cas+ar_grain - cas+ar = "
                     f"{m['cas+ar_grain'] - m['cas+ar']:+.1f} us; fsr_grain - fsr = {m['fsr_grain'] - m['fsr']:+.1f} us (twin + film_grain launch: "
                     f"{m['fsr'] + alone:.1f} us, fused {m['fsr_grain']:.1f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    p.close()


if __name__ == "__main__":
    main()
