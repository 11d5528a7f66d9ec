#!/usr/bin/env python3
"""HG need lists (variant hg_sparse): a stream of frames of one kind through enqueue_frame, and the executed-tile shares.

  python tools/hg_sparse_stream.py --kind noise --frames 30 --sparse 2      # the worst case: ms per frame of a noise-only stream
                                                                             # (bench.py's own frames of that kind: seeds 1234 / 1236 noise, 1235 / 1237 gradient)
  python tools/hg_sparse_stream.py --kind gradient --seed0 1234             # two frames of that kind from seeds 1234 / 1236 instead
  python tools/hg_sparse_stream.py --shares --sparse 2                      # per HG layer, executed / dense tiles on bench.py's four frames

--sparse: 0 every tile, 1 need in 16x16 cells of every level, 2 (the default) in sub-tile units (csrc/hg_need.hip).

Prints one line per figure; run each invocation under a time limit of its own."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "hdr-realtime-video-pipeline_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="noise", choices=("noise", "gradient"))
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--sparse", type=int, default=2, choices=(0, 1, 2))
    ap.add_argument("--seed0", type=int, default=None, help="seed of the stream's first frame (the second: + 2); default bench.py's frames of --kind")
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--shares", action="store_true")
    a = ap.parse_args()
    import torch
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    h, w = a.height, a.width
    p = HDRTVNetMI355X(os.path.join(REPO, "tests", "golden", "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    dev = p.device
    try:
        if a.shares:
            # bench.py's frames: seeds 1234 .. 1237, noise and gradient alternating
            p.profile_enable(True)
            for i in range(4):
                kind = ("noise", "gradient")[i % 2]
                f = W.synthetic_frame(h, w, seed=1234 + i, kind=kind)
                prof = {}
                p.set_variant("hg_sparse", a.sparse or 2)
                p.infer(p.preprocess(f))
                m = p.tap("hg.mask")[0, :h, :w]
                print(f"shares {kind} {1234 + i} masked pixels {int(m.sum())} of {h * w} = {100.0 * float(m.sum()) / (h * w):.4f} %, "
                      f"16x16 cells holding one {100.0 * float((torch.nn.functional.max_pool2d(m[None, None], 16, ceil_mode=True) > 0).float().mean()):.3f} %")
                for sparse in (0, a.sparse or 2):
                    p.set_variant("hg_sparse", sparse)
                    p.infer(p.preprocess(f))
                    torch.cuda.synchronize(dev)
                    prof[min(sparse, 1)] = [r for r in p.profile_read() if r[0].startswith("hg.")]
                # executed / dense tiles of every launch that walked a list (conv_prw, conv_pglds, conv_glds1): read back from the device
                tiles = {r[0]: r[2:] for r in p.profile_tiles() if r[3]}
                for d, s in zip(prof[0], prof[1]):
                    assert d[0] == s[0], (d, s)
                    done, total = tiles.get(s[0], (1, 1))
                    print(f"shares {kind} {1234 + i} {d[0]:14s} {s[1]:18s} executed/dense tiles {done / total:6.3f}  ms {d[2]:6.3f} -> {s[2]:6.3f}")
                print(f"shares {kind} {1234 + i} HG layers total ms {sum(r[2] for r in prof[0]):6.3f} -> {sum(r[2] for r in prof[1]):6.3f}")
            return
        p.set_variant("hg_sparse", a.sparse)
        seed0 = a.seed0 if a.seed0 is not None else (1234 if a.kind == "noise" else 1235)          # bench.py's frames of that kind
        frames = [torch.from_numpy(W.synthetic_frame(h, w, seed=seed0 + 2 * i, kind=a.kind)).to(dev) for i in range(2)]
        out = torch.empty((h, w, 3), dtype=torch.uint16, device=dev)
        for i in range(5):
            p.enqueue_frame(0, frames[i % 2].data_ptr(), h, w, out.data_ptr())
        torch.cuda.synchronize(dev)
        for rep in range(3):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = p.lane_stream(0)
            torch.cuda.synchronize(dev)
            t0.record(st)
            for i in range(a.frames):
                p.enqueue_frame(0, frames[i % 2].data_ptr(), h, w, out.data_ptr())
            t1.record(st)
            torch.cuda.synchronize(dev)
            print(f"stream kind={a.kind} seeds={seed0},{seed0 + 2} hg_sparse={a.sparse} {h}x{w} frames={a.frames} rep={rep}: {t0.elapsed_time(t1) / a.frames:.3f} ms/frame")
    finally:
        p.close()


if __name__ == "__main__":
    main()
