"""HG need lists (variant hg_sparse, csrc/hg_need.hip): the head computes only the tiles the highlight mask lets reach the output.

The output must not change by a bit: every GPU case runs one frame twice on one context, hg_sparse = 0 then 1, and compares the
whole tensor with torch.equal.  Between the two runs a DIFFERENT image runs over every tile (_pollute), so a tile the sparse run
skips holds another frame's values: a needed tile that was wrongly skipped shows.  Each case asserts the mask it was written for from the hg.mask tap (a failed precondition fails).
The CPU test holds the propagation rules -- mirrored in numpy from the layer table of csrc/api.h -- against a per-pixel
receptive-field computation: the needed cells must cover the true dependency set at every layer."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ the rules, on the CPU
def _layer_table():
    """hg_layers of csrc/api.h: [(name, ks, mode, level, in, skip, out)], mode 0 same level / 1 pool-fused / 2 pixel shuffle."""
    src = open(os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc", "api.h")).read()
    body = src.split("inline constexpr HgLayer hg_layers[] = {", 1)[1].split("};", 1)[0]
    rows = []
    for m in re.finditer(r'\{"(\w+)", (\d+), (\d+), (\d+), (\d), (\d+), (ST_\w+), ACT_\w+, (\d), ("\w+"|nullptr), ("\w+"|nullptr), ("\w+"|nullptr),', body):
        name, _, _, _, ks, ps, mode, level, tin, skip, out = m.groups()
        unq = lambda s: None if s == "nullptr" else s.strip('"')
        rows.append((name, int(ks), 1 if mode == "ST_POOL" else (2 if int(ps) else 0), int(level), unq(tin), unq(skip), unq(out) or "part"))
    assert len(rows) == 18 and rows[0][0] == "conv2" and rows[-1][0] == "Up_conv5", [r[0] for r in rows]
    return rows


def _dilate(a):
    p = np.pad(a, 1)
    out = np.zeros_like(a)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + a.shape[0], dx:dx + a.shape[1]]
    return out


def _down_any(a, shape):
    """any-of-2x2: a at level l -> `shape` at level l + 1"""
    p = np.zeros((2 * shape[0], 2 * shape[1]), bool)
    p[:a.shape[0], :a.shape[1]] = a
    return p.reshape(shape[0], 2, shape[1], 2).any(axis=(1, 3))


def _up2(a, shape):
    return np.repeat(np.repeat(a, 2, 0), 2, 1)[:shape[0], :shape[1]]


def _propagate(flags, Hp, Wp, unit):
    """hg_need's rules on maps of `unit` x `unit` pixels per element (16: the kernel's cells, 1: per pixel = the true dependency set).
    Returns {layer: K, the elements the layer computes}."""
    size = lambda lev: (-(-(Hp >> lev) // unit), -(-(Wp >> lev) // unit))
    need = {"part": flags}
    K = {}
    for name, ks, mode, level, tin, skip, out in reversed(_layer_table()):
        o = need[out]
        k = _up2(o, size(level)) if mode == 1 else (_down_any(o, size(level)) if mode == 2 else o)
        assert k.shape == size(level), (name, k.shape, size(level))
        K[name] = k
        reads = _dilate(k) if ks == 3 else k
        for t in (tin, skip):
            if t is not None:
                need[t] = need.get(t, np.zeros(size(level), bool)) | reads
    return K


def _true_pixels(mask):
    """The conv-output pixels every layer must compute for the masked output pixels, per pixel and written out by hand from the
    generator's forward (Hallucination_arch.py: five conv / conv+pool encoder stages, code, five Up blocks with 1x1 fuse convs over
    the skip concat) -- on purpose neither the layer table nor _propagate.  Sizes are multiples of 32."""
    d = _dilate
    up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)                      # pooled pixel -> its 2x2 pre-pool pixels
    dn = lambda a: a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2).any(axis=(1, 3))      # shuffled 2x2 pixels -> their source pixel
    K = {}
    # decoder, from the output back: out = mask * conv10(cat(conv1, shuffle(Up_conv5(conv9)))) + img
    K["Up_conv5"] = dn(mask)
    K["conv9"] = d(K["Up_conv5"])                  # 1x1 over cat(shuffle(Up_conv4(conv8)), conv2)
    K["Up_conv4"] = dn(K["conv9"])
    K["conv8"] = d(K["Up_conv4"])                  # ... cat(shuffle(Up_conv3(conv7)), conv3_2)
    K["Up_conv3"] = dn(K["conv8"])
    K["conv7"] = d(K["Up_conv3"])                  # ... cat(shuffle(Up_conv2(conv6)), conv4_2)
    K["Up_conv2"] = dn(K["conv7"])
    K["conv6"] = d(K["Up_conv2"])                  # ... cat(shuffle(Up_conv1(conv_code2)), conv5_2)
    K["Up_conv1"] = dn(K["conv6"])
    K["conv_code2"] = d(K["Up_conv1"])
    # encoder, from the code back up: each stage is read by the next one (3x3, through the pool) and by its fuse conv
    K["conv_code1"] = up(d(K["conv_code2"]))
    K["conv5_2"] = K["conv6"] | d(K["conv_code1"])
    K["conv5_1"] = up(d(K["conv5_2"]))
    K["conv4_2"] = K["conv7"] | d(K["conv5_1"])
    K["conv4_1"] = up(d(K["conv4_2"]))
    K["conv3_2"] = K["conv8"] | d(K["conv4_1"])
    K["conv3_1"] = up(d(K["conv3_2"]))
    K["conv2"] = K["conv9"] | d(K["conv3_1"])
    return K


def _cells_of(px):
    """the 16x16 cells that hold a set pixel"""
    h, w = px.shape
    return np.pad(px, ((0, -h % 16), (0, -w % 16))).reshape(-(-h // 16), 16, -(-w // 16), 16).any(axis=(1, 3))


def test_need_rules_cover_the_true_dependency_set():
    Hp, Wp = 1056, 1568                 # 33 x 49 pixels at the deepest level: several cells everywhere, ragged last cells
    rng = np.random.default_rng(7)
    mask = np.zeros((Hp, Wp), bool)
    mask[rng.integers(0, Hp, 12), rng.integers(0, Wp, 12)] = True          # single pixels
    mask[400:420, 900:1000] = True                                          # a blob
    mask[Hp - 1, Wp - 1] = mask[0, 0] = True                                # the corners
    cells, true = _propagate(_cells_of(mask), Hp, Wp, 16), _true_pixels(mask)
    assert set(cells) == set(true)
    print()
    for name, _, _, level, *_ in _layer_table():
        k, t = cells[name], true[name]
        assert t.shape == (Hp >> level, Wp >> level), (name, t.shape)
        cover = np.repeat(np.repeat(k, 16, 0), 16, 1)[:t.shape[0], :t.shape[1]]
        assert not (t & ~cover).any(), (name, int((t & ~cover).sum()))
        print(f"  {name:11s} level {level}: {int(k.sum()):5d} of {k.size:5d} cells needed, {int(_cells_of(t).sum()):5d} hold a pixel that is, "
              f"{cover.sum() / max(1, t.sum()):6.2f} x the pixels that are")
    # the first step back from the output only rounds to cells: there the needed cells are exactly the cells of the true set.  Every
    # further 3x3 step may add one ring of cells to it (the figures above record how much that is per layer).
    assert np.array_equal(cells["Up_conv5"], _cells_of(true["Up_conv5"]))


# ------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
    return torch


def _make(golden_dir, **kw):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    return HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0, **kw)


def _frame(kind, h, w, seed):
    from hdrtv_mi355x import weights as W
    return np.zeros((h, w, 3), np.uint8) if kind == "zero" else W.synthetic_frame(h, w, seed=seed, kind=kind)


def _infer(p, frame, sparse):
    p.set_variant("hg_sparse", sparse)
    out, _ = p.infer(p.preprocess(frame))
    return out.clone()


def _mask_fraction(p, h, w):
    m = p.tap("hg.mask")[0, :h, :w]
    return float(m.sum()) / (h * w), int(m.sum())


def _pollute(p, h, w):
    """Another image (noise) through every tile of every HG tensor of the lane: nothing of the frame under test is left behind."""
    _infer(p, _frame("noise", h, w, 977), 0)


def _dense_then_sparse(p, frame, check):
    h, w = frame.shape[:2]
    dense = _infer(p, frame, 0)
    frac, n = _mask_fraction(p, h, w)
    print(f"  mask: {n} pixels, {100 * frac:.3f} %")
    check(frac, n)
    _pollute(p, h, w)
    sparse = _infer(p, frame, 1)
    return dense, sparse


CASES = {
    "gradient11": ("gradient", 540, 960, 11, None, lambda f, n: 0 < f < 0.05),
    "gradient11_r0.3": ("gradient", 540, 960, 11, 0.3, lambda f, n: f >= 0.5),
    "gradient61": ("gradient", 540, 960, 61, None, lambda f, n: n > 0 and f < 1e-4),
    "zero_small": ("zero", 128, 192, 0, None, lambda f, n: n == 0),
    "zero": ("zero", 540, 960, 0, None, lambda f, n: n == 0),
    "noise3": ("noise", 272, 480, 3, None, lambda f, n: n > 0),
}


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_sparse_output_is_the_dense_output(torch_cuda, golden_dir, case):
    torch = torch_cuda
    kind, h, w, seed, mask_r, pre = CASES[case]
    frame = _frame(kind, h, w, seed)
    p = _make(golden_dir)
    try:
        if mask_r is not None:
            p.set_hg_mask_r(mask_r)

        def check(f, n):
            assert pre(f, n), (case, f, n)
        dense, sparse = _dense_then_sparse(p, frame, check)
        assert torch.equal(dense, sparse), (case, int((dense != sparse).sum()))
        assert torch.isfinite(sparse).all()
    finally:
        p.close()


@gpu
def test_sparse_rgb48_and_graph_replay_are_the_dense_bytes(torch_cuda, golden_dir):
    torch = torch_cuda
    h, w = 540, 960
    frame = _frame("gradient", h, w, 11)
    p = _make(golden_dir)
    try:
        dev = p.device
        f = torch.from_numpy(frame).to(dev)
        noise = torch.from_numpy(_frame("noise", h, w, 977)).to(dev)
        got = []
        for sparse, src in ((0, f), (0, noise), (1, f)):        # dense, another image over every tile, sparse
            p.set_variant("hg_sparse", sparse)
            o = torch.zeros((h, w, 3), dtype=torch.uint16, device=dev)
            p.enqueue_frame(0, src.data_ptr(), h, w, o.data_ptr())
            torch.cuda.synchronize(dev)
            got.append(o)
        got = [got[0], got[2]]
        frac, n = _mask_fraction(p, h, w)
        assert 0 < frac < 0.05, frac
        assert torch.equal(got[0], got[1]), int((got[0] != got[1]).sum())
        other = _frame("gradient", h, w, 61)
        want, want_other = _infer(p, frame, 0), _infer(p, other, 0)
        assert not torch.equal(want, want_other)
    finally:
        p.close()
    p = _make(golden_dir, use_cuda_graphs=True)
    try:
        p.set_variant("hg_sparse", 1)
        # the first call captures the graph; the replays' lists follow each frame's content (counts and lists stay on the device)
        for fr, ref in ((other, want_other), (frame, want), (other, want_other), (frame, want)):
            out, _ = p.infer(p.preprocess(fr))
            assert torch.equal(out, ref), int((out != ref).sum())
        assert p._graphs, "infer did not run from a captured graph"
    finally:
        p.close()


@gpu
def test_taps_after_a_sparse_frame_are_the_whole_tensors(torch_cuda, golden_dir):
    torch = torch_cuda
    h, w = 540, 960
    frame = _frame("gradient", h, w, 11)
    names = ("hg.conv2", "hg.conv5_2", "hg.conv9", "hg.part")
    p = _make(golden_dir)
    try:
        want = _infer(p, frame, 0)
        frac, _ = _mask_fraction(p, h, w)
        assert 0 < frac < 0.05, frac
        dense = {n: p.tap(n) for n in names}
        # another image over every tile in between: a tile the sparse frame skips cannot still hold this frame's dense values
        _pollute(p, h, w)
        out = _infer(p, frame, 1)
        assert torch.equal(out, want), int((out != want).sum())
        for n in names:
            t = p.tap(n)
            assert torch.equal(t, dense[n]), (n, int((t != dense[n]).sum()))
        # completing the taps leaves the frame's output alone, and the next frame is sparse again
        assert torch.equal(out, p._gpu_out)
        assert torch.equal(_infer(p, frame, 1), out)
    finally:
        p.close()


@gpu
def test_stale_tiles_of_an_earlier_frame_do_not_reach_the_output(torch_cuda, golden_dir):
    torch = torch_cuda
    h, w = 540, 960
    frame = _frame("gradient", h, w, 11)
    p = _make(golden_dir)
    try:
        want = _infer(p, frame, 0).cpu()
    finally:
        p.close()
    p = _make(golden_dir)
    try:
        p.set_hg_mask_r(0.3)                       # a dense frame of ANOTHER image: every list full, every tile holds its values
        _infer(p, _frame("gradient", h, w, 61), 1)
        frac, _ = _mask_fraction(p, h, w)
        assert frac >= 0.5, frac
        p.set_hg_mask_r(0.75)
        got = _infer(p, frame, 1)
        frac, _ = _mask_fraction(p, h, w)
        assert 0 < frac < 0.05, frac
        assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    finally:
        p.close()


def _need_plan(Hp, Wp):
    """hg_need_plan's layout of the hg.need buffer (csrc/api_graph.hip): {layer: byte offset of its list}."""
    ncell = lambda lev: (-(-(Hp >> lev) // 16)) * (-(-(Wp >> lev) // 16))
    off = 0

    def take(n):
        nonlocal off
        o, off = off, (off + n + 15) & ~15
        return o
    take(ncell(0))                                  # flags
    take(ncell(0))                                  # the layer's own cells
    seen = {"part"}
    table = _layer_table()
    for name, ks, mode, level, tin, skip, out in table:
        for t, lev in ((tin, level), (skip, level), (out, level + (mode == 1) - (mode == 2))):
            if t is not None and t not in seen:
                seen.add(t)
                take(ncell(lev))
    return {name: take(4 * (2 * ncell(level) + 4)) for name, _, _, level, *_ in table}


@gpu
@pytest.mark.parametrize("kind,h,w,seed", [("gradient", 540, 960, 11), ("noise", 272, 480, 3), ("gradient", 540, 960, 61)])
def test_device_lists_are_the_rules_applied_to_the_frames_mask(torch_cuda, golden_dir, kind, h, w, seed):
    """hg_need.hip's own output, read back from hg.need after a sparse frame, against the numpy mirror of the rules on that frame's
    mask: per layer the count and the set of tiles, in 16-row tiles (one per cell) or 8-row tiles (two per cell, the second only
    where the map has that tile row) -- whichever the layer's kernel uses."""
    Hp, Wp = -(-h // 32) * 32, -(-w // 32) * 32
    p = _make(golden_dir)
    try:
        _infer(p, _frame(kind, h, w, seed), 1)
        mask = p.tap("hg.mask")[0].numpy() > 0
        buf = p.tap("hg.need").numpy().astype(np.uint8).ravel()
    finally:
        p.close()
    mask[h:, :] = False
    mask[:, w:] = False
    want = _propagate(_cells_of(mask), Hp, Wp, 16)
    offs = _need_plan(Hp, Wp)
    eight = 0
    for name, _, _, level, *_ in _layer_table():
        k = want[name]
        gh, gw = k.shape
        n = int(buf[offs[name]:offs[name] + 4].view(np.int32)[0])
        assert 0 <= n <= 2 * k.size, (name, n)
        got = buf[offs[name] + 4:offs[name] + 4 + 4 * n].view(np.int32)
        cells16 = sorted(np.flatnonzero(k).tolist())
        ty8 = -(-(Hp >> level) // 8)
        tiles8 = sorted(t for c in cells16 for t in ([2 * (c // gw) * gw + c % gw] + ([(2 * (c // gw) + 1) * gw + c % gw] if 2 * (c // gw) + 1 < ty8 else [])))
        assert sorted(got.tolist()) in (cells16, tiles8), (name, n, len(cells16), len(tiles8))
        assert len(set(got.tolist())) == n, name
        eight += sorted(got.tolist()) == tiles8 and tiles8 != cells16
    print(f"  {eight} layers listed in 8-row tiles")
