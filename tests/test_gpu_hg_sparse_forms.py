"""HG need lists, second file: every conv_prw form, long runs, the launcher's dense fallback and masks placed on purpose.

tests/test_gpu_hg_sparse.py runs whatever forms the cost heuristic picks at three sizes, with masks where the synthetic blobs fall.
Here the frames are built: uniform background 40 with 4x4 blocks of 255.  On the CPU oracle such a block is masked (14 - 16 of its
16 pixels; LE output 0.86 - 0.97 inside, 0.20 outside, threshold 0.775) and nothing else is, so the set of 16x16 cells that hold a
masked pixel is exactly the set of cells the blocks touch: test_placed_blocks_mask_exactly_their_cells pins that on the CPU, and
every GPU case asserts it from the hg.mask tap before it compares anything.

  A       536 x 1000 (padded 544 x 1024: 8 rows / 24 columns beyond H x W; 17 tile rows of 8 at level 2; 2 x 2 cells at level 5).
          Blocks at the four corners of H x W, at (12, 14) (columns straddle x = 16), at (250, 510) (straddles x = 512, the border
          of the deepest level's cells) and at (318, 222) (straddles y = 320 and x = 224, borders of the level-1 cells too).
  A2      the same size, other positions (the second lane's frame)
  A_full  536 x 1000, all 255: every pixel masked at the default mask_r = 0.75 (LE output 0.80 - 0.86)
  B       72 x 104 (96 x 128): the deep layers have fewer than 8 tiles, conv_prw_launch drops their lists (grid < 8)
  S       136 x 200, the size of the CPU test
  W       72 x 1600 (96 x 1600), blocks in the leftmost 512 columns.  Not in the issue's list: with 2 x 2 cells at the deepest level
          (A) one needed cell dilates to the whole map, and from there every encoder layer is needed everywhere -- no frame of A's
          size gives conv3_1 .. conv_code2 (the <pool> and <nhwc> forms) a partial list.  W has 1 x 4 cells at level 5, so
          conv_code2 needs 2 of 4 and conv_code1 6 of 7.
  BIG     1152 x 2048, once: conv3_1 has 72 x 64 = 4608 8-row tiles, a run on 8 workgroups is 577 > LIST_N = 512

Reference of every bit-for-bit comparison: the same frame on the same context with hg_sparse = 0 and prw = 0 (conv_pglds on every
3x3 layer, no list anywhere).  Between reference and sparse run another image runs over every tile (_pollute)."""
import os
import re

import numpy as np
import pytest

from test_gpu_hg_sparse import REPO, _cells_of, _frame, _layer_table, _make, _need_plan, _pollute, _propagate
from test_gpu_parity import HG_OUT_MAX

gpu = pytest.mark.gpu

FRAMES = {
    "A": (536, 1000, ((0, 0), (0, 996), (532, 0), (532, 996), (12, 14), (250, 510), (318, 222))),
    "A2": (536, 1000, ((100, 100), (20, 700), (400, 508), (500, 30), (270, 990))),
    "A_full": (536, 1000, None),
    "B": (72, 104, ((0, 0), (68, 100), (34, 50))),
    "S": (136, 200, ((0, 0), (132, 196), (60, 100))),
    "W": (72, 1600, ((0, 0), (34, 20))),
    "BIG": (1152, 2048, ((0, 0), (600, 40), (1148, 300))),
    "B0": (72, 104, ()),                     # no highlight: every list is empty, so a launch that reports MACs did not walk its list
    "BIG0": (1152, 2048, ()),
}
PRW_FORMS = ("conv_prw<nhwc>", "conv_prw<pool>", "conv_prw<ps>", "conv_prw<ps_dot3>", "conv_prw8<nhwc>", "conv_prw8<pool>", "conv_prw8<ps>")


def placed_frame(h, w, blocks, bg=40):
    """u8 BGR: uniform `bg`, a 4x4 block of 255 with its top left pixel at each (y, x)"""
    f = np.full((h, w, 3), bg, np.uint8)
    for y, x in blocks:
        assert 0 <= y <= h - 4 and 0 <= x <= w - 4, (y, x)
        f[y:y + 4, x:x + 4] = 255
    return f


def _build(name):
    h, w, blocks = FRAMES[name]
    return np.full((h, w, 3), 255, np.uint8) if blocks is None else placed_frame(h, w, blocks)


def _block_cells(name):
    """the 16x16 cells of the padded frame that the frame's blocks touch"""
    h, w, blocks = FRAMES[name]
    m = np.zeros((-(-h // 32) * 32, -(-w // 32) * 32), bool)
    if blocks is None:
        m[:h, :w] = True
    for y, x in blocks or ():
        m[y:y + 4, x:x + 4] = True
    return _cells_of(m)


def _layer_dims():
    """{layer: (cout, cin, ks)} of hg_layers (csrc/api.h)"""
    src = open(os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc", "api.h")).read()
    body = src.split("inline constexpr HgLayer hg_layers[] = {", 1)[1].split("};", 1)[0]
    return {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r'\{"(\w+)", (\d+), (\d+), \d+, (\d),', body)}


# ------------------------------------------------------------------------------------------------------------------------- CPU
def test_placed_blocks_mask_exactly_their_cells(hr_state):
    """The builder's contract, on the CPU oracle: the cells that hold a masked pixel are the cells the blocks touch (136 x 200 and
    72 x 104; 536 x 1000 and 72 x 1600 give the same, 5 s and 2 s of oracle time -- every GPU case asserts it at its own size)."""
    from oracle import hdrtvnet_oracle as O
    print()
    for name in ("S", "B"):
        h, w, blocks = FRAMES[name]
        base, _ = O.hr_forward(hr_state, *O.preprocess(_build(name)))
        mask = O.hg_mask(base)[0] > 0
        per_block = [int(mask[y:y + 4, x:x + 4].sum()) for y, x in blocks]
        print(f"  {name}: {int(mask.sum())} masked pixels, per block {per_block}, background {float(np.median(base)):.3f}, peak {float(base.max()):.3f}")
        assert all(n >= 12 for n in per_block), per_block
        assert np.array_equal(_cells_of(np.pad(mask, ((0, -h % 32), (0, -w % 32)))), _block_cells(name)), name
    one = placed_frame(136, 200, ())
    one[60, 100] = 255                              # a single pixel stays below the threshold: blocks, not pixels
    base, _ = O.hr_forward(hr_state, *O.preprocess(one))
    assert not O.hg_mask(base).any()


def test_frame_a_is_sparse_and_the_wide_frame_cuts_the_encoder():
    """The caps that keep a sparse case from being a dense one, from the cells the blocks touch (= the mask's cells, see above):
    frame A's Up_conv5 list holds < 10 % of the layer's tiles and conv9 needs < 15 %.  Per-layer counts are printed."""
    print()
    K = {}
    for name in ("A", "W", "BIG", "B"):
        h, w, _ = FRAMES[name]
        K[name] = _propagate(_block_cells(name), -(-h // 32) * 32, -(-w // 32) * 32, 16)
        print(f"  {name} ({h} x {w}): " + ", ".join(f"{n} {int(k.sum())}/{k.size}" for n, k in reversed(list(K[name].items()))))
    assert K["A"]["Up_conv5"].mean() < 0.10 and K["A"]["conv9"].mean() < 0.15
    # A: the deepest level has 2 x 2 cells, the encoder is needed everywhere; W: its deep encoder layers are partial
    assert all(K["A"][n].all() for n in ("conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5_1", "conv5_2", "conv_code1", "conv_code2"))
    assert 0 < K["W"]["conv_code1"].sum() < K["W"]["conv_code1"].size and 0 < K["W"]["conv_code2"].sum() < K["W"]["conv_code2"].size


# ------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
    return torch


def _set(p, sparse, prw=1, nt=3, ncu=0):
    p.set_variant("hg_sparse", sparse)
    p.set_variant("prw", prw)
    p.set_variant("pglds_nt_slow", nt)
    p.set_variant("force_ncu", ncu)


def _out(p, frame):
    out, _ = p.infer(p.preprocess(frame))
    return out.clone()


def _rgb48(torch, p, frame, lane=0):
    h, w = frame.shape[:2]
    f = torch.from_numpy(frame).to(p.device)
    o = torch.zeros((h, w, 3), dtype=torch.uint16, device=p.device)
    torch.cuda.synchronize(p.device)
    p.enqueue_frame(lane, f.data_ptr(), h, w, o.data_ptr())
    torch.cuda.synchronize(p.device)
    return o


def _mask(p, name):
    """The hg.mask tap inside H x W, after the precondition of every case: its cells are the cells the frame was built for."""
    h, w, blocks = FRAMES[name]
    m = p.tap("hg.mask")[0].numpy() > 0
    m[h:, :] = False
    m[:, w:] = False
    if blocks is None:
        frac = m.sum() / (h * w)
        assert frac >= 0.99, (name, frac)             # mask_r = 0.75, the default
    assert np.array_equal(_cells_of(m), _block_cells(name)), (name, int(m.sum()))
    return m


def _same(torch, got, want, what):
    if not torch.equal(got, want):
        d = (got.float() - want.float()).abs()
        pytest.fail(f"{what}: {int((got != want).sum())} of {got.numel()} values differ, max |d| = {d.max().item():.3e}")


def _lists(p, name, prof, expect_th=None):
    """The device's lists of the last (sparse, profiled) frame against the rules applied to its mask, per layer in the tile geometry
    of the kernel the layer ran on (the profile's tag; expect_th(layer, ks, cout) pins it where the variant does).
    Returns [(layer, tag, count, dense tile count, list walked: True / False / None = cannot tell, the list is full)]."""
    h, w, _ = FRAMES[name]
    Hp, Wp = -(-h // 32) * 32, -(-w // 32) * 32
    want = _propagate(_cells_of(_mask(p, name)), Hp, Wp, 16)
    buf = p.tap("hg.need").numpy().astype(np.uint8).ravel()
    offs, dims = _need_plan(Hp, Wp), _layer_dims()
    tags = {layer[3:]: (kern, macs) for layer, kern, _, macs, _ in prof if layer.startswith("hg.")}
    rows = []
    for lname, ks, _, level, *_ in _layer_table():
        kern, macs = tags[lname]
        cout, cin, _ = dims[lname]
        th = 8 if kern.startswith("conv_prw8") else 16
        if expect_th is not None:
            assert th == expect_th(lname, ks, cout), (lname, kern)
            assert kern.startswith("conv_prw") == (ks == 3 and cout % 256 == 0), (lname, kern)
        k = want[lname]
        gh, gw = k.shape
        Hl, Wl = Hp >> level, Wp >> level
        ty = -(-Hl // th)
        n = int(buf[offs[lname]:offs[lname] + 4].view(np.int32)[0])
        assert 0 <= n <= ty * gw, (lname, n)
        got = buf[offs[lname] + 4:offs[lname] + 4 + 4 * n].view(np.int32).tolist()
        cells = np.flatnonzero(k).tolist()
        if th == 16:
            exp = cells
        else:
            exp = sorted(t for c in cells for t in [2 * (c // gw) * gw + c % gw] + ([(2 * (c // gw) + 1) * gw + c % gw] if 2 * (c // gw) + 1 < ty else []))
        assert sorted(got) == exp, (name, lname, kern, n, len(exp))
        dense = float(Hl) * Wl * cin * ks * ks * cout
        walked = None
        if kern.startswith("conv_prw") and n < ty * gw:
            if abs(macs - dense) <= 1e-9 * dense:
                walked = False
            else:
                assert abs(macs - dense * n / (ty * gw)) <= 1e-9 * dense, (lname, kern, macs, dense, n, ty * gw)
                walked = True
        else:
            assert abs(macs - dense) <= 1e-9 * dense, (lname, kern, macs, dense)      # no list: the dense layer's figure
        rows.append((lname, kern, n, ty * gw, walked))
    return rows


def _th_prw2(lname, ks, cout):
    return 16


def _th_prw3(lname, ks, cout):
    return 8 if ks == 3 and cout % 256 == 0 and lname != "Up_conv5" else 16


# (prw, pglds_nt_slow, force_ncu, frames).  force_ncu = 8 is the smallest grid conv_prw_launch takes (n_cu < 8 is refused); on frame A
# it gives conv3_1 runs of 136 entries (2176 8-row tiles x 256 / 256 channels over 8 workgroups), Up_conv3 9 and 18 of them
MATRIX = (
    (1, 3, 0, ("A", "A_full", "B", "W")),
    (2, 3, 0, ("A", "A_full", "B", "W")),
    (3, 3, 0, ("A", "A_full", "B", "W")),
    (2, 0, 0, ("A",)),
    (3, 1, 0, ("A",)),
    (3, 3, 8, ("A", "A_full")),
    (2, 3, 16, ("A", "W")),
    (3, 3, 0, ("B0",)),
)
CASES = [(prw, nt, ncu, f) for prw, nt, ncu, fs in MATRIX for f in fs]


class _Runs:
    """One context for the whole matrix: per frame the reference (hg_sparse = 0, prw = 0) once, per case the sparse run."""

    def __init__(self, torch, golden_dir):
        self.torch, self.p = torch, _make(golden_dir)
        self.ref, self.done = {}, {}

    def reference(self, name):
        if name not in self.ref:
            p, frame = self.p, _build(name)
            _set(p, 0, prw=0)
            out = _out(p, frame)
            mask = _mask(p, name)
            self.ref[name] = (out, _rgb48(self.torch, p, frame), mask)
        return self.ref[name]

    def run(self, case):
        if case in self.done:
            return self.done[case]
        prw, nt, ncu, name = case
        p, torch, frame = self.p, self.torch, _build(name)
        h, w = frame.shape[:2]
        self.reference(name)
        try:
            _set(p, 0, prw, nt)
            same_kernels = _out(p, frame)               # dense on the case's own kernels (default grid)
            _pollute(p, h, w)
            _set(p, 1, prw, nt, ncu)
            p.profile_enable(True)
            try:
                out = _out(p, frame)
                prof = p.profile_read()
            finally:
                p.profile_enable(False)
            rows = _lists(p, name, prof, {2: _th_prw2, 3: _th_prw3}.get(prw))
            base = p.tap("le.out")
            _set(p, 0, prw, nt)
            _pollute(p, h, w)
            _set(p, 1, prw, nt, ncu)
            rgb = _rgb48(torch, p, frame)
        finally:
            p.set_variant("force_ncu", 0)
        self.done[case] = (out, rgb, rows, same_kernels, base)
        return self.done[case]


@pytest.fixture(scope="module")
def runs(torch_cuda, golden_dir):
    r = _Runs(torch_cuda, golden_dir)
    yield r
    r.p.close()


def _id(case):
    return "prw{}-nt{}-ncu{}-{}".format(*case)


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_form_order_and_run_length_is_the_dense_output(torch_cuda, runs, case):
    """Sparse output (float tensor and RGB48 through enqueue_frame) of every variant row against the oldest dense path, bit for bit;
    the device's lists of that frame against the rules (in the geometry prw = 2 / 3 fix: 16-row everywhere / 8-row everywhere but
    Up_conv5); the profile's MACs follow the list count exactly where a list was walked and are the dense figure where not.

    Each case is also held against hg_sparse = 0 on its own kernels (asserted first), which tells a list fault from a difference
    between the kernels of prw = 0 and prw >= 1.  The four A_full cases found one: conv_pglds<ps_dot3> (Up_conv5 under prw = 0) added
    the fused 64 -> 3 dot products per lane in fp32, conv_prw<ps_dot3> per 32-channel half on the matrix pipe, and 197 of the
    1 608 000 values of the fully masked frame moved by one f16 step of conv10 (max 9.766e-4).  conv_pglds now forms the sums as
    conv_prw does."""
    torch = torch_cuda
    want, want_rgb, _ = runs.reference(case[3])
    out, rgb, rows, same_kernels, _ = runs.run(case)
    print()
    for lname, kern, n, total, walked in rows:
        print(f"  {lname:11s} {kern:20s} {n:5d} of {total:5d} tiles{'' if walked is None else (', list walked' if walked else ', list dropped: dense')}")
    assert torch.isfinite(out).all()
    _same(torch, out, same_kernels, f"{_id(case)}: sparse against dense on the same kernels")
    _same(torch, out, want, f"{_id(case)}: sparse against hg_sparse = 0, prw = 0")
    _same(torch, rgb, want_rgb, f"{_id(case)}: RGB48, sparse against hg_sparse = 0, prw = 0")


@gpu
def test_every_conv_prw_form_walked_a_partial_list(runs):
    """Over the whole matrix: each of the seven conv_prw instantiations ran at least once with a list of more than 0 and fewer than
    all of its layer's tiles, and walked it (profile MACs = count / tiles of the dense figure)."""
    seen = {}
    for case in CASES:
        for lname, kern, n, total, walked in runs.run(case)[2]:
            if walked and 0 < n < total:
                seen.setdefault(kern, (_id(case), lname, n, total))
    print()
    for form in PRW_FORMS:
        print(f"  {form:18s} {seen.get(form)}")
    missing = [f for f in PRW_FORMS if f not in seen]
    assert not missing, f"never ran with a partial list: {missing}"
    # 72 x 104: the deep layers have fewer than 8 tiles (spatial x 256-channel tiles) and the launcher drops their lists (grid < 8).
    # In frame B those layers are needed everywhere, which hides it; in B0 (no highlight, every list empty) a launch that reports
    # the dense MACs did not walk its list, one that reports none did
    dims = _layer_dims()
    rows = [r for r in runs.run((3, 3, 0, "B0"))[2] if r[1].startswith("conv_prw")]
    dropped = [r[0] for r in rows if r[4] is False]
    print(f"  B0, prw = 3: lists dropped for {dropped}")
    assert dropped and all(r[2] == 0 for r in rows)
    for lname, kern, n, total, walked in rows:
        assert walked is (total * (dims[lname][0] // 256) >= 8), (lname, kern, total, walked)


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_unmasked_pixels_are_the_le_output(torch_cuda, runs, name):
    """Independent of every HG kernel: where the mask is 0 the output is img (the f16 LE output) itself, 0 * hg + img in f32."""
    out, _, _, _, base = runs.run((1, 3, 0, name))
    mask = runs.reference(name)[2]
    got, base = out[0].cpu().numpy(), base.numpy()
    h, w, _ = FRAMES[name]
    assert got.shape == base.shape == (3, h, w)
    off = ~mask[:h, :w]
    assert off.sum() > 0.9 * h * w
    assert np.array_equal(got[:, off], base[:, off]), int((got[:, off] != base[:, off]).sum())
    assert not np.array_equal(got[:, ~off], base[:, ~off])         # and the masked pixels did get the head's output


_ORACLE = {}


@gpu
@pytest.mark.parametrize("name,prw", [("B", 1), ("B", 3), ("S", 1), ("S", 3)])
def test_sparse_output_against_the_oracle(torch_cuda, golden_dir, hg_state, name, prw):
    """Sparse frames against O.hg_generator on the device's own LE output (reflect-padded as in test_hg_golden), bar HG_OUT_MAX of
    tests/test_gpu_parity.py over all pixels and over the masked pixels alone."""
    from oracle import hdrtvnet_oracle as O
    h, w, _ = FRAMES[name]
    p = _make(golden_dir)
    try:
        _pollute(p, h, w)
        _set(p, 1, prw)
        out = _out(p, _build(name))[0].cpu().numpy()
        m = _mask(p, name)[:h, :w]
        base = p.tap("le.out").numpy()
    finally:
        p.close()
    if name not in _ORACLE or not np.array_equal(_ORACLE[name][0], base):
        mask = O.hg_mask(base)
        ph, pw = -h % 32, -w % 32
        ref = O.hg_generator(hg_state, np.pad(base, ((0, 0), (0, ph), (0, pw)), mode="reflect"),
                             np.pad(mask, ((0, 0), (0, ph), (0, pw)), mode="reflect"))[:, :h, :w]
        _ORACLE[name] = (base, mask, ref)
    _, mask, ref = _ORACLE[name]
    assert np.array_equal(mask[0] > 0, m)
    d = np.abs(out.astype(np.float64) - ref)
    print(f"\n  {name} prw = {prw}: max |out - oracle| = {d.max():.3e} over all pixels, {d[:, m].max():.3e} over the {int(m.sum())} masked pixels")
    assert d.max() <= HG_OUT_MAX and d[:, m].max() <= HG_OUT_MAX


@gpu
def test_a_run_longer_than_the_lds_list_runs_dense_and_the_profile_says_so(torch_cuda, golden_dir):
    """conv_prw_launch's fallback: 1152 x 2048 on 8 workgroups in 8-row tiles gives conv3_1 4608 tiles, a run of 577 > LIST_N = 512:
    its list is dropped, the layer runs dense and reports the dense MACs; Up_conv5 (16-row tiles, a run of 289) walks its list and
    reports count / tiles of the dense figure in the same frame."""
    torch = torch_cuda
    name = "BIG"
    h, w, _ = FRAMES[name]
    frame = _build(name)
    p = _make(golden_dir)
    try:
        _set(p, 0, prw=0)
        want = _out(p, frame)
        _mask(p, name)
        want_rgb = _rgb48(torch, p, frame)
        _pollute(p, h, w)
        try:
            _set(p, 1, 3, 3, 8)
            p.profile_enable(True)
            try:
                out = _out(p, frame)
                prof = p.profile_read()
            finally:
                p.profile_enable(False)
            rows = {r[0]: r for r in _lists(p, name, prof, _th_prw3)}
            rgb = _rgb48(torch, p, frame)          # no pollution in between: the float output above is the check of the tiles
        finally:
            p.set_variant("force_ncu", 0)
        ms = sum(e[2] for e in prof)
        print(f"\n  frame time on 8 workgroups: {ms:.1f} ms")
        for r in rows.values():
            print(f"  {r[0]:11s} {r[1]:20s} {r[2]:5d} of {r[3]:5d} tiles, walked: {r[4]}")
        assert rows["conv3_1"][1] == "conv_prw8<pool>" and rows["conv3_1"][3] == 4608 and rows["conv3_1"][2] == 4608
        macs = {layer[3:]: m for layer, _, _, m, _ in prof if layer.startswith("hg.")}
        assert macs["conv3_1"] == 576.0 * 1024 * 128 * 9 * 256                       # dense: the list was not taken
        # the deep encoder is partial in this frame: a partial list that was dropped would show as walked = False
        assert rows["conv_code2"][4] is True and rows["Up_conv1"][4] is True
        assert all(r[4] is not False for r in rows.values() if r[0] != "conv3_1"), rows
        n, total = rows["Up_conv5"][2], rows["Up_conv5"][3]
        dense5 = 576.0 * 1024 * 64 * 9 * 256
        assert rows["Up_conv5"][4] is True and 0 < n < 0.01 * total
        assert abs(macs["Up_conv5"] - dense5 * n / total) <= dense5 / total      # within one tile
        _same(torch, out, want, "1152 x 2048, prw = 3 on 8 workgroups against hg_sparse = 0, prw = 0")
        _same(torch, rgb, want_rgb, "1152 x 2048 RGB48")
        # conv3_1 is needed everywhere in that frame (as in any frame of this size with a highlight: the deepest level has 3 x 4
        # cells), so its dense MACs do not yet say that the list was dropped.  The same size once more without a highlight: every
        # list is empty, conv3_1 alone reports the dense layer's MACs, every other conv_prw layer none
        try:
            _set(p, 1, 3, 3, 8)
            p.profile_enable(True)
            try:
                _out(p, _build("BIG0"))
                prof = p.profile_read()
            finally:
                p.profile_enable(False)
            rows0 = [r for r in _lists(p, "BIG0", prof, _th_prw3) if r[1].startswith("conv_prw")]
        finally:
            p.set_variant("force_ncu", 0)
        assert len(rows0) == 13 and all(r[2] == 0 for r in rows0)
        assert [r[0] for r in rows0 if r[4] is False] == ["conv3_1"] and all(r[4] is True for r in rows0 if r[0] != "conv3_1"), rows0
    finally:
        p.close()


def _dense_refs(torch, golden_dir, names):
    """{frame: (float output, RGB48)} with hg_sparse = 0 (every other variant at its default) on a context of its own, one lane"""
    p = _make(golden_dir)
    try:
        refs = {}
        for name in names:
            _set(p, 0)
            out = _out(p, _build(name))
            _mask(p, name)
            refs[name] = (out, _rgb48(torch, p, _build(name)))
        return refs
    finally:
        p.close()


@gpu
def test_two_lanes_run_sparse_frames_side_by_side(torch_cuda, golden_dir):
    """Each lane owns an hg.need: frame A on lane 0 and A2 on lane 1 back to back on the lanes' own streams, three rounds, the frames
    swapped between the lanes every round; every RGB48 output is the single-lane dense output of its frame."""
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    refs = _dense_refs(torch, golden_dir, ("A", "A2"))
    assert not torch.equal(refs["A"][1], refs["A2"][1])
    h, w, _ = FRAMES["A"]
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0, lanes=2)
    try:
        assert p.lanes == 2
        dev = p.device
        src = {n: torch.from_numpy(_build(n)).to(dev) for n in ("A", "A2")}
        noise = torch.from_numpy(_frame("noise", h, w, 977)).to(dev)
        scratch = torch.zeros((h, w, 3), dtype=torch.uint16, device=dev)
        p.set_variant("hg_sparse", 0)
        for lane in (0, 1):                             # another image over every tile of both lanes
            p.enqueue_frame(lane, noise.data_ptr(), h, w, scratch.data_ptr())
            torch.cuda.synchronize(dev)
        p.set_variant("hg_sparse", 1)
        outs = []
        torch.cuda.synchronize(dev)
        for rnd in range(3):
            for lane in (0, 1):
                n = ("A", "A2")[(lane + rnd) % 2]
                o = torch.zeros((h, w, 3), dtype=torch.uint16, device=dev)
                p.enqueue_frame(lane, src[n].data_ptr(), h, w, o.data_ptr())
                outs.append((rnd, lane, n, o))
        torch.cuda.synchronize(dev)
        for rnd, lane, n, o in outs:
            _same(torch, o, refs[n][1], f"round {rnd}, lane {lane}, frame {n}")
    finally:
        p.close()


@gpu
def test_one_context_runs_sparse_frames_of_different_sizes_in_turn(torch_cuda, golden_dir):
    """hg.need's layout follows Hp x Wp: A reserves the context, then B, A, B, A_full, A run sparse, each against its own dense
    output from a separate context."""
    torch = torch_cuda
    refs = _dense_refs(torch, golden_dir, ("A", "B", "A_full"))
    p = _make(golden_dir)
    try:
        _set(p, 1)
        for i, name in enumerate(("A", "B", "A", "B", "A_full", "A")):
            out = _out(p, _build(name))
            _mask(p, name)
            _same(torch, out, refs[name][0], f"frame {i} ({name})")
    finally:
        p.close()


@gpu
def test_toggling_the_tile_height_between_frames(torch_cuda, golden_dir):
    """prw 3, 2, 1, 3 on one context with frame A sparse and NO other image in between: what a frame finds in the tiles it skips was
    left by a frame that cut the maps into tiles of the other height."""
    torch = torch_cuda
    p = _make(golden_dir)
    try:
        frame = _build("A")
        _set(p, 0, prw=0)
        want = _out(p, frame)
        _mask(p, "A")
        _pollute(p, *frame.shape[:2])
        for i, prw in enumerate((3, 2, 1, 3)):
            _set(p, 1, prw)
            _same(torch, _out(p, frame), want, f"step {i}, prw = {prw}")
    finally:
        p.close()
