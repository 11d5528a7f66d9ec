"""HG need lists in sub-tile units (variant hg_sparse = 2) on the device: outputs against hg_sparse = 0, lists against the numpy mirror.

Frames as in tests/test_gpu_hg_sparse_forms.py: uniform background 40 with 4x4 blocks of 255, which the head masks cell for cell
(asserted from the hg.mask tap in every case).  Sizes and placements are chosen for where a bit row of csrc/hg_need.hip can go wrong:

  A       536 x 1000 (padded 544 x 1024): ragged last cells; rows of 128 units at levels 1 - 3 (two words), 17 tile rows of 8 at level 2.
          Blocks at the four corners, across x = 512 (the word border of levels 1 - 3), in the last unit below it (x = 504: the halo
          carries up into the next word) and the first above it (x = 512: it carries down), a pair two units apart around it
          (x = 496 and 520), and in the last ragged rows.
  A0      the same size without a block: every list is empty;   A_full  all 255: every list is complete
  W       96 x 2112: the 1/32 level is 66 pixels wide, the word border (x = 2048) lies inside the deepest map; the 1/16 level has 132
          (three words), levels 1 - 3 have 264 units (five).  Blocks at the corners, across x = 2048, 1536 and below 1024.
  B       72 x 104 (96 x 128): layers with fewer than 8 tiles, where the launcher drops the list
  T       9300 x 600 (9312 x 608), once: 1164 rows x 2 words at levels 1 - 3, more than the 2304 words the kernel keeps in LDS per map, so
          those layers' own maps lie in device memory (levels 4 and 5 fit: both forms run in one frame); 5.6 M pixels, less than a
          3840 x 2160 frame.  Blocks at two corners, across x = 512, in the middle and in the last ragged rows.

Per case: hg_sparse = 0, another image over every tile (_pollute), hg_sparse = 2; the float output and RGB48 must be the dense ones bit
for bit, the device's lists (read from hg.need) the mirror's tile lists entry for entry, the profile's MACs dense x count / tiles."""
import os

import numpy as np
import pytest

from test_gpu_hg_sparse import _cells_of, _frame, _layer_table, _make, _need_plan, _pollute
from test_gpu_hg_sparse_forms import _layer_dims, _out, _rgb48, _same, _set, placed_frame
from test_hg_need_fine import UNITS_CELL, UNITS_FINE, layer_tiles

gpu = pytest.mark.gpu

FRAMES = {
    "A": (536, 1000, ((0, 0), (0, 996), (532, 0), (532, 996), (250, 510), (100, 504), (400, 512), (180, 496), (180, 520), (530, 300))),
    "A2": (536, 1000, ((60, 200), (300, 508), (470, 760))),
    "A0": (536, 1000, ()),
    "A_full": (536, 1000, None),
    "W": (96, 2112, ((0, 0), (0, 2108), (92, 0), (92, 2108), (40, 2046), (50, 1534), (70, 1020))),
    "B": (72, 104, ((0, 0), (68, 100), (34, 50))),
    "T": (9300, 600, ((0, 0), (9296, 596), (2000, 510), (4000, 300), (9290, 10))),
}


def _build(name):
    h, w, blocks = FRAMES[name]
    return np.full((h, w, 3), 255, np.uint8) if blocks is None else placed_frame(h, w, blocks)


def _padded(name):
    h, w, _ = FRAMES[name]
    return -(-h // 32) * 32, -(-w // 32) * 32


def _mask(p, name):
    """hg.mask inside H x W; its 16x16 cells are the cells the frame's blocks touch (all of them for the full frame)"""
    h, w, blocks = FRAMES[name]
    m = p.tap("hg.mask")[0].numpy() > 0
    m[h:, :] = False
    m[:, w:] = False
    want = np.zeros(_padded(name), bool)
    if blocks is None:
        assert m.sum() >= 0.99 * h * w, (name, int(m.sum()))
        want[:h, :w] = True
    for y, x in blocks or ():
        want[y:y + 4, x:x + 4] = True
    assert np.array_equal(_cells_of(m), _cells_of(want)), (name, int(m.sum()))
    return m


def _check_lists(p, name, prof, units):
    """The device's lists of the last (profiled) frame against the mirror under `units`, in each layer's own tile height; the
    profile's MACs follow count / tiles.  Returns [(layer, kernel, count, tiles)]."""
    Hp, Wp = _padded(name)
    buf = p.tap("hg.need").numpy().astype(np.uint8).ravel()
    offs, dims = _need_plan(Hp, Wp), _layer_dims()
    tags = {layer[3:]: (kern, macs) for layer, kern, _, macs, _ in prof if layer.startswith("hg.")}
    th_of = lambda lname: 8 if tags[lname][0].startswith("conv_prw8") else 16
    want = layer_tiles(_cells_of(_mask(p, name)), Hp, Wp, units, th_of)
    rows = []
    for lname, ks, _, level, *_ in _layer_table():
        kern, macs = tags[lname]
        cout, cin, _ = dims[lname]
        exp, total = want[lname]
        n = int(buf[offs[lname]:offs[lname] + 4].view(np.int32)[0])
        assert 0 <= n <= total, (name, lname, n, total)
        got = buf[offs[lname] + 4:offs[lname] + 4 + 4 * n].view(np.int32).tolist()
        assert got == exp, (name, lname, kern, n, len(exp), [t for t in got if t not in exp][:8], [t for t in exp if t not in got][:8])
        assert len(set(got)) == n, (name, lname)
        dense = float(Hp >> level) * (Wp >> level) * cin * ks * ks * cout
        if kern.startswith("conv_prw") and n < total and total * (cout // 256) >= 8:
            assert abs(macs - dense * n / total) <= 1e-9 * dense, (name, lname, kern, macs, dense, n, total)     # a list that was walked
        elif not kern.startswith("conv_prw") or n == total:
            assert abs(macs - dense) <= 1e-9 * dense, (name, lname, kern, macs, dense)
        rows.append((lname, kern, n, total))
    return rows


def _profiled(p, frame):
    p.profile_enable(True)
    try:
        out = _out(p, frame)
        return out, p.profile_read()
    finally:
        p.profile_enable(False)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
    return torch


class _Ctx:
    """One context for every case; the dense reference (hg_sparse = 0) of a frame is computed once and not touched again."""

    def __init__(self, torch, golden_dir):
        self.torch, self.p, self.ref = torch, _make(golden_dir), {}

    def reference(self, name):
        if name not in self.ref:
            frame = _build(name)
            _set(self.p, 0)
            out = _out(self.p, frame)
            _mask(self.p, name)
            self.ref[name] = (out, _rgb48(self.torch, self.p, frame))
        return self.ref[name]


@pytest.fixture(scope="module")
def ctx(torch_cuda, golden_dir):
    c = _Ctx(torch_cuda, golden_dir)
    yield c
    c.p.close()


@gpu
@pytest.mark.parametrize("prw", [1, 2, 3])
@pytest.mark.parametrize("name", ["A", "A0", "A_full", "W", "B"])
def test_sub_tile_lists_give_the_dense_output_and_are_the_mirrors_lists(torch_cuda, ctx, name, prw):
    torch, p = torch_cuda, ctx.p
    h, w, _ = FRAMES[name]
    frame = _build(name)
    want, want_rgb = ctx.reference(name)
    _set(p, 0, prw)
    _pollute(p, h, w)
    _set(p, 2, prw)
    out, prof = _profiled(p, frame)
    rows = _check_lists(p, name, prof, UNITS_FINE)
    print()
    for lname, kern, n, total in rows:
        print(f"  {lname:11s} {kern:20s} {n:5d} of {total:5d} tiles")
    assert torch.isfinite(out).all()
    _same(torch, out, want, f"{name}, prw = {prw}: hg_sparse = 2 against 0")
    if name == "A0":
        assert all(r[2] == 0 for r in rows)
    if name == "A_full":
        assert all(r[2] == r[3] for r in rows)
    if name == "A":
        # what the sub-tile units are for: the encoder no longer runs every tile of a frame with a few highlights
        assert all(r[2] < r[3] for r in rows if r[0] in ("conv3_1", "conv3_2", "conv4_1", "conv5_1")), rows
    _set(p, 0, prw)
    _pollute(p, h, w)
    _set(p, 2, prw)
    _same(torch, _rgb48(torch, p, frame), want_rgb, f"{name}, prw = {prw}: RGB48, hg_sparse = 2 against 0")


@gpu
def test_maps_too_large_for_lds(torch_cuda, ctx):
    torch, p = torch_cuda, ctx.p
    name = "T"
    h, w, _ = FRAMES[name]
    frame = _build(name)
    want, want_rgb = ctx.reference(name)
    _pollute(p, h, w)
    _set(p, 2)
    out, prof = _profiled(p, frame)
    rows = _check_lists(p, name, prof, UNITS_FINE)
    print()
    for lname, kern, n, total in rows:
        print(f"  {lname:11s} {kern:20s} {n:5d} of {total:5d} tiles")
    assert all(0 < r[2] < 0.25 * r[3] for r in rows), rows
    assert torch.isfinite(out).all()
    _same(torch, out, want, "9300 x 600: hg_sparse = 2 against 0")
    _same(torch, _rgb48(torch, p, frame), want_rgb, "9300 x 600: RGB48")


@gpu
def test_settings_1_and_2_alternate_on_one_context(torch_cuda, ctx):
    """Frames A, W, A under hg_sparse 1, 2, 1, 2, ... without another image in between: each frame's lists are its setting's own
    (the maps of both settings share their storage), and every output is the dense one."""
    torch, p = torch_cuda, ctx.p
    for name in ("A", "W"):
        ctx.reference(name)
    _set(p, 0)
    _pollute(p, 536, 1000)
    for i, (name, sparse) in enumerate((("A", 1), ("A", 2), ("W", 1), ("W", 2), ("A", 2), ("A", 1), ("A", 2))):
        _set(p, sparse)
        out, prof = _profiled(p, _build(name))
        _check_lists(p, name, prof, UNITS_CELL if sparse == 1 else UNITS_FINE)
        _same(torch, out, ctx.ref[name][0], f"step {i}: {name} under hg_sparse = {sparse}")


@gpu
def test_graph_replay_follows_each_frames_own_lists(torch_cuda, ctx, golden_dir):
    torch = torch_cuda
    refs = {n: ctx.reference(n)[0] for n in ("A", "A2", "A0")}
    assert not torch.equal(refs["A"], refs["A2"])
    p = _make(golden_dir, use_cuda_graphs=True)
    try:
        p.set_variant("hg_sparse", 2)
        for i, n in enumerate(("A2", "A", "A0", "A2", "A")):          # the first call captures, the others replay
            out, _ = p.infer(p.preprocess(_build(n)))
            _same(torch, out, refs[n], f"replay {i}, frame {n}")
        assert p._graphs, "infer did not run from a captured graph"
    finally:
        p.close()


@gpu
def test_two_lanes_with_swapped_frames(torch_cuda, ctx, golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    refs = {n: ctx.reference(n)[1] for n in ("A", "A2")}
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
        p.set_variant("hg_sparse", 2)
        outs = []
        for rnd in range(3):
            for lane in (0, 1):
                n = ("A", "A2")[(lane + rnd) % 2]
                o = torch.zeros((h, w, 3), dtype=torch.uint16, device=dev)
                p.enqueue_frame(lane, src[n].data_ptr(), h, w, o.data_ptr())
                outs.append((rnd, lane, n, o))
        torch.cuda.synchronize(dev)
        for rnd, lane, n, o in outs:
            _same(torch, o, refs[n], f"round {rnd}, lane {lane}, frame {n}")
    finally:
        p.close()
