"""HG need lists on the rest of the head: conv1 (conv_c3<64,dot3>), conv2 (conv_pglds) and the 1x1 fuse convs conv6 .. conv9 (conv_glds1).

Frames as in tests/test_gpu_hg_need_fine.py: uniform background 40 with 4x4 blocks of 255; the mask is asserted from the hg.mask tap
in every case, so a failed precondition fails the test.  Per case: hg_sparse = 0 (the reference, once per frame), another image over
every tile (_pollute), then the sparse setting; the float output and RGB48 must be the dense ones bit for bit, profile_tiles() of the
six layers must be (the mirror's count, the dense tile count) -- tests/test_hg_need_conv1.py and tests/test_hg_need_fine.py hold the
mirror -- and hdrtv_profile_get's MACs of the six stay the dense layer's.  On the single-block frames every one of the six runs some
but not all of its tiles (a silently dense run cannot pass), conv1 and conv2 at most 20 %.

force_ncu = 8 at 536 x 1000: the longest run of the six layers is conv1's, 2176 tiles over 8 workgroups per resident block = 91 .. 272
entries, which fits the 512-entry LDS block of every kernel here; the lists are walked there (total > 0).  The launchers drop a list
whose run could exceed that block, from 4089 tiles per eight workgroups on: the case for it is 1152 x 3712 with prw = 0 on eight
workgroups, where conv1 (16704 tiles, runs of 696 on three resident blocks per workgroup slot), conv2 and conv9 (4176 tiles: 523),
conv3_1 and Up_conv5 (8352: 1045), conv4_1 and Up_conv4 (4176: 523) run dense and report total = 0, and the other eleven layers walk
partial lists in the same frame.  That reaches the drop of conv_c3_launch, conv_pglds_launch and conv_glds1_launch."""
import os

import numpy as np
import pytest

from test_gpu_hg_sparse import _cells_of, _frame, _layer_table, _make, _pollute
from test_gpu_hg_sparse_forms import _layer_dims, _out, _rgb48, _same, _set, placed_frame
from test_hg_need_conv1 import conv1_tiles
from test_hg_need_fine import UNITS_CELL, UNITS_FINE, layer_tiles

gpu = pytest.mark.gpu

SIX = ("conv1", "conv2", "conv6", "conv7", "conv8", "conv9")
FRAMES = {
    "none": (536, 1000, ()),
    "first": (536, 1000, ((0, 0),)),
    "last": (536, 1000, ((532, 996),)),
    "straddle": (536, 1000, ((6, 254),)),          # rows 6-9, columns 254-257: conv1's 8-row and 32-column tile borders, a 16x16 cell border
    "full": (536, 1000, None),
    "two": (536, 1000, ((300, 508), (60, 200))),
    "wide": (96, 2112, ((40, 1000),)),
    "small": (72, 104, ((34, 50),)),               # conv6 and conv7 have one tile: grids smaller than 8
    "small0": (72, 104, ()),
    "big": (1152, 3712, ((600, 1800),)),
}
# 1152 x 3712, prw = 0, force_ncu = 8: the layers whose run does not fit the kernels' 512-entry LDS block
BIG_DROPPED = {"conv1", "conv2", "conv3_1", "conv4_1", "Up_conv4", "conv9", "Up_conv5"}
LIST_N = 512
SINGLE = ("first", "last", "straddle")
TAP_FRAME, TAPS = "two", ("hg.p1", "hg.conv2", "hg.conv6", "hg.conv9")


def _build(name):
    h, w, blocks = FRAMES[name]
    return np.full((h, w, 3), 255, np.uint8) if blocks is None else placed_frame(h, w, blocks)


def _padded(name):
    h, w, _ = FRAMES[name]
    return -(-h // 32) * 32, -(-w // 32) * 32


def _mask(p, name):
    """hg.mask inside H x W; its 16x16 cells must be the cells the frame's blocks touch (all of them for the full frame)"""
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


def _mirror(flags, Hp, Wp, units):
    """{layer: (tiles to run, tiles of the dense layer)} of the six layers, the table's in 16-row tiles"""
    want = layer_tiles(flags, Hp, Wp, units, lambda n: 16)
    out = {n: (len(want[n][0]), want[n][1]) for n in SIX[1:]}
    c1, n1 = conv1_tiles(flags, Hp, Wp, units)
    out["conv1"] = (len(c1), n1)
    return out


def _dense_macs(Hp, Wp):
    dims = _layer_dims()
    macs = {"conv1": float(Hp) * Wp * (27 * 64 + 192)}
    for lname, ks, _, level, *_ in _layer_table():
        cout, cin, _ = dims[lname]
        macs[lname] = float(Hp >> level) * (Wp >> level) * cin * ks * ks * cout
    return macs


def _profiled(p, frame):
    """(output, {layer: (kernel, executed, total)}, {layer: MACs}) of one profiled frame, HG launches only"""
    p.profile_enable(True)
    try:
        out = _out(p, frame)
        tiles = {layer[3:]: (kern, done, total) for layer, kern, done, total in p.profile_tiles() if layer.startswith("hg.")}
        macs = {layer[3:]: m for layer, _, _, m, _ in p.profile_read() if layer.startswith("hg.")}
        return out, tiles, macs
    finally:
        p.profile_enable(False)


def _check_six(p, name, tiles, macs, units):
    """profile_tiles() of the six layers against the mirror on the frame's own mask; the profile's MACs are the dense layer's."""
    Hp, Wp = _padded(name)
    want = _mirror(_cells_of(_mask(p, name)), Hp, Wp, units)
    dense = _dense_macs(Hp, Wp)
    print()
    for n in SIX:
        kern, done, total = tiles[n]
        print(f"  {n:6s} {kern:20s} {done:5d} of {total:5d} tiles (mirror {want[n][0]} of {want[n][1]})")
        assert not kern.startswith("conv_prw"), (n, kern)
        assert (done, total) == want[n], (name, n, kern, done, total, want[n])
        assert abs(macs[n] - dense[n]) <= 1e-9 * dense[n], (name, n, kern, macs[n], dense[n])
    return want


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
    return torch


class _Ctx:
    """One context for every case; the dense reference (hg_sparse = 0) of a frame is computed once and not touched again."""

    def __init__(self, torch, golden_dir):
        self.torch, self.p, self.ref, self.taps = torch, _make(golden_dir), {}, {}

    def reference(self, name):
        if name not in self.ref:
            frame = _build(name)
            _set(self.p, 0)
            out = _out(self.p, frame)
            _mask(self.p, name)
            if name == TAP_FRAME:
                self.taps = {t: self.p.tap(t) for t in TAPS}
            self.ref[name] = (out, _rgb48(self.torch, self.p, frame))
        return self.ref[name]


@pytest.fixture(scope="module")
def ctx(torch_cuda, golden_dir):
    c = _Ctx(torch_cuda, golden_dir)
    yield c
    c.p.close()


def _case(torch, ctx, name, sparse=2, prw=1, ncu=0):
    p = ctx.p
    h, w, _ = FRAMES[name]
    frame = _build(name)
    want, want_rgb = ctx.reference(name)
    _set(p, 0, prw, ncu=ncu)
    _pollute(p, h, w)
    _set(p, sparse, prw, ncu=ncu)
    try:
        out, tiles, macs = _profiled(p, frame)
        rows = _check_six(p, name, tiles, macs, UNITS_CELL if sparse == 1 else UNITS_FINE)
        assert torch.isfinite(out).all()
        _same(torch, out, want, f"{name}: hg_sparse = {sparse}, prw = {prw}, force_ncu = {ncu} against hg_sparse = 0")
        _set(p, 0, prw, ncu=ncu)
        _pollute(p, h, w)
        _set(p, sparse, prw, ncu=ncu)
        _same(torch, _rgb48(torch, p, frame), want_rgb, f"{name}: RGB48, hg_sparse = {sparse}, prw = {prw}, force_ncu = {ncu}")
    finally:
        _set(p, 2)
    return rows, tiles


@gpu
@pytest.mark.parametrize("name", ["none", "first", "last", "straddle", "full", "wide", "small", "small0"])
def test_the_six_layers_walk_their_lists_and_the_output_is_the_dense_one(torch_cuda, ctx, name):
    rows, _ = _case(torch_cuda, ctx, name)
    if name in ("none", "small0"):
        assert all(rows[n][0] == 0 for n in SIX), rows
    if name == "full":
        assert all(rows[n][0] == rows[n][1] for n in SIX), rows
    if name in SINGLE:
        assert all(0 < rows[n][0] < rows[n][1] for n in SIX), rows
        assert all(rows[n][0] <= 0.2 * rows[n][1] for n in ("conv1", "conv2")), rows
        assert all(1 <= rows[n][0] <= 2 for n in SIX[2:]), rows
        assert [rows[n][1] for n in SIX] == [2176, 544, 12, 40, 144, 544], rows
    if name == "wide":
        assert all(0 < rows[n][0] < rows[n][1] for n in SIX), rows
    if name == "small":
        assert rows["conv6"] == (1, 1) and rows["conv7"] == (1, 1), rows


@gpu
def test_cell_units(torch_cuda, ctx):
    _case(torch_cuda, ctx, "straddle", sparse=1)


@gpu
def test_every_3x3_layer_on_conv_pglds_walks_its_list(torch_cuda, ctx):
    """prw = 0: conv_pglds runs every 3x3 layer of the table with the 16-row lists, Cout-tile slowest on the Up convs"""
    _, tiles = _case(torch_cuda, ctx, "straddle", prw=0)
    Hp, Wp = _padded("straddle")
    want = layer_tiles(_cells_of(_mask(ctx.p, "straddle")), Hp, Wp, UNITS_FINE, lambda n: 16)      # (the last frame was this one)
    for lname, ks, *_ in _layer_table():
        kern, done, total = tiles[lname]
        assert kern.startswith("conv_pglds" if ks == 3 else "conv_glds1"), (lname, kern)
        assert (done, total) == (len(want[lname][0]), want[lname][1]), (lname, kern, done, total)
        assert 0 < done < total, (lname, done, total)


@gpu
def test_eight_workgroups(torch_cuda, ctx):
    rows, _ = _case(torch_cuda, ctx, "straddle", ncu=8)
    assert all(0 < rows[n][0] < rows[n][1] for n in SIX), rows


@gpu
def test_lists_too_long_for_the_lds_block_are_dropped_and_the_layer_runs_dense(torch_cuda, ctx):
    """conv_c3_launch, conv_pglds_launch and conv_glds1_launch on eight workgroups: a launch whose dense run exceeds LIST_N entries runs
    every tile and reports total = 0; the launches with shorter runs walk partial lists in the same frame.  Which is which follows
    from the launchers' rule (dense tiles x Cout-tiles / 8 + 1 entries on a grid of eight), mirrored here and pinned by name."""
    torch, p = torch_cuda, ctx.p
    name = "big"
    h, w, _ = FRAMES[name]
    Hp, Wp = _padded(name)
    frame = _build(name)
    want, want_rgb = ctx.reference(name)
    _set(p, 0)
    _pollute(p, h, w)
    _set(p, 2, 0, ncu=8)
    try:
        out, tiles, macs = _profiled(p, frame)
        flags = _cells_of(_mask(p, name))
        mirror = {n: (len(t), total) for n, (t, total) in layer_tiles(flags, Hp, Wp, UNITS_FINE, lambda n: 16).items()}
        c1, n1 = conv1_tiles(flags, Hp, Wp, UNITS_FINE)
        mirror["conv1"] = (len(c1), n1)
        dims, dense = _layer_dims(), _dense_macs(Hp, Wp)
        dropped = {"conv1"} if -(-n1 // (4 * 8)) > LIST_N else set()         # conv_c3: at most four resident blocks per CU
        for lname, *_ in _layer_table():
            if mirror[lname][1] * (max(dims[lname][0], 128) // 128) // 8 + 1 > LIST_N:
                dropped.add(lname)
        assert dropped == BIG_DROPPED, sorted(dropped)
        print()
        for n in ["conv1"] + [r[0] for r in _layer_table()]:
            kern, done, total = tiles[n]
            print(f"  {n:11s} {kern:20s} {done:5d} of {total:5d} tiles (mirror {mirror[n][0]} of {mirror[n][1]})")
            assert not kern.startswith("conv_prw"), (n, kern)
            if n in dropped:
                assert (done, total) == (0, 0), (n, kern, done, total)
            else:
                assert (done, total) == mirror[n] and 0 < done < total, (n, kern, done, total, mirror[n])
            assert abs(macs[n] - dense[n]) <= 1e-9 * dense[n], (n, kern, macs[n], dense[n])
        assert torch.isfinite(out).all()
        _same(torch, out, want, "1152 x 3712, prw = 0 on 8 workgroups: hg_sparse = 2 against 0")
        _set(p, 0)
        _pollute(p, h, w)
        _set(p, 2, 0, ncu=8)
        _same(torch, _rgb48(torch, p, frame), want_rgb, "1152 x 3712, prw = 0 on 8 workgroups: RGB48")
    finally:
        _set(p, 2)


@gpu
def test_taps_after_a_sparse_frame_are_the_dense_tensors(torch_cuda, ctx):
    torch, p = torch_cuda, ctx.p
    h, w, _ = FRAMES[TAP_FRAME]
    frame = _build(TAP_FRAME)
    want, _ = ctx.reference(TAP_FRAME)
    _set(p, 0)
    _pollute(p, h, w)
    _set(p, 2)
    out = _out(p, frame)
    _same(torch, out, want, "two blocks: hg_sparse = 2 against 0")
    for n in TAPS:
        _same(torch, p.tap(n), ctx.taps[n], f"tap {n} after a sparse frame")
    _same(torch, _out(p, frame), want, "the frame behind the completed taps")


@gpu
def test_graph_replay_follows_each_frames_own_lists(torch_cuda, ctx, golden_dir):
    torch = torch_cuda
    refs = {n: ctx.reference(n)[0] for n in ("straddle", "two", "none")}
    assert not torch.equal(refs["straddle"], refs["two"])
    p = _make(golden_dir, use_cuda_graphs=True)
    try:
        p.set_variant("hg_sparse", 2)
        for i, n in enumerate(("two", "straddle", "none", "two", "straddle")):          # the first call captures, the others replay
            out, _ = p.infer(p.preprocess(_build(n)))
            _same(torch, out, refs[n], f"replay {i}, frame {n}")
        assert p._graphs, "infer did not run from a captured graph"
    finally:
        p.close()


@gpu
def test_two_lanes_with_swapped_frames(torch_cuda, ctx, golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    refs = {n: ctx.reference(n)[1] for n in ("straddle", "two")}
    h, w, _ = FRAMES["two"]
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0, lanes=2)
    try:
        assert p.lanes == 2
        dev = p.device
        src = {n: torch.from_numpy(_build(n)).to(dev) for n in ("straddle", "two")}
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
                n = ("straddle", "two")[(lane + rnd) % 2]
                o = torch.zeros((h, w, 3), dtype=torch.uint16, device=dev)
                p.enqueue_frame(lane, src[n].data_ptr(), h, w, o.data_ptr())
                outs.append((rnd, lane, n, o))
        torch.cuda.synchronize(dev)
        for rnd, lane, n, o in outs:
            _same(torch, o, refs[n], f"round {rnd}, lane {lane}, frame {n}")
    finally:
        p.close()
