"""HG need list of conv1 (csrc/hg_need.hip, HgNeedParams::L[0]): the rule on the CPU.

conv1 is not a row of the layer table: a pool-fused 3x3 layer at level 0 on conv_c3, whose tiles are 8 rows x 32 columns.  It writes the
pooled map p1 (level 1), conv2's input, and per pixel part2, which the per-pixel tail reads at masked pixels only.  Its K is the
existing pool-fused rule: need(p1) -- conv2's K dilated by one unit -- resampled to the level-0 map, whose unit is hg_prep's 16x16
cell.  The mirror is built from the mirrors of test_hg_need_fine.py / test_gpu_hg_sparse.py; tests/test_gpu_hg_sparse_rest.py holds
the device's counts against it."""
import numpy as np

from test_gpu_hg_sparse import _cells_of, _dilate, _down_any, _true_pixels, _up2
from test_hg_need_fine import UNITS_CELL, UNITS_FINE, _mask_of_the_rules_test, need_units, tiles_of

C1_TH, C1_TW = 8, 32            # conv_c3's tile (C3_TH x C3_TW, csrc/le_hg_misc.hip)


def conv1_need(flags, Hp, Wp, units):
    """K(conv1) in 16x16 cells of level 0.  conv2 is p1's only reader, a 3x3 layer: need(p1) = dilate(K(conv2))."""
    lg = lambda v: v.bit_length() - 1
    size0 = (-(-Hp // 16), -(-Wp // 16))
    need_p1 = _dilate(need_units(flags, Hp, Wp, units)["conv2"])
    sh = lg(units[1]) - lg(units[0]) + 1           # a K cell spans 2^-sh units of p1's map: 8 pixels of level 1
    assert units[0] == 16 and sh in (-1, 1), sh
    return _up2(need_p1, size0) if sh == 1 else _down_any(need_p1, size0)


def tiles_wh(k, unit, Hl, Wl, th, tw):
    """Sorted indices ty * ceil(Wl / tw) + tx of the th x tw tiles of an Hl x Wl map that hold a unit of k."""
    px = np.repeat(np.repeat(k, unit, 0), unit, 1)[:Hl, :Wl]
    ty, tx = -(-Hl // th), -(-Wl // tw)
    t = np.pad(px, ((0, ty * th - Hl), (0, tx * tw - Wl))).reshape(ty, th, tx, tw).any(axis=(1, 3))
    return np.flatnonzero(t).tolist()


def conv1_tiles(flags, Hp, Wp, units):
    """(sorted list of conv1's 8 x 32 tiles, tiles of the dense layer)"""
    return tiles_wh(conv1_need(flags, Hp, Wp, units), 16, Hp, Wp, C1_TH, C1_TW), -(-Hp // C1_TH) * -(-Wp // C1_TW)


def test_tiles_wh_at_width_16_is_tiles_of():
    Hp, Wp, mask = _mask_of_the_rules_test()
    k = need_units(_cells_of(mask), Hp, Wp, UNITS_FINE)["conv2"]
    for th in (8, 16):
        assert tiles_wh(k, UNITS_FINE[1], Hp >> 1, Wp >> 1, th, 16) == tiles_of(k, UNITS_FINE[1], Hp >> 1, Wp >> 1, th)


def test_conv1_tiles_cover_what_conv2_and_the_tail_read():
    Hp, Wp, mask = _mask_of_the_rules_test()
    flags = _cells_of(mask)
    true = _true_pixels(mask)
    # the pre-pool pixels of every p1 pixel conv2 reads, and part2 at the masked pixels themselves
    want = np.repeat(np.repeat(_dilate(true["conv2"]), 2, 0), 2, 1) | mask
    ty, tx = -(-Hp // C1_TH), -(-Wp // C1_TW)
    got = {}
    for units in (UNITS_FINE, UNITS_CELL):
        k = conv1_need(flags, Hp, Wp, units)
        assert k.shape == flags.shape
        assert not (flags & ~k).any(), int((flags & ~k).sum())               # K(conv1) holds every flagged cell
        tiles, total = conv1_tiles(flags, Hp, Wp, units)
        assert total == ty * tx
        t = np.zeros(ty * tx, bool)
        t[tiles] = True
        cover = np.repeat(np.repeat(t.reshape(ty, tx), C1_TH, 0), C1_TW, 1)[:Hp, :Wp]
        assert not (want & ~cover).any(), int((want & ~cover).sum())
        got[units] = set(tiles)
        print(f"  units {units[:3]}: {len(tiles)} of {total} tiles, {len(tiles_wh(want, 1, Hp, Wp, C1_TH, C1_TW))} hold a pixel that is needed")
    assert got[UNITS_FINE] <= got[UNITS_CELL]


def test_one_block_at_2176x3840_leaves_conv1_and_conv2_nearly_empty():
    Hp, Wp = 2176, 3840
    mask = np.zeros((Hp, Wp), bool)
    mask[1000:1004, 2000:2004] = True
    flags = _cells_of(mask)
    c1, n1 = conv1_tiles(flags, Hp, Wp, UNITS_FINE)
    c2 = tiles_of(need_units(flags, Hp, Wp, UNITS_FINE)["conv2"], UNITS_FINE[1], Hp >> 1, Wp >> 1, 16)
    n2 = (Hp >> 1) // 16 * ((Wp >> 1) // 16)
    print(f"  conv1 {len(c1)} of {n1}, conv2 {len(c2)} of {n2}")
    assert (n1, n2) == (32640, 8160)
    assert 0 < len(c1) < 0.05 * n1 and 0 < len(c2) < 0.05 * n2
    assert (len(c1), len(c2)) == (728, 196)          # 52 x 14 tiles of 8 x 32 and 14 x 14 of 16 x 16: the encoder's reach around one cell, no border
    # setting 1: one flagged cell reaches every cell of the deepest level within two 3x3 layers, so the encoder and with it conv1 are
    # dense even here (which is why "setting 2 inside setting 1" above says little for conv1: setting 1 is every tile)
    cell1, _ = conv1_tiles(flags, Hp, Wp, UNITS_CELL)
    assert set(c1) < set(cell1) and len(cell1) == n1, (len(c1), len(cell1), n1)
