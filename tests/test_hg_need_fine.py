"""HG need lists in sub-tile units (variant hg_sparse = 2, csrc/hg_need.hip): the rules on the CPU.

A numpy mirror of the unit rules, written from the layer table of csrc/api.h as the mirror of tests/test_gpu_hg_sparse.py is; the unit
table is copied by hand from csrc/launchers.h (hg_need_unit_log2), not parsed.  Need is a boolean array per tensor with one element per
u x u pixels of the tensor's level; a layer's list is the set of kernel tiles (16 x 16, or 8 rows x 16) that hold a unit of its K.
tests/test_gpu_hg_need_fine.py holds the device's lists against this mirror."""
import numpy as np

from test_gpu_hg_sparse import _cells_of, _dilate, _down_any, _layer_table, _propagate, _true_pixels, _up2

UNITS_FINE = (16, 4, 2, 1, 1, 1)            # hg_sparse = 2: pixels of levels 0 .. 5 per need-map unit (level 0: hg_prep's flags)
UNITS_CELL = (16, 16, 16, 16, 16, 16)       # hg_sparse = 1


def need_units(flags, Hp, Wp, units):
    """{layer: K}, K in units of the layer's level.  flags: the 16x16 full-resolution cells that hold a masked pixel."""
    size = lambda lev: (-(-(Hp >> lev) // units[lev]), -(-(Wp >> lev) // units[lev]))
    lg = lambda v: v.bit_length() - 1
    assert flags.shape == size(0) and units[0] == 16
    need = {"part": flags}
    K = {}
    for name, ks, mode, level, tin, skip, out in reversed(_layer_table()):
        olev = level + (mode == 1) - (mode == 2)
        o = need[out]
        assert o.shape == size(olev), (name, o.shape)
        # a K unit spans 2^-sh out units: the same pixels seen from the output's level (one level down / up: half / twice as many)
        sh = lg(units[olev]) - lg(units[level]) + olev - level
        assert sh in (-1, 0, 1), (name, sh)
        k = o if sh == 0 else (_up2(o, size(level)) if sh == 1 else _down_any(o, size(level)))
        assert k.shape == size(level), (name, k.shape, size(level))
        K[name] = k
        reads = _dilate(k) if ks == 3 else k        # the halo of a 3x3 layer is one pixel: one unit or less
        for t in (tin, skip):
            if t is not None:
                need[t] = need.get(t, np.zeros(size(level), bool)) | reads
    return K


def tiles_of(k, unit, Hl, Wl, th):
    """Sorted indices ty * ceil(Wl / 16) + tx of the th x 16 tiles of an Hl x Wl map that hold a unit of k."""
    px = np.repeat(np.repeat(k, unit, 0), unit, 1)[:Hl, :Wl]
    ty, tx = -(-Hl // th), -(-Wl // 16)
    t = np.pad(px, ((0, ty * th - Hl), (0, tx * 16 - Wl))).reshape(ty, th, tx, 16).any(axis=(1, 3))
    return np.flatnonzero(t).tolist()


def layer_tiles(flags, Hp, Wp, units, th_of):
    """{layer: (sorted tile list, tiles of the dense layer)}; th_of(layer) -> 8 or 16."""
    K = need_units(flags, Hp, Wp, units)
    out = {}
    for name, _, _, level, *_ in _layer_table():
        th, Hl, Wl = th_of(name), Hp >> level, Wp >> level
        out[name] = (tiles_of(K[name], units[level], Hl, Wl, th), -(-Hl // th) * -(-Wl // 16))
    return out


def _mask_of_the_rules_test():
    Hp, Wp = 1056, 1568                 # the mask of test_need_rules_cover_the_true_dependency_set
    rng = np.random.default_rng(7)
    mask = np.zeros((Hp, Wp), bool)
    mask[rng.integers(0, Hp, 12), rng.integers(0, Wp, 12)] = True
    mask[400:420, 900:1000] = True
    mask[Hp - 1, Wp - 1] = mask[0, 0] = True
    return Hp, Wp, mask


def test_unit_rules_cover_the_true_set_and_stay_inside_the_cell_rules():
    Hp, Wp, mask = _mask_of_the_rules_test()
    flags = _cells_of(mask)
    fine, cells, true = need_units(flags, Hp, Wp, UNITS_FINE), _propagate(flags, Hp, Wp, 16), _true_pixels(mask)
    assert set(fine) == set(cells) == set(true)
    print()
    for name, _, _, level, *_ in _layer_table():
        u, t = UNITS_FINE[level], true[name]
        Hl, Wl = Hp >> level, Wp >> level
        cover = np.repeat(np.repeat(fine[name], u, 0), u, 1)[:Hl, :Wl]
        assert not (t & ~cover).any(), (name, int((t & ~cover).sum()))
        for th in (16, 8):
            got = set(tiles_of(fine[name], u, Hl, Wl, th))
            allowed = set(tiles_of(cells[name], 16, Hl, Wl, th))          # th = 8: both tiles of a cell
            assert got <= allowed, (name, th, len(got - allowed))
            assert set(tiles_of(t, 1, Hl, Wl, th)) <= got
        n16, c16 = len(tiles_of(fine[name], u, Hl, Wl, 16)), int(cells[name].sum())
        print(f"  {name:11s} level {level}: {n16:5d} 16-row tiles under the unit rules, {c16:5d} under the cell rules, "
              f"{len(tiles_of(t, 1, Hl, Wl, 16)):5d} hold a pixel that is needed")


def test_unit_16_everywhere_is_the_cell_rule():
    Hp, Wp, mask = _mask_of_the_rules_test()
    flags = _cells_of(mask)
    mirror, cells = need_units(flags, Hp, Wp, UNITS_CELL), _propagate(flags, Hp, Wp, 16)
    for name, _, _, level, *_ in _layer_table():
        assert np.array_equal(mirror[name], cells[name]), name
        gw = cells[name].shape[1]
        Hl, Wl = Hp >> level, Wp >> level
        c = np.flatnonzero(cells[name]).tolist()
        assert tiles_of(mirror[name], 16, Hl, Wl, 16) == c
        ty8 = -(-Hl // 8)             # the 8-row lists of the cell rule: both tiles of a cell, the second where the map has that row
        both = sorted(t for i in c for t in [2 * (i // gw) * gw + i % gw] + ([(2 * (i // gw) + 1) * gw + i % gw] if 2 * (i // gw) + 1 < ty8 else []))
        assert tiles_of(mirror[name], 16, Hl, Wl, 8) == both, name


def test_one_block_at_2176x3840_leaves_the_encoder_nearly_empty():
    Hp, Wp = 2176, 3840
    mask = np.zeros((Hp, Wp), bool)
    mask[1000:1004, 2000:2004] = True
    flags = _cells_of(mask)
    print()
    for th in (16, 8):
        fine = layer_tiles(flags, Hp, Wp, UNITS_FINE, lambda n: th)
        cell = layer_tiles(flags, Hp, Wp, UNITS_CELL, lambda n: th)
        for name in ("conv3_1", "conv4_1", "conv5_1"):
            (t, total), (tc, _) = fine[name], cell[name]
            print(f"  {name}, {th}-row tiles: {len(t)} of {total} = {100.0 * len(t) / total:.2f} % (cell rule: {100.0 * len(tc) / total:.1f} %)")
            assert 0 < len(t) < 0.05 * total, (name, th, len(t), total)
        assert all(len(fine[n][0]) <= len(cell[n][0]) for n in fine)
