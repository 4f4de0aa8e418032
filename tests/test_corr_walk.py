"""What tests/test_gpu_correlation.py's cases reach, proved on the host (no GPU): the float64 reference and its
bound against the project's sequential float32 oracle, and -- on a restatement of correlation_sp_kernel's tile walk
(_corr_cases.walk) -- that the case table makes persistent workgroups take second and later tiles in every way the
kernel tells apart.  The older parity cases have at most 90 tiles on a grid of 512 workgroups: every workgroup
leaves after its first tile, and none of the copies issued for a next tile is ever read."""
import numpy as np
import pytest

import _corr_cases as cc
from oracle import tfops

ORACLE_SHAPES = [cc.Case(40, 56, 5, 2, 5, ()), cc.Case(72, 88, 5, 2, 5, ()), cc.Case(25, 40, 4, 2, 5, ()),
                 cc.Case(18, 33, 5, 2, 3, ()), cc.Case(21, 35, 3, 2, 1, ()), cc.Case(40, 37, 6, 3, 6, ())]


# ---- the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', ORACLE_SHAPES, ids=cc.case_id)
def test_reference_equals_the_oracle_on_integer_maps(c):
    a, b = cc.pair(c, 'int')
    ref, mag = cc.reference(a, b, c.md, c.s2, c.pad)
    want = tfops.correlation(a, b, c.md, c.s2, c.pad)
    assert ref.shape == want.shape == cc.out_shape(c.H, c.W, c.md, c.s2, c.pad)
    assert np.array_equal(ref, want.astype(np.float64))
    assert np.abs(ref).max() > 1 and (mag >= np.abs(ref)).all()


@pytest.mark.parametrize('c', ORACLE_SHAPES, ids=cc.case_id)
def test_oracle_lies_within_the_bound_on_normal_maps(c):
    a, b = cc.pair(c, 'normal')
    ref, mag = cc.reference(a, b, c.md, c.s2, c.pad)
    want = tfops.correlation(a, b, c.md, c.s2, c.pad)
    ratio = cc.worst_ratio(want, ref, mag)
    print('oracle %s: %.3f of the bound' % (cc.case_id(c), ratio))
    assert (np.abs(want - ref) <= cc.bound(mag)).all()
    # the bound leaves a correct kernel room, and not much more: a sequential float32 sum uses a fifth of it
    assert 0.01 < ratio < 0.5


def test_bound_is_gamma_33_rounded_up():
    u = 2.0 ** -24
    assert 33 * u / (1 - 33 * u) < 34 * u
    assert cc.bound(np.zeros(1))[0] == 1e-30 and cc.bound(np.ones(1))[0] == 34 * u + 1e-30


@pytest.mark.parametrize('c,rows', [(cc.Case(72, 88, 5, 2, 5, ()), (0, 16)), (cc.Case(72, 88, 5, 2, 5, ()), (30, 47)),
                                    (cc.Case(72, 88, 5, 2, 5, ()), (60, 72)), (cc.Case(70, 90, 4, 2, 5, ()), (0, 3)),
                                    (cc.Case(70, 90, 4, 2, 5, ()), (65, 72)), (cc.Case(76, 95, 5, 2, 3, ()), (0, 9)),
                                    (cc.Case(76, 95, 5, 2, 3, ()), (70, 72)), (cc.Case(40, 37, 6, 3, 6, ()), (11, 12))])
def test_a_row_band_of_the_reference_equals_those_rows_of_the_whole(c, rows):
    a, b = cc.pair(c, 'normal')
    ref, mag = cc.reference(a, b, c.md, c.s2, c.pad)
    band, band_mag = cc.reference(a, b, c.md, c.s2, c.pad, rows=rows)
    assert band.shape[0] == rows[1] - rows[0]
    assert np.array_equal(band, ref[rows[0]:rows[1]]) and np.array_equal(band_mag, mag[rows[0]:rows[1]])


def test_integer_maps_are_exact_in_float32():
    """Products are at most 16, sums of 32 at most 512: integers far below 2^24, and 1/32 is a power of two."""
    a, b = cc.pair(cc.BASE, 'int')
    assert np.array_equal(a, np.round(a)) and np.abs(a).max() == 4 and np.abs(b).max() == 4
    assert 32 * 16 < 2 ** 24


# ---- the walk ------------------------------------------------------------------------------------------------------
def _walks(c, mode):
    """[[(ty, tx), ...] per workgroup] of a case under a mode, and its grid."""
    ty, tx = cc.tiles_of(c)
    order = cc.curve(ty, tx)
    grid = cc.grid_of(len(order), cc.mode_grid(mode))
    w = cc.walk(len(order), grid)
    return [[order[s] for s in w[b]] for b in range(grid)], grid


# (the two-pass kernel has no walk: one tile per block, test_two_pass_kernel_covers_every_tile_exactly_once)
EVERY = [(c, m) for c in cc.SP_CASES for m in c.modes if m != 'two_pass']


@pytest.mark.parametrize('c,mode', EVERY, ids=['%s-%s' % (cc.case_id(c), m) for c, m in EVERY])
def test_walk_covers_every_tile_exactly_once(c, mode):
    walks, grid = _walks(c, mode)
    ty, tx = cc.tiles_of(c)
    assert grid % 8 == 0 and 8 <= grid <= cc.mode_grid(mode)
    assert sorted(t for w in walks for t in w) == sorted((y, x) for y in range(ty) for x in range(tx))


@pytest.mark.parametrize('c', cc.WALK, ids=cc.case_id)
def test_two_pass_kernel_covers_every_tile_exactly_once(c):
    OH, OW, _ = cc.out_shape(c.H, c.W, c.md, c.s2, c.pad)
    n = -(-OW // 16) * -(-OH // 32)
    tiles = [t for t in cc.two_pass_tiles(n).values() if t < n]
    assert sorted(tiles) == list(range(n))


def test_curve_is_a_permutation_in_blocks_of_8_by_8():
    order = cc.curve(10, 13)
    assert sorted(order) == [(y, x) for y in range(10) for x in range(13)]
    assert order[:9] == [(0, x) for x in range(8)] + [(1, 0)] and order[64] == (0, 8) and order[104] == (8, 0)


def test_case_shapes_are_what_their_comments_say():
    shapes = {cc.case_id(c): (cc.out_shape(c.H, c.W, c.md, c.s2, c.pad)[:2], cc.tiles_of(c)) for c in cc.CASES}
    assert shapes['72x88-md5-s2-pad5'] == ((72, 88), (5, 6))
    assert shapes['150x200-md5-s2-pad5'] == ((150, 200), (10, 13))
    assert shapes['70x90-md4-s2-pad5'] == ((72, 92), (5, 6))          # larger than the input, shift -1
    assert shapes['76x95-md5-s2-pad3'] == ((72, 91), (5, 6))          # smaller, shift +2
    assert shapes['40x56-md5-s2-pad5'] == ((40, 56), (3, 4))
    assert shapes['18x33-md5-s2-pad3'] == ((14, 29), (1, 2))
    assert shapes['368x368-md5-s2-pad5'] == ((368, 368), (23, 23))
    # the 5 x 5 grid of displacements two apart is what the one-pass kernel takes; the generic cases are not it
    assert all(c.s2 == 2 and c.md // c.s2 == 2 for c in cc.SP_CASES)
    assert not any(c.s2 == 2 and c.md // c.s2 == 2 for c in cc.GENERIC)
    assert [cc.out_shape(c.H, c.W, c.md, c.s2, c.pad)[2] for c in cc.GENERIC] == [1, 9, 9, 25, 25]


def _case(name):
    return [c for c in cc.CASES if cc.case_id(c) == name][0]


def test_walk_lengths_under_the_short_grids():
    def lengths(name, mode):
        return sorted(set(len(w) for w in _walks(_case(name), mode)[0]))
    assert lengths('72x88-md5-s2-pad5', 'grid8') == [2, 4]
    assert lengths('150x200-md5-s2-pad5', 'grid8') == [11, 17]
    assert lengths('150x200-md5-s2-pad5', 'grid24') == [3, 4, 5, 6]
    assert lengths('40x56-md5-s2-pad5', 'grid8') == [0, 2]
    assert lengths('18x33-md5-s2-pad3', 'grid8') == [0, 1]
    # the older parity cases' largest map, (130,150): one tile per workgroup on the device's own grid
    n = 9 * 10
    assert set(len(w) for w in cc.walk(n, cc.grid_of(n)).values()) <= {0, 1}


def _all_walks():
    return [(c, m, w, g) for c, m in EVERY for w, g in [_walks(c, m)]]


def test_table_reaches_a_workgroup_with_three_or_more_tiles():
    """The second trip through the loop is the first whose neighbourhood came by the Early and Late copies; the third
    is the first that starts from a hand-over (ah = an) which itself followed a hand-over."""
    for mode in ('grid8', 'grid16', 'grid24', 'halves2_grid8'):
        assert any(len(w) >= 3 for c, m, ws, _ in _all_walks() if m == mode for w in ws), mode


def test_table_reaches_a_one_tile_workgroup_beside_a_two_tile_one():
    """Workgroups of one XCD that leave the loop at different trips: the one that leaves must not be waited for, and
    must not have issued copies for a tile it does not have."""
    hit = [(cc.case_id(c), m) for c, m, ws, g in _all_walks()
           for x in range(8) if {1, 2} <= set(len(ws[b]) for b in range(x, g, 8))]
    assert hit


def test_table_reaches_an_xcd_without_tiles():
    """first >= last: every workgroup of that XCD returns before its first barrier."""
    hit = [(cc.case_id(c), m) for c, m, ws, g in _all_walks()
           if any(not any(ws[b] for b in range(x, g, 8)) for x in range(8)) and any(ws)]
    assert ('40x56-md5-s2-pad5', 'grid8') in hit and ('18x33-md5-s2-pad3', 'default') in hit


def test_table_reaches_ragged_tiles_that_are_not_a_workgroups_first():
    """The row and column guards of the stores, and the descriptor's zeros, on a tile whose neighbourhood arrived by
    the Early and Late copies."""
    for mode in ('grid8', 'halves2_grid8'):
        rows = cols = 0
        for c, m, ws, _ in _all_walks():
            if m != mode:
                continue
            OH, OW, _k = cc.out_shape(c.H, c.W, c.md, c.s2, c.pad)
            for w in ws:
                rows += sum(1 for ty, tx in w[1:] if ty * 16 + 16 > OH)
                cols += sum(1 for ty, tx in w[1:] if tx * 16 + 16 > OW)
        assert rows > 0 and cols > 0, mode


def test_table_reaches_a_walk_from_quad_stores_to_scalar_stores_and_back():
    """(70,90) md4 pad5: OW * 25 is a multiple of 4 and the last tile column is ragged, so one workgroup's loop takes
    the 16-byte store path, then the scalar one, then the 16-byte one again; (76,95) pad3 is scalar throughout."""
    c = _case('70x90-md4-s2-pad5')
    paths = [[cc.tile_store_path(c, t) for t in w] for w in _walks(c, 'grid8')[0]]
    assert any(''.join(p[0] for p in w).find('vsv') >= 0 for w in paths)
    c = _case('76x95-md5-s2-pad3')
    assert {cc.tile_store_path(c, t) for w in _walks(c, 'grid8')[0] for t in w} == {'scalar'}


def test_table_reaches_a_walk_across_a_super_block_boundary():
    """Consecutive tiles of one workgroup that are far apart on the map: the next tile's coordinates come from the
    list, not from the current tile's."""
    c = _case('150x200-md5-s2-pad5')
    for mode in ('grid8', 'grid24'):
        ws, _ = _walks(c, mode)
        block = lambda t: (t[0] // 8, t[1] // 8)        # noqa: E731
        assert any(block(p) != block(q) for w in ws for p, q in zip(w, w[1:])), mode


def test_default_grid_gives_some_workgroups_a_second_tile():
    """529 tiles on the device's own 512 workgroups: the multi-tile loop as every frame pair runs it."""
    ws, grid = _walks(cc.DEFAULT_GRID_CASE, 'default')
    assert grid == 512
    lens = [len(w) for w in ws]
    # (per = 67: three workgroups of an XCD take a second tile; the last XCD has 60 tiles for its 64 workgroups)
    assert set(lens) == {0, 1, 2} and lens.count(2) == 21 and lens.count(0) == 4
    # and the full-size map: 2200 tiles, four or five per workgroup
    n = 44 * 50
    assert set(len(w) for w in cc.walk(n, cc.grid_of(n)).values()) == {4, 5}


def test_listed_tiles_case_walks_two_tiles_per_workgroup():
    tiles, lst = cc.listed_tiles()
    assert len(set(tiles)) == cc.LISTED['n_list'] == 17 and len(lst) == 30
    w = cc.walk(13, cc.grid_of(13, 8))
    assert sorted(len(v) for v in w.values()) == [0, 1, 2, 2, 2, 2, 2, 2]
    assert sorted(s for v in w.values() for s in v) == list(range(13))


# ---- the tile-list inputs --------------------------------------------------------------------------------------------
def test_list_boxes_show_a_dropped_or_shortened_chunk():
    """Three chunks of 256, the last one partial: each contributes tiles no other does, and so does the last box."""
    oh, ow = cc.LIST_HW
    boxes = cc.list_boxes()
    assert len(boxes) == 700
    every = cc.expected_tiles(boxes, oh, ow)
    assert 0 < len(every) < 130
    for lo, hi in ((0, 256), (256, 512), (512, 700), (699, 700)):
        rest = np.concatenate([boxes[:lo], boxes[hi:]])
        assert cc.expected_tiles(rest, oh, ow) < every, (lo, hi)
    flat = boxes.reshape(-1)
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any()
    assert (flat == np.float32(1e30)).any() and (flat == np.float32(-1e30)).any()
    assert (boxes[:, 0] > boxes[:, 2]).any() and (boxes[:, 0] == boxes[:, 2]).any() and (boxes[:, 0] > 1).any()


def test_list_index_has_bad_rows_and_changes_the_list():
    oh, ow = cc.LIST_HW
    boxes, idx = cc.list_boxes(), cc.list_index()
    assert len(idx) == 700 and (idx < 0).any() and (idx >= 700).any() and len(set(idx.tolist())) < 700
    sel = cc.expected_tiles(cc.index_rows(boxes, idx), oh, ow)
    assert 0 < len(sel) < len(cc.expected_tiles(boxes, oh, ow))
    assert (8, 10) in sel            # the last box's tile: row 699 is listed


def test_numpy_rule_skips_nan_and_clamps_far_coordinates():
    assert cc.axis_range(np.nan, 0.5, 150) is None and cc.axis_range(0.5, np.nan, 150) is None
    assert cc.axis_range(np.inf, np.inf, 150) is None and cc.axis_range(-np.inf, -np.inf, 150) is None
    assert cc.axis_range(1e30, 1e30, 150) is None and cc.axis_range(-1e30, -1e30, 150) is None
    # sample 0 is lo * (size - 1) + 0 * step: a number while the step is one
    assert cc.axis_range(0.5, 1e30, 150) == (73, 149)
    assert cc.axis_range(-1e30, 0.5, 150)[0] == 0
    assert cc.axis_range(0.5, np.inf, 150) is None          # 0 * inf: every sample NaN
    assert cc.axis_range(0.2, 0.1, 150) == cc.axis_range(0.1, 0.2, 150) == (13, 31)
    big = cc.expected_list(cc.big_boxes(), *cc.BIG_HW)
    assert 0 < len(big) < 8190 and big[0] == (0, 0) and (89, 90) in big
