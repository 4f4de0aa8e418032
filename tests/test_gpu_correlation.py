"""correlation.hip on the device against a float64 reference, at the cases of tests/_corr_cases.py.  Needs an MI355X.

What the older correlation tests cannot see (tests/test_corr_walk.py proves on the host that these cases do):
persistent workgroups that take a second and later tiles -- the next tile's A pixel loaded under the arithmetic, its
neighbourhood arriving in two parts around the output phase -- under short grids (DODT_CORR_GRID) and on the device's
own; every displacement channel of every pixel compared, element by element, with a bound derived from float32
arithmetic (_corr_cases.bound), and bit for bit on integer maps; nothing written outside the map; the two-pass and
the half-wave forms held to the same; the tile-list kernel over three chunks of boxes with NaN, infinite and huge
edges, at its limits and its clamps; the entry points' refusals.

Every launch happens in a child process of its mode (the library reads DODT_CORR_* once per process), one child per
mode, one after another; this process only compares.  After a child that ended by a signal, an abort or its time
limit no further child is started (_corr_cases.run_mode)."""
import json

import numpy as np
import pytest

import _corr_cases as cc

pytestmark = pytest.mark.gpu
u32 = np.uint32


@pytest.fixture(scope='module')
def outdir(tmp_path_factory):
    return tmp_path_factory.mktemp('corr')


_refs = {}


def _reference(c, kind):
    """(ref, mag) of a case's pair, computed once and shared; callers must not write into it."""
    key = (cc.case_id(c), kind)
    if key not in _refs:
        a, b = cc.pair(c, kind)
        _refs[key] = cc.reference(a, b, c.md, c.s2, c.pad)
    return _refs[key]


def _split(buf, c):
    """(map, guard) of a downloaded buffer."""
    OH, OW, K = cc.out_shape(c.H, c.W, c.md, c.s2, c.pad)
    assert buf.shape == (OH * OW * K + cc.GUARD,)
    return buf[:OH * OW * K].reshape(OH, OW, K), buf[OH * OW * K:]


def _bits_equal(x, y):
    return x.shape == y.shape and np.array_equal(x.view(u32), y.view(u32))


def _check(buf, c, kind, what, ref=None, mag=None):
    """A downloaded buffer against the reference: exact on integer maps, within the bound on normal ones; no NaN
    left in the map, every NaN left in the guard.  Prints the figure before it asserts."""
    got, guard = _split(buf, c)
    if ref is None:
        ref, mag = _reference(c, kind)
    assert np.isnan(guard).all(), '%s: %d floats written behind the map' % (what, (~np.isnan(guard)).sum())
    assert not np.isnan(got).any(), '%s: %d elements of the map not written' % (what, np.isnan(got).sum())
    if kind == 'int':
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, '%s: %d elements differ, first at (y, x, k) = %s' % (what, len(bad), bad[0])
        return 0.0
    ratio = cc.worst_ratio(got, ref, mag)
    print('RATIO %s %.4f' % (what, ratio))
    bad = np.argwhere(np.abs(got - ref) > cc.bound(mag))
    assert len(bad) == 0, '%s: %d elements beyond the bound (worst %.3g of it), first at (y, x, k) = %s' % (
        what, len(bad), ratio, bad[0])
    return ratio


# ---- every mode against the reference ------------------------------------------------------------------------------
PARITY = [(m, c, kind) for m in cc.MODES for c in cc.CASES if m in c.modes for kind in cc.KINDS]


@pytest.mark.parametrize('mode,c,kind', PARITY, ids=['%s-%s-%s' % (m, cc.case_id(c), k) for m, c, k in PARITY])
def test_matches_float64_reference(outdir, mode, c, kind):
    out = cc.run_mode(mode, outdir)
    _check(out['par__%s__%s' % (cc.case_id(c), kind)], c, kind, '%s %s' % (mode, cc.case_id(c)))


# ---- across modes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['grid8', 'grid16', 'grid24', 'two_pass'])
def test_bit_equal_to_the_default_whoever_walks_the_tile(outdir, mode):
    """A pixel's arithmetic does not depend on the grid, and the two-pass kernel sums in the one-pass kernel's
    order (correlation.hip: 'Same sums in the same order')."""
    base, out = cc.run_mode('default', outdir), cc.run_mode(mode, outdir)
    shared = [k for k in out if k.startswith('par__') and k in base]
    assert len(shared) >= 2 * len(cc.WALK)
    differ = [k for k in shared if not _bits_equal(out[k], base[k])]
    assert not differ, differ


def test_half_wave_form_does_not_depend_on_the_grid(outdir):
    a, b = cc.run_mode('halves2', outdir), cc.run_mode('halves2_grid8', outdir)
    assert sorted(a) == sorted(b) and len(a) == 2 * len(cc.WALK)
    differ = [k for k in a if not _bits_equal(a[k], b[k])]
    assert not differ, differ


# ---- aliasing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cc.KINDS)
def test_a_map_correlated_with_itself(outdir, kind):
    out = cc.run_mode('grid8', outdir)
    a, _ = cc.pair(cc.BASE, kind)
    ref, mag = cc.reference(a, a, cc.BASE.md, cc.BASE.s2, cc.BASE.pad)
    _check(out['alias__' + kind], cc.BASE, kind, 'grid8 alias', ref, mag)


# ---- locality ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['default', 'grid8'])
def test_a_poisoned_pixel_shows_in_the_outputs_that_read_it_and_nowhere_else(outdir, mode):
    c = cc.BASE
    got, guard = _split(cc.run_mode(mode, outdir)['locality'], c)
    a, b = cc.locality_pair()
    assert (a != 0).all() and (~np.isfinite(b)).sum() == len(cc.POISON)
    ref, mag = cc.reference(a, b, c.md, c.s2, c.pad)
    assert np.isnan(guard).all()
    # by the geometry: B[py, px] is read by output (py - s2p, px - s2o) in channel k(s2p, s2o); md == pad, so A is
    # inside the image for every output and no product is 0 * inf
    want = np.zeros(got.shape, bool)
    for py, px, _ch in cc.POISON:
        hits = 0
        for k in range(25):
            y, x = py - (k // 5 - 2) * 2, px - (k % 5 - 2) * 2
            if 0 <= y < c.H and 0 <= x < c.W:
                want[y, x, k] = True
                hits += 1
        assert hits == (9 if (py, px) in ((0, 0), (c.H - 1, c.W - 1)) else 25)
    assert np.array_equal(~np.isfinite(ref), want)
    assert np.array_equal(~np.isfinite(got), want)
    assert np.array_equal(got[want], ref[want].astype(np.float32))        # one infinite term: its sign
    clean = ~want
    ratio = cc.worst_ratio(np.where(clean, got, 0), np.where(clean, ref, 0), np.where(clean, mag, 0))
    print('RATIO %s locality %.4f' % (mode, ratio))
    assert (np.abs(got[clean] - ref[clean]) <= cc.bound(mag[clean])).all()


# ---- listed tiles under a short grid -------------------------------------------------------------------------------
@pytest.mark.parametrize('count', cc.LISTED['counts'] + ('cap0',))
def test_listed_tiles_under_a_short_grid(outdir, count):
    """17 shuffled tiles, of which the device's count takes some: 13 make two tiles per workgroup on a grid of 8 (and
    one XCD idle); a count above the capacity is clamped to it, a negative one to 0."""
    c = cc.BASE
    out = cc.run_mode('grid8', outdir)
    full, _ = _split(out['listed__full'], c)
    _check(out['listed__full'], c, 'normal', 'grid8 listed, full map')
    got, guard = _split(out['listed__%s' % count], c)
    tiles, _ = cc.listed_tiles()
    n = 0 if count == 'cap0' else min(max(count, 0), cc.LISTED['n_list'])
    m = np.zeros(got.shape[:2], bool)
    for ty, tx in tiles[:n]:
        m[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = True
    assert m.any() == (n > 0)
    assert np.isnan(guard).all()
    assert _bits_equal(got[m], full[m])
    assert np.isnan(got[~m]).all()


# ---- full size -----------------------------------------------------------------------------------------------------
def test_full_size_bands_match_float64_reference(outdir):
    """(700,800,32), a != b: 2200 tiles, four or five per workgroup on the device's own grid.  Row bands at the top,
    across a super-block seam, in the middle and in the ragged last tile row, all 800 columns and 25 channels."""
    out = cc.run_mode('default', outdir)
    assert int(out['full__nans']) == 0 and np.isnan(out['full__guard']).all()
    assert len(out['full__guard']) == cc.GUARD
    c = cc.FULL
    a, b = cc.full_pair()
    worst = 0.0
    for y0, y1 in cc.FULL_BANDS:
        got = out['full__band_%d' % y0]
        ref, mag = cc.reference(a, b, c.md, c.s2, c.pad, rows=(y0, y1))
        assert got.shape == ref.shape == (y1 - y0, 800, 25)
        ratio = cc.worst_ratio(got, ref, mag)
        print('RATIO default full rows %d:%d %.4f' % (y0, y1, ratio))
        worst = max(worst, ratio)
        bad = np.argwhere(np.abs(got - ref) > cc.bound(mag))
        assert len(bad) == 0, 'rows %d:%d: %d elements beyond the bound, first at %s' % (y0, y1, len(bad), bad[0])
    assert worst > 0


# ---- the tile list -------------------------------------------------------------------------------------------------
def _listed(out, name):
    nt = int(out['tl__%s__n' % name][0])
    tiles = out['tl__%s__tiles' % name]
    assert 0 <= nt <= len(tiles)
    assert (tiles[nt:] == -1).all()                      # nothing written past the count
    return [(int(t) >> 16, int(t) & 0xffff) for t in tiles[:nt]]


@pytest.mark.parametrize('name', ['plain', 'indexed'])
def test_tile_list_of_700_boxes_follows_the_numpy_rule_and_serves_every_crop(outdir, name):
    """Three chunks of 256 boxes, the last one partial; NaN, infinite, huge, flipped, degenerate and outside boxes;
    with an index list: negative and too-large indices, repeats."""
    out = cc.run_mode('default', outdir)
    oh, ow = cc.LIST_HW
    boxes = cc.list_boxes()
    rows = boxes if name == 'plain' else cc.index_rows(boxes, cc.list_index())
    tiles = _listed(out, name)
    assert tiles == cc.expected_list(rows, oh, ow)
    # the map over the list: the listed tiles are written, nothing else is
    m = np.zeros((oh, ow), bool)
    for ty, tx in tiles:
        m[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = True
    assert np.array_equal(out['tl__%s__part_nan' % name], ~m)
    # the contract: crops of that map are crops of the full map, all 700 rows
    full, part = out['tl__%s__crops_full' % name], out['tl__%s__crops_part' % name]
    assert full.shape == (cc.N_BOXES, 7 * 7 * 25) and np.isfinite(full).all()
    assert np.count_nonzero(np.abs(full).max(1)) > 350
    assert _bits_equal(part, full)


def test_tile_list_clamps_the_devices_count(outdir):
    out = cc.run_mode('default', outdir)
    oh, ow = cc.LIST_HW
    assert _listed(out, 'neg') == []
    assert _listed(out, 'above') == cc.expected_list(cc.list_boxes()[:300], oh, ow)
    assert _listed(out, 'none') == []


def test_tile_list_of_8190_tiles(outdir):
    out = cc.run_mode('default', outdir)
    assert len(out['tl__big__tiles']) == 8190
    assert _listed(out, 'big') == cc.expected_list(cc.big_boxes(), *cc.BIG_HW)


# ---- what the entry points refuse -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kind,text', [
    ('c16', 'ValueError', 'only 32 channels'), ('k121', 'ValueError', '121 displacement channels exceed 32'),
    ('empty', 'ValueError', 'empty output'), ('tiles_c16', 'ValueError', 'only 32 channels'),
    ('tiles_empty', 'ValueError', 'empty output'), ('tiles_generic', 'DodtError', 'only the 5 x 5 grid'),
    ('list_too_big', 'ValueError', '91 x 91 tiles, at most 8192'),
    ('list_capacity', 'ValueError', 'room for 129 tiles, the map has 130')])
def test_refusals(outdir, name, kind, text):
    got = json.loads(str(cc.run_mode('default', outdir)['errors']))[name]
    assert got.startswith(kind + ':') and text in got, got
    if name == 'tiles_generic':
        assert '(status 3)' in got              # DODT_ERR_UNSUPPORTED
