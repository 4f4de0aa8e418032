"""What the cases of tests/_fc_cases.py reach, proved on the host: no GPU.

tests/test_gpu_fc_forms.py runs the table on the device and asserts that each built layer selects what the host plan
says (FullyConnected.form == ops.fc_plan_host); this file computes the plans with dodt_fc_plan_host -- the library's
own select_fc_form on the traits dodt_fc_create_ex builds a layer from -- and asserts that together they

  * select every form of the selector, kNone and the 64-k stage depth of the bf16-row kernel included, and every one of
    the 28 kernel instantiations behind it (UNREACHABLE is empty);
  * take every fallback of the selector, sit on both sides of the 512-tile switch of fc_dma_kernel, and cut, per
    kernel, a ragged last m-tile, a ragged last n-tile and rows by the device count;
  * contain every instantiation the workload's own layer calls run;

and that every 'int' case's comparison rejects a reference that lost a k, swapped two k, or lost its last row or
column -- so that degenerate data cannot hide a kernel error."""
import numpy as np
import pytest

import _fc_cases as fcc
from dodt_amd import ops

CASES, REFUSED = fcc.CASES, fcc.REFUSED

# instantiation -> why no call can reach it, from select_fc_form / launch_fc's code.  Empty: all 28 are reached.
UNREACHABLE = {}


def _plans(bf16_bk=32):
    return [(c, fcc.host_plan(c, bf16_bk)) for c in CASES]


def _by_name(name):
    return next(c for c in CASES + REFUSED if c.name == name)


def test_cases_plan_the_form_they_are_there_for():
    for bk in (32, 64):
        for c in CASES + REFUSED:
            p = fcc.host_plan(c, bk)
            assert p['name'] == fcc.expected_form(c, bk), (c.name, p)
            if p['name'].startswith('kTiled'):
                assert (p['xvec'], p['fuse']) == (c.xvec, int(c.fuse)), (c.name, p)
            else:
                assert c.xvec is None and p['xvec'] == 0 and p['fuse'] == 0, (c.name, p)
            assert p['name'] == 'kNone' or fcc.group(p['name']) in fcc.GROUPS


def test_cases_stay_small():
    for c in CASES + REFUSED:
        assert c.M * c.K * c.N <= fcc.MAX_WORK, c.name
        assert c.K <= 2048          # |sum| <= 64 K + 8 < 2^24: the 'int' data's sums are exact in float32


def test_every_form_is_selected():
    names = set(p['name'] for _, p in _plans(32)) | set(p['name'] for _, p in _plans(64)) | \
        set(fcc.host_plan(c)['name'] for c in REFUSED)
    assert names == {'kNone', 'kSmallK', 'kSkinny', 'kSkinnyBf16', 'kSkinnyBf16Rows', 'kDmaNt1', 'kDmaNt2', 'kDmaFused',
                     'kBf16RowsDma32', 'kBf16RowsDma64', 'kTiled64x128', 'kTiled128x32', 'kTiled64x128Bf16',
                     'kTiled128x32Bf16'}
    # the integers are the header's DODT_FC_FORM_*
    forms = dict((p['name'], p['form']) for bk in (32, 64) for _, p in _plans(bk))
    assert forms['kSmallK'] == 1 and forms['kDmaNt2'] == 6 and forms['kBf16RowsDma64'] == 9 and \
        forms['kTiled128x32Bf16'] == 13 and fcc.host_plan(REFUSED[0])['form'] == 0
    assert sorted(forms.values()) == list(range(1, 14))


def test_every_kernel_instantiation_is_reached():
    reached = set(fcc.instantiation(p, c.dtype, c.fuse) for bk in (32, 64) for c, p in _plans(bk))
    assert not set(UNREACHABLE) & reached, 'reached after all: %s' % sorted(set(UNREACHABLE) & reached)
    assert sorted(reached | set(UNREACHABLE)) == fcc.ALL_INSTANTIATIONS
    assert all(len(why) > 40 for why in UNREACHABLE.values())
    # both row stores of the small-K kernel, in both arithmetics
    stores = set((c.dtype, p['vec_store']) for c, p in _plans() if p['name'] == 'kSmallK')
    assert stores == {('f32', 0), ('f32', 1), ('bf16', 0), ('bf16', 1)}
    # the mean inside the small-K kernel and without it
    assert set((c.dtype, c.fuse) for c, p in _plans() if p['name'] == 'kSmallK') == \
        {('f32', False), ('f32', True), ('bf16', False), ('bf16', True)}


def test_every_fallback_of_the_selector_is_taken():
    def plan(name):
        c = _by_name(name)
        p = fcc.host_plan(c)
        return c, p, (p['name'], p['xvec'], p['fuse'])

    # a skinny layer (the traits say so) ...
    for name, want in [('skinny-x2-33x16x17-f32', ('kTiled128x32', 1, 1)),            # ... with a second input
                       ('skinny-ldx17-33x16x17-f32', ('kTiled128x32', 0, 0)),         # ... rows 4 bytes apart mod 16
                       ('skinny-xoff4-33x16x17-f32', ('kTiled128x32', 1, 0)),         # ... x 4 bytes off
                       ('skinny-x2-33x16x17-bf16', ('kTiled128x32Bf16', 1, 1)),
                       ('skinny-ldx17-33x16x17-bf16', ('kTiled128x32Bf16', 0, 0)),
                       ('skinny-xoff4-33x16x17-bf16', ('kTiled128x32Bf16', 1, 0))]:
        c, p, got = plan(name)
        assert p['skinny'] and got == want, (name, p)
    c, p, _ = plan('skinny-xoff4-33x16x17-f32')
    assert c.x_off == 4 and c.ldx % 4 == 0 and not c.fuse
    c, p, _ = plan('skinny-ldx17-33x16x17-f32')
    assert c.x_off == 0 and c.ldx == c.K + 1
    # a layer with the LDS-DMA kernel
    for name, want in [('t128-xoff4-65x64x128', ('kTiled64x128', 1, 0)), ('t128-ldx65-65x64x128', ('kTiled64x128', 0, 0)),
                       ('t128-x2off4-65x64x128', ('kTiled64x128', 1, 1))]:
        c, p, got = plan(name)
        assert p['dma'] and got == want and (c.M, c.K, c.N) == (65, 64, 128), (name, p)
    assert _by_name('t128-x2off4-65x64x128').x_off == 0 and _by_name('t128-x2off4-65x64x128').x2_off == 4
    # a small-K layer whose y is 4 bytes off, at both weight blockings; one whose N is no multiple of 4
    for name, want in [('smallk-yoff4-37x9x64-f32', 'kTiled128x32'), ('smallk-yoff4-37x9x128-f32', 'kTiled64x128'),
                       ('smallk-yoff4-37x9x64-bf16', 'kTiled128x32Bf16'), ('smallk-yoff4-37x9x128-bf16', 'kTiled64x128Bf16')]:
        c, p, got = plan(name)
        assert p['smallk'] and c.y_off == 4 and got[0] == want, (name, p)
    c, p, got = plan('smallk-n66-37x12x66-f32')
    assert not p['plain'] and got[0] == 'kTiled128x32' and p['grid'] == (1, 3)
    # bf16 rows 8 but not 16 bytes aligned feed the skinny kernel; refusals plan kNone
    c, p, got = plan('skinny-bf16_rows-33x144x17-xoff8')
    assert c.x_off == 8 and got[0] == 'kSkinnyBf16Rows'
    for c in REFUSED:
        p = fcc.host_plan(c)
        assert p['name'] == 'kNone' and p['grid'] == (0, 0), (c.name, p)
    assert [(c.K, c.N, c.y_bf16) for c in REFUSED] == [(120, 128, False), (128, 130, False), (144, 17, True)]


def test_both_sides_of_the_tile_switch():
    lo, hi = fcc.host_plan(_by_name('dma1-32704x64x128')), fcc.host_plan(_by_name('dma2-32705x64x128'))
    assert (lo['name'], lo['grid']) == ('kDmaNt1', (511 * 2, 1))      # 511 tiles of 64 x 128 = 1022 of 64 x 64
    assert (hi['name'], hi['grid']) == ('kDmaNt2', (512, 1))
    # the XCD map's two branches with a ragged N: 512 tiles, and 513
    a, b = fcc.host_plan(_by_name('dma2-4040x64x1024')), fcc.host_plan(_by_name('dma2-3648x64x1100'))
    assert a['name'] == b['name'] == 'kDmaNt2' and a['grid'][0] == 512 and b['grid'][0] == 513 and b['Npad'] == 1152
    nt1 = [p['grid'][0] for c, p in _plans() if p['name'] == 'kDmaNt1']
    assert any(g % 8 == 0 for g in nt1) and any(g % 8 for g in nt1)


# tile of a form: rows, columns (0: the kernel has no n-tiles)
def _tile(p):
    f = p['name']
    if f == 'kSmallK':
        return 1, 0
    if f.startswith('kSkinny'):
        return 16, 0
    if f in ('kDmaNt1', 'kDmaFused'):
        return 64, 64
    if f == 'kDmaNt2' or f.startswith('kBf16RowsDma') or '64x128' in f:
        return 64, 128
    return 128, 32


def test_every_kernel_cuts_ragged_tiles_and_rows():
    seen = dict((g, set()) for g in fcc.GROUPS)
    for c, p in _plans():
        g, (bm, bn) = fcc.group(p['name']), _tile(p)
        if c.M % bm:
            seen[g].add('ragged m')
        if bn and c.N % bn:
            seen[g].add('ragged n')
        if c.data == 'int' and c.d_m is not None:
            if c.d_m == 0:
                seen[g].add('d_m 0')
            elif c.d_m == c.M:
                seen[g].add('d_m M')
            elif c.d_m == c.M + 5:
                seen[g].add('d_m beyond M')
            elif 0 < c.d_m < c.M and c.d_m % 32:
                seen[g].add('d_m inside a 32-row tile')
    for g in fcc.GROUPS:
        want = {'d_m 0', 'd_m M', 'd_m beyond M', 'd_m inside a 32-row tile'}
        if g != 'smallk':
            want.add('ragged m')        # (a thread of the small-K kernel is one row: it has no m-tile)
        # the bf16-row kernel refuses N % 128 != 0 (REFUSED), the small-K and the skinny kernel have no n-tiles
        if g not in ('smallk', 'skinny', 'bf16_rows_dma'):
            want.add('ragged n')
        assert want <= seen[g], (g, sorted(want - seen[g]))
    # the two tile shapes of the register-staged kernel each, both arithmetics
    for form in ('kTiled64x128', 'kTiled128x32', 'kTiled64x128Bf16', 'kTiled128x32Bf16'):
        mine = [c for c, p in _plans() if p['name'] == form]
        bm, bn = (64, 128) if '64x128' in form else (128, 32)
        assert any(c.M % bm for c in mine) and any(c.N % bn for c in mine), form
        assert any(c.d_m is not None and 0 < c.d_m < c.M for c in mine), form
    # a 64-column tile of fc_dma_kernel<false, 1> that lies wholly beyond N
    assert any(p['name'] == 'kDmaNt1' and p['Npad'] - c.N >= 64 for c, p in _plans())


def test_the_workloads_calls_are_in_the_table():
    have = set((fcc.instantiation(p, c.dtype, c.fuse), p['vec_store']) for c, p in _plans())
    forms = set()
    for what, K, N, M, dtype, kw in fcc.WORKLOAD:
        p = ops.fc_plan_host(K, N, M, dtype=dtype, **kw)
        assert p['name'] != 'kNone', what
        fuse = kw.get('x2_off') is not None
        assert (fcc.instantiation(p, dtype, fuse), p['vec_store']) in have, (what, p)
        forms.add(p['name'])
    assert forms == {'kSmallK', 'kDmaNt1', 'kTiled64x128Bf16', 'kSkinny', 'kSkinnyBf16', 'kSkinnyBf16Rows',
                     'kBf16RowsDma32'}


def test_plan_arguments_are_checked():
    with pytest.raises(ValueError):
        ops.fc_plan_host(64, 64, 1, bf16_bk=48)
    with pytest.raises(ValueError):
        ops.fc_plan_host(64, 64, 1, x_off=16)
    with pytest.raises(ValueError):
        ops.fc_plan_host(0, 64, 1)
    p = ops.fc_plan_host(129, 256, 65, dtype='bf16', x_bf16=True, ldx=192, bf16_bk=64)
    assert (p['name'], p['Kd'], p['dma_bk'], p['bf16_rows'], p['Kp'], p['BN'], p['Npad']) == \
        ('kBf16RowsDma64', 192, 64, 1, 256, 128, 256)
    p = ops.fc_plan_host(9, 100, 7)
    assert (p['name'], p['plain'], p['smallk'], p['Kp'], p['BN'], p['Npad'], p['grid']) == \
        ('kSmallK', 1, 1, 64, 32, 128, (1, 1))


# ---- the comparison of every 'int' case can fail ---------------------------------------------------------------------

INT_CASES = [c for c in CASES if c.data == 'int']


def _mutants(c):
    """References a wrong kernel could produce, as float32 (M, N): (what, array)."""
    w, b = fcc.layer_params(fcc.layer_key(c))
    x = fcc.fused_rows(c).astype(np.float64)
    w64 = w.astype(np.float64)
    full = x @ w64 + b.astype(np.float64)

    def done(y):
        y = y.astype(np.float32)
        return np.maximum(y, np.float32(0)) if c.relu else y

    assert np.array_equal(done(full), fcc.reference(c))
    out = []
    for k in sorted(set([c.K - 1, c.K // 2, 0])):
        out.append(('k = %d dropped' % k, done(full - np.outer(x[:, k], w64[k]))))
    if c.K >= 2:
        k1, k2 = 0, c.K - 1
        d = x[:, k1] - x[:, k2]
        out.append(('k = %d and %d of x swapped' % (k1, k2), done(full - np.outer(d, w64[k1]) + np.outer(d, w64[k2]))))
    else:
        # K = 1: the only k swapped with its neighbour in the row, which is the row's poisoned padding
        assert c.ldx > c.K
        out.append(('k = 0 swapped with the padding behind it', done(full * np.nan)))
    n = fcc.rows(c)
    z = fcc.reference(c).copy()
    z[:, c.N - 1] = 0
    out.append(('last column zeroed', z))
    z = fcc.reference(c).copy()
    z[n - 1] = 0
    out.append(('last valid row zeroed', z))
    if c.widths:                                    # the last column of every part
        for end in np.cumsum(c.widths):
            z = fcc.reference(c).copy()
            z[:, end - 1] = 0
            out.append(('column %d zeroed' % (end - 1), z))
    return out


@pytest.mark.parametrize('c', INT_CASES, ids=[c.name for c in INT_CASES])
def test_the_comparison_of_an_int_case_can_fail(c):
    want = fcc.reference(c)
    assert np.abs(want).max() <= 64 * c.K + 8
    good = fcc.expected_images(c, want)
    assert fcc.check_outputs(c, good, want) == []
    n = fcc.rows(c)
    if n == 0:
        # nothing may be written: any element written anywhere is a complaint (there is no reference to mutate)
        for img in good:
            assert (img == fcc.y_sentinel(c)).all()
        for r, col in ((0, 0), (c.M - 1, good[-1].shape[1] - 1), (c.M + fcc.Y_EXTRA_ROWS - 1, 0)):
            bad = [g.copy() for g in good]
            bad[-1][r, col] = 0
            assert fcc.check_outputs(c, bad, want), (r, col)
        return
    for what, wrong in _mutants(c):
        assert fcc.check_outputs(c, fcc.expected_images(c, wrong), want), what
    # ... and a write behind the valid region, in the row stride's padding or below the last row
    for r, col in ((n, 0), (0, good[0].shape[1] - 1)):
        if col >= fcc.y_shapes(c)[0][2] or r >= n:
            bad = [g.copy() for g in good]
            bad[0][r, col] = 0
            assert fcc.check_outputs(c, bad, want), (r, col)


def test_normal_cases_cover_every_kernel():
    groups = set(fcc.group(fcc.host_plan(c)['name']) for c in CASES if c.data == 'normal')
    assert groups == set(fcc.GROUPS)
