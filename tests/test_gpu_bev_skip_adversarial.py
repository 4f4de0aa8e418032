"""The fp32 BEV net's skip tables under inputs made to expose an under-reach: isolated cells on tile corners, on the
32-bit word seams of the masks, in the first and last row and column of the map, on the edge of the static mask,
diagonal neighbours across a tile corner, a value in the last channel only, -0.0 and denormal cells -- written straight
into the extractor's padded input layout.  Two weight sets: synth.pyramid_params as it is, and the live-fringe set
(|w|, beta = 0) for which tests/test_bev_skip_soundness.py shows on the CPU that every pixel of the true reach changes,
so that a tile skipped wrongly cannot compare equal by luck.  Every comparison is byte-equality between a net with
tables and a net on full tables: every layer buffer, the feature map and the bottleneck."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dodt_amd import config, device, ops, synth
from dodt_amd.core.feature_extractors.vgg_pyramid import BevVggPyr
from tests import test_bev_skip_soundness as sound
from tests import test_bev_support_mask as geom
from tests import test_gpu_bev_frame_skip as fskip
from tests import test_gpu_bev_skip as base

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
ROOT = base.ROOT
PAD, H, W = base.PAD, base.H, base.W
DEPTH = C['bev_depth']
LAST = PAD + H - 1                  # the last real row of the padded map
WEIGHTS = ('plain', 'live')
_CACHE = {}


def _params(kind):
    return synth.pyramid_params(DEPTH) if kind == 'plain' else sound.live_fringe_params(DEPTH)


def _nets(ctx, batch):
    """(net that takes tables, net on full tables, the full tables' layer records), made once per batch size."""
    if batch not in _CACHE:
        nets = []
        for _ in range(2):
            ex = BevVggPyr(ctx=ctx, shared_gpu=True)
            ex.load_params(_params('plain'))
            ex._ensure(batch, H, W, DEPTH)
            nets.append(ex)
        x = ctx.zeros((batch, PAD + H, W, DEPTH), np.float32)
        out = _out_pair(ctx, batch)
        nets[1].set_input(x)
        full = nets[1].forward_timed(None, *out)
        nets[1].set_input(None)
        _CACHE[batch] = (nets[0], nets[1], full)
    return _CACHE[batch]


def _out_pair(ctx, batch):
    return ctx.empty((batch, H, W, 32), np.float32), ctx.empty((batch, H, W, 1), np.float32)


def _frame(cells, value=None):
    """(PAD + H, W, 6) host frame with the cells (y, x, channel) of the padded map set; the pad rows stay zero."""
    x = np.zeros((PAD + H, W, DEPTH), np.float32)
    for k, (y, cx, c) in enumerate(cells):
        assert PAD <= y <= LAST and 0 <= cx < W
        x[y, cx, c] = (1.0, 0.5, 0.75)[k % 3] if value is None else value
    return x


def _real_rows():
    """The static mask that allows every cell of the real rows: cells on the map's borders are legal."""
    m = np.ones((PAD + H, W), np.uint8)
    m[:PAD] = 0
    return m


def _cell_mask(frame):
    return np.any(frame.view(np.uint32) != 0, axis=2).astype(np.uint8)


def _forward(ctx, ex, x, out, layers=True):
    ex.forward_device_padded(x, *out)
    ctx.sync()
    got = {n: ex.activation(n) for n in base.LAYERS} if layers else {}
    got['feat'] = out[0].download()
    got['bneck'] = out[1].download()
    return got


def _compare(ctx, on, off, host, out_on, out_off, what, layers=True):
    """One forward of both nets on the host batch; on == off bit for bit, off finite."""
    x = ctx.array(np.ascontiguousarray(host, np.float32))
    got = _forward(ctx, on, x, out_on, layers)
    want = _forward(ctx, off, x, out_off, layers)
    assert np.isfinite(want['feat']).all() and np.isfinite(want['bneck']).all(), what
    base._assert_same(got, want, what)
    return x


def _expected_items(full, static_mask):
    """Per layer (kept items of the static table, full items) in conv mode 2: layer_masks at each kernel's tiles."""
    masks = geom.layer_masks(static_mask)
    out = []
    for b in full:
        reached, tiles = geom.tiles_reached(masks[b['name']], *fskip.TILE[b['kernel']])
        assert b['items'] % tiles == 0, (b['name'], b['items'], tiles)
        out.append((b['items'] // tiles * reached, b['items']))
    return out


# -- static tables under hand-made masks ------------------------------------------------------------------------------

def static_cell_sets():
    """name -> [(y, x, channel)] in the padded map; the static mask of a set is exactly its cells."""
    sets = {}
    # isolated cells on the corners of 16- and 32-aligned tiles, one per combination
    sets['tile_corners'] = [(yy + 64 * (i + 1), xx + 64 * (j + 2), (4 * i + j) % DEPTH)
                            for i, yy in enumerate((15, 16, 31, 32)) for j, xx in enumerate((15, 16, 31, 32))]
    # the first and last real row, column 0 and column 799
    sets['borders'] = [(PAD, 0, 0), (PAD, W - 1, 1), (LAST, 0, 2), (LAST, W - 1, 3), (PAD, 400, 4), (LAST, 431, 5),
                       (337, 0, 0), (368, W - 1, 1)]
    # diagonal neighbours across a corner shared by 16- and 32-aligned tiles (both diagonals), and a lone value in the
    # last channel
    sets['diagonal'] = [(255, 255, 0), (256, 256, 1), (127, 544, 2), (128, 543, 3), (400, 100, 5)]
    # every position inside a 4 x 4 output block (the F(4x4,3x3) form reaches block-wise), and neighbours on both sides
    # of a block border
    sets['blocks'] = [(448 + 64 * (k // 4) + r, 320 + 64 * (k % 4) + s, k % DEPTH)
                      for k, (r, s) in enumerate(((0, 0), (1, 1), (2, 2), (3, 3), (0, 3), (3, 0), (1, 2), (2, 1)))]
    sets['blocks'] += [(612, 99, 4), (612, 100, 5), (635, 200, 0), (636, 200, 1)]
    return sets


def _run_static(kind):
    ctx = device.default_context()
    mode = ctx.lib.dodt_conv_mode()
    on, off, full = _nets(ctx, 1)
    params = _params(kind)
    on.load_params(params)
    off.load_params(params)
    out_on, out_off = _out_pair(ctx, 1), _out_pair(ctx, 1)
    all_items = sum(b['items'] for b in full)
    for name, cells in static_cell_sets().items():
        everything = _frame(cells)
        mask = _cell_mask(everything)
        assert int(mask.sum()) == len(cells) and not mask[:PAD].any()
        skipped = on.set_input_support(mask)
        print('mode %d %s %s: %d of %d items skipped' % (mode, kind, name, skipped, all_items))
        assert skipped > 0.5 * all_items, (name, skipped, all_items)
        expect = None
        if mode == 2:
            expect = _expected_items(full, mask)
            assert skipped == sum(b - a for a, b in expect), (name, skipped, expect)
        # primed with every cell set, then two subsets, nothing, everything again
        frames = [everything, _frame(cells[0::2]), _frame(cells[1::3]), _frame([]), everything]
        for i, f in enumerate(frames):
            x = _compare(ctx, on, off, f[None], out_on, out_off, '%s %s forward %d' % (kind, name, i))
        if expect:      # the items the kernels ran in steady state, layer by layer
            on.set_input(x)
            steady = on.forward_timed(None, *out_on)
            on.set_input(None)
            assert [(l['name'], l['items']) for l in steady] == [(b['name'], a) for b, (a, _) in zip(full, expect)]
    on.set_input_support(None)


@pytest.mark.parametrize('kind', WEIGHTS)
def test_static_tables_under_hand_made_masks(kind):
    _run_static(kind)


# -- per-frame tables with adversarial frames -------------------------------------------------------------------------

def _erode(m):
    p = np.pad(m.astype(bool), 1)
    return p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]


def frame_cell_sets(static):
    """A and B: isolated cells more than 200 rows apart, inside the static mask.  A: the map's first row and both its
    ends, tile corners and word seams; B: the last row, and where the mask has an edge inside the map, cells on it."""
    static = np.asarray(static).astype(bool)
    a = [(PAD, 0, 0), (PAD, W - 1, 1), (15, 15, 2), (16, 32, 3), (31, 31, 4), (32, 64, 5), (100, 767, 0),
         (101, 768, 1), (63, 415, 5)]
    b = [(LAST, 0, 2), (LAST, W - 1, 3), (LAST, 400, 4), (511, 511, 5), (512, 512, 0), (640, 31, 1), (655, 32, 2),
         (LAST - 15, 416, 3), (592, 399, 5)]
    # (the pad rows count as inside, so that the first real row is no edge)
    edge = static & ~_erode(np.pad(static[PAD:], ((PAD, 0), (0, 0)), constant_values=True))
    edge[:480] = False
    cand = [(int(y), int(x)) for y, x in np.argwhere(edge) if 0 < x < W - 1 and y < LAST]
    corner = [c for c in cand if c[0] % 16 in (0, 15) and c[1] % 16 in (0, 15)]
    on_edge = corner[::max(1, len(corner) // 5)][:5] + cand[::max(1, len(cand) // 5)][:5]
    b += [(y, x, k % DEPTH) for k, (y, x) in enumerate(on_edge)]
    a = [c for c in a if static[c[0], c[1]]]
    b = [c for c in b if static[c[0], c[1]]]
    return a, b, len(on_edge)


def _run_frames(mask_kind, kind):
    ctx = device.default_context()
    mode = ctx.lib.dodt_conv_mode()
    on, off, full = _nets(ctx, 2)
    params = _params(kind)
    on.load_params(params)
    off.load_params(params)
    bp = base._bev_params()
    static = ops.bev_support_mask(bp, PAD) if mask_kind == 'wedge' else _real_rows()
    a, b, n_edge = frame_cell_sets(static)
    assert len(a) >= 5 and len(b) >= 4 and (mask_kind != 'wedge' or n_edge >= 4), (a, b, n_edge)
    assert min(c[0] for c in b) - max(c[0] for c in a) > 200 and not set(a) & set(b)
    assert on.set_input_support(static, frame_tables=True) >= 0
    assert on.frame_tables_on == (mode != 4)        # (F(4x4) reaches block-wise: the static tables stay)
    dense = base._bev_maps(ctx, [synth.lidar_frame(40, 0)], bp).download()[0]
    assert dense.max() <= 1.0 and not (np.any(dense != 0, axis=2) & (static == 0)).any()
    one, two = [c for c in a if c[:2] == (31, 31)], b[-1:]
    assert one and two
    F = dict(A=_frame(a), B=_frame(b), AB=_frame(a + b), empty=_frame([]), dense=dense, one=_frame(one),
             two=_frame(two))
    # (frame 0, frame 1, output pair, compare the layer buffers too).  sparse -> disjoint sparse with the frames
    # swapping (1 -> 2), sparse -> empty -> the same sparse (2 -> 3 -> 4, frame 0), dense -> single cell (7 -> 8,
    # frame 0, and frame 1 the other way round), a single cell behind itself (9 -> 10); pairs 0, 1 and 2 all come back
    steps = [('dense', 'A', 0, False), ('A', 'B', 0, True), ('B', 'A', 0, True), ('empty', 'A', 0, True),
             ('B', 'A', 0, True), ('AB', 'empty', 1, False), ('A', 'B', 1, False), ('dense', 'one', 2, False),
             ('one', 'dense', 2, True), ('one', 'two', 0, False), ('one', 'two', 1, True), ('empty', 'empty', 2, False),
             ('AB', 'dense', 0, False), ('two', 'one', 2, True), ('A', 'B', 1, False)]
    assert len(steps) >= 12 and len({s[2] for s in steps}) >= 3
    model = fskip._Model(static, full, 2) if mode == 2 and on.frame_tables_on else None
    pairs = [_out_pair(ctx, 2) for _ in range(3)]
    ref = _out_pair(ctx, 2)
    for i, (f0, f1, k, layers) in enumerate(steps):
        host = np.stack([F[f0], F[f1]])
        what = '%s %s step %d (%s, %s into pair %d)' % (mask_kind, kind, i, f0, f1, k)
        _compare(ctx, on, off, host, pairs[k], ref, what, layers)
        if model:
            items = on.frame_items()
            expect = model.forward(host, k)
            print('step %2d %-5s %-5s pair %d items %s' % (i, f0, f1, k, items))
            assert items == expect, (i, list(zip(fskip.NAMES, items, expect)))
            if i == 10:     # a single cell behind a single cell: a handful of tiles of the static table
                table = [int(model.static_tiles[n].sum()) * 2 * model.nt[n] for n in fskip.NAMES]
                for li in (1, 3):
                    assert fskip.NAMES[li] in ('conv1_2', 'conv2_2')
                    assert 0 < items[li] < 0.05 * table[li], (fskip.NAMES[li], items[li], table[li])
    on.set_input_support(None)


@pytest.mark.parametrize('kind', WEIGHTS)
@pytest.mark.parametrize('mask_kind', ('wedge', 'ones'))
def test_frame_tables_with_adversarial_frames(mask_kind, kind):
    _run_frames(mask_kind, kind)


# -- signed zero and denormals ----------------------------------------------------------------------------------------

def _run_signed_zero(kind):
    """frame_support_kernel counts a cell that holds only -0.0 as empty.  That is safe if a -0.0 input gives the bits a
    +0.0 input gives: every conv form starts its accumulators at +0.0 and x w with x = -0.0 adds +-0.0.  The net on full
    tables reads the -0.0, the net with per-frame tables skips it: they must agree bit for bit.  A denormal counts as
    non-zero."""
    ctx = device.default_context()
    mode = ctx.lib.dodt_conv_mode()
    on, off, full = _nets(ctx, 1)
    params = _params(kind)
    on.load_params(params)
    off.load_params(params)
    static = _real_rows()
    on.set_input_support(static, frame_tables=True)
    model = fskip._Model(static, full, 1) if mode == 2 and on.frame_tables_on else None
    q = [(PAD, 0, 0), (200, 31, 1), (200, 32, 5), (351, 400, 3), (LAST, W - 1, 2)]
    tiny = np.float32(1e-40)
    assert tiny != 0 and tiny < np.finfo(np.float32).tiny
    negz = _frame(q, -0.0)
    for y, cx, _ in q[1:3]:
        negz[y, cx, :] = -0.0                  # (every channel of a cell)
    assert not np.any(negz != 0) and np.any(negz.view(np.uint32) != 0)
    beside = {}
    for name, v in (('negz', np.float32(-0.0)), ('tiny', tiny)):
        f = _frame([(y, cx + 1, c) for y, cx, c in q[:-1]] + [(LAST, W - 2, 2)], 1.0)
        for y, cx, c in q:
            f[y, cx, c] = v                    # next to a +1.0 cell ...
        f[200, 33, 0] = v                      # ... and inside one, in another channel
        beside[name] = f
    F = dict(ones=_frame(q, 1.0), empty=_frame([]), negz=negz, negz_beside=beside['negz'], tiny=_frame(q, tiny),
             tiny_beside=beside['tiny'])
    out_on, out_off = _out_pair(ctx, 1), _out_pair(ctx, 1)
    steps = ['ones', 'negz', 'empty', 'empty', 'negz', 'negz_beside', 'negz', 'tiny', 'empty', 'tiny_beside', 'tiny',
             'ones']
    for i, name in enumerate(steps):
        _compare(ctx, on, off, F[name][None], out_on, out_off, '%s step %d (%s)' % (kind, i, name))
        if model:
            items = on.frame_items()
            expect = model.forward(F[name][None], 0)     # (numpy's != 0 takes -0.0 for zero, as the kernel does)
            assert items == expect, (i, name, list(zip(fskip.NAMES, items, expect)))
            if i == 4:       # -0.0 cells behind an empty frame: nothing runs
                assert items == [0] * len(items), items
            if i == 7:       # denormal cells behind -0.0 cells: the denormals' tiles alone
                assert all(0 < n for n in items), items
    on.set_input_support(None)


@pytest.mark.parametrize('kind', WEIGHTS)
def test_negative_zero_counts_as_empty_and_denormals_as_cells(kind):
    _run_signed_zero(kind)


# -- the other conv forms ---------------------------------------------------------------------------------------------

def _run_all():
    for kind in WEIGHTS:
        _run_static(kind)
        for mask_kind in ('wedge', 'ones'):
            _run_frames(mask_kind, kind)
        _run_signed_zero(kind)


@pytest.mark.parametrize('mode', ['0', '4'])
def test_other_conv_forms_in_child_process(mode):
    """DODT_CONV_WINO is read once per process: the direct kernels (0) and F(4x4,3x3) (4, static tables only: the
    hand-made masks are what reaches its block-wise rule), one fresh child each."""
    env = dict(os.environ, DODT_CONV_WINO=mode)
    code = ('import sys; sys.path.insert(0, %r); import tests.test_gpu_bev_skip_adversarial as t; '
            't._run_all(); print("ok")' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
