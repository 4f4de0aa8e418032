"""The two lists a forward on per-frame tables takes (dodt_frame_lists_host, the functions of frame_tables.h the device
builder runs): run = the items this frame reaches, restore = the items the previous frame reached and this one does
not, both in the table's order; merged in that order they are the union dodt_frame_tables_host returns.  Checked
against numpy for real and synthetic frame pairs, the previous frame a real one."""
import os

import numpy as np

from dodt_amd import ops, synth
from tests import test_bev_frame_tables as ft
from tests import test_bev_support_mask as geom

GOLDEN = ft.GOLDEN
PAD = ft.PAD


def _check(prev_masks, now_masks, static_mask):
    """Every layer: run and restore against numpy's A_now and A_prev \\ A_now.  Returns {layer: (run, restore)}."""
    frames = len(now_masks)
    static = geom.layer_masks(static_mask)
    now = [geom.layer_masks(m) for m in now_masks]
    before = [geom.layer_masks(m) for m in prev_masks]
    counts = {}
    for li, name in enumerate(ft.LAYERS):
        th, tw = ft.TILES[name][:2]
        table = ft._filter(name, ft._table(name, frames), [static] * frames)
        a_now = set(ft._filter(name, table, now))
        a_prev = set(ft._filter(name, table, before))
        prev = np.asarray([it in a_prev for it in table], np.uint8)
        want_run = [it for it in table if it in a_now]
        want_restore = [it for it in table if it in a_prev and it not in a_now]
        items = np.asarray(table, np.int32)
        run, restore = ops.frame_lists_host(np.stack(now_masks), li, th, tw, items, prev=prev)
        assert [tuple(r) for r in run] == want_run, name
        assert [tuple(r) for r in restore] == want_restore, name
        # merged in table order: the union the existing entry returns
        both = set(want_run) | set(want_restore)
        union = ops.frame_tables_host(np.stack(now_masks), li, th, tw, items, prev=prev)
        assert [tuple(r) for r in union] == [it for it in table if it in both], name
        assert len(union) == len(run) + len(restore)
        # without a previous frame nothing is restored
        run0, restore0 = ops.frame_lists_host(np.stack(now_masks), li, th, tw, items)
        assert [tuple(r) for r in run0] == want_run and len(restore0) == 0, name
        counts[name] = (len(run), len(restore))
    return counts


def _not_vacuous(counts, what):
    for layer in ('conv1_2', 'conv2_2'):
        run, restore = counts[layer]
        assert 0 < restore < run, (what, layer, run, restore)


def test_golden_frames():
    g = np.load(os.path.join(GOLDEN, 'frames.npz'))
    names = sorted({k[:-5] for k in g.files if k.endswith('_xyzi')})
    assert names
    for name in names:
        bp, cal = ft._calib(g[name + '_p2'], g[name + '_r0'], g[name + '_tr'], g[name + '_imwh'])
        static = ops.bev_support_mask(bp, PAD)
        full = ft._frame_mask(g[name + '_xyzi'], cal)
        thin = ft._frame_mask(g[name + '_xyzi'][::4], cal)
        other = ft._frame_mask(synth.lidar_frame(5, 3), cal)
        # the decimated cloud behind the full one restores what it no longer reaches; a synthetic frame behind both
        _not_vacuous(_check([full, full], [thin, thin], static), name)
        _check([thin, full], [other, thin], static)
        counts = _check([thin, thin], [full, full], static)        # (a superset of the previous frame: nothing to restore)
        assert all(restore == 0 for _, restore in counts.values()), (name, counts)


def test_synthetic_frame_pairs():
    """The frames the benchmark feeds: batch i = sequence i, frames (2 i, 2 i + 2); and consecutive pairs of one
    sequence."""
    bp, cal = ft._calib()
    static = ops.bev_support_mask(bp, PAD)
    pairs = [[ft._frame_mask(synth.lidar_frame(i, f), cal) for f in (2 * i, 2 * i + 2)] for i in range(3)]
    for k in range(3):
        _not_vacuous(_check(pairs[k], pairs[(k + 1) % 3], static), 'sequence %d -> %d' % (k, (k + 1) % 3))
    seq = [ft._frame_mask(synth.lidar_frame(0, f), cal) for f in (0, 2, 4)]
    _not_vacuous(_check(seq[0:2], seq[1:3], static), 'frames (0, 2) -> (2, 4)')


def test_empty_and_wedge_filling_frames():
    bp, cal = ft._calib()
    static = ops.bev_support_mask(bp, PAD)
    empty = np.zeros((PAD + 700, 800), np.uint8)
    frame = ft._frame_mask(synth.lidar_frame(1, 1), cal)
    counts = _check([frame], [empty], static)           # everything the frame reached goes back
    assert all(run == 0 and restore > 0 for run, restore in counts.values()), counts
    counts = _check([frame], [static], static)          # every cell the voxeliser can write: the static table runs
    assert all(restore == 0 for _, restore in counts.values()), counts
