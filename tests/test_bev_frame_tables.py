"""Per-frame skip tables of the fp32 BEV net, the rule on the host (dodt_frame_tables_host: the same functions the
device builder runs, frame_tables.h): a frame's non-zero BEV cells, propagated through the net's geometry at cell
resolution, keep the items of a layer's static skip table that the frame reaches, in the table's order.  Checked
against the numpy propagation of tests/test_bev_support_mask.py for real, synthetic, empty and wedge-filling frames."""
import os

import numpy as np
import pytest

from dodt_amd import config, ops, synth
from oracle import pipeline as opipe
from tests import test_bev_support_mask as geom

C = config.PYRAMID_DODT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PAD = 4
LAYERS = ('conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2',
          'conv4_3', 'upconv3', 'pyramid_fusion3', 'upconv2', 'pyramid_fusion2', 'upconv1', 'pyramid_fusion1')
# (tile rows, tile columns on the layer's GEMM grid, channel tiles, channel tiles of a pixel tile adjacent): the fp32
# net's kernels -- the first-layer kernel's 16 x 32 tiles, 16 x 16 for the Winograd and transposed-conv kernels
TILES = {n: (16, 16, 2, True) for n in LAYERS}
TILES['conv1_1'] = (16, 32, 1, False)
TILES['conv4_2'] = (16, 16, 4, True)


def _calib(p2=synth.P2, r0=synth.R0_RECT, tr=synth.TR_VELO_TO_CAM, imwh=synth.IMAGE_WH):
    p2, r0, tr = (np.asarray(a, np.float64) for a in (p2, r0, tr))
    bp = ops.make_bev_params(C, config.velo_to_cam(r0, tr), p2, tuple(imwh))
    return bp, (r0, tr, p2, tuple(imwh))


def _frame_mask(xyzi, cal):
    """(PAD + 700, 800) uint8: the non-zero cells (any channel) of the frame's BEV input, padded like the extractor's."""
    bev = opipe.frame_inputs(xyzi, C, *cal)['bev']
    return np.concatenate([np.zeros((PAD, bev.shape[1]), np.uint8), np.any(bev != 0, axis=2).astype(np.uint8)])


def _tile_reach(out, th, tw):
    """[ty, tx] bool: the th x tw tile holds an input-dependent output."""
    h, w = out.shape
    ty, tx = -(-h // th), -(-w // tw)
    p = np.zeros((ty * th, tx * tw), bool)
    p[:h, :w] = out
    return p.reshape(ty, th, tx, tw).any(axis=(1, 3))


def _table(name, frames):
    """The full table of a layer in the extractor's order: {frame, channel tile, y0, x0} on the layer's GEMM grid."""
    th, tw, nt, grouped = TILES[name]
    lvl = {'1': 0, '2': 1, '3': 2, '4': 3}[name[4]] if name.startswith('conv') else \
        {'upconv3': 3, 'pyramid_fusion3': 2, 'upconv2': 2, 'pyramid_fusion2': 1, 'upconv1': 1, 'pyramid_fusion1': 0}[name]
    h, w = (PAD + 700) >> lvl, 800 >> lvl
    ty, tx = -(-h // th), -(-w // tw)
    if grouped:
        return [(f, n, y * th, x * tw) for f in range(frames) for y in range(ty) for x in range(tx) for n in range(nt)]
    return [(f, n, y * th, x * tw) for f in range(frames) for n in range(nt) for y in range(ty) for x in range(tx)]


def _filter(name, items, masks_per_frame):
    """The items whose outputs (th x tw, or 2 th x 2 tw for a transposed conv) hold a bit of their frame's mask."""
    th, tw = TILES[name][:2]
    f = 2 if name.startswith('up') else 1
    reach = [_tile_reach(m[name], f * th, f * tw) for m in masks_per_frame]
    return [it for it in items if reach[it[0]][it[2] // th, it[3] // tw]]


def _check(frame_masks, static_mask, prev_rng=None):
    """Every layer: the host entry's items against numpy's, on the static table of static_mask.  Returns
    {layer: (kept, static items)}."""
    frames = len(frame_masks)
    static = geom.layer_masks(static_mask)
    per_frame = [geom.layer_masks(m) for m in frame_masks]
    counts = {}
    for li, name in enumerate(LAYERS):
        th, tw = TILES[name][:2]
        table = _filter(name, _table(name, frames), [static] * frames)
        want = _filter(name, table, per_frame)
        got = ops.frame_tables_host(np.stack(frame_masks), li, th, tw, np.asarray(table, np.int32))
        assert [tuple(r) for r in got] == want, name
        counts[name] = (len(want), len(table))
        if prev_rng is not None:      # the union with the last forward's items, in table order
            prev = (prev_rng.uniform(size=len(table)) < 0.2).astype(np.uint8)
            keep = set(want)
            union = [it for it, p in zip(table, prev) if p or it in keep]
            got = ops.frame_tables_host(np.stack(frame_masks), li, th, tw, np.asarray(table, np.int32), prev=prev)
            assert [tuple(r) for r in got] == union, name
    return counts


def test_golden_frames():
    g = np.load(os.path.join(GOLDEN, 'frames.npz'))
    names = sorted({k[:-5] for k in g.files if k.endswith('_xyzi')})
    assert names
    for k, name in enumerate(names):
        bp, cal = _calib(g[name + '_p2'], g[name + '_r0'], g[name + '_tr'], g[name + '_imwh'])
        static = ops.bev_support_mask(bp, PAD)
        full = _frame_mask(g[name + '_xyzi'], cal)
        thin = _frame_mask(g[name + '_xyzi'][::4], cal)        # (decimated: a sparser frame in the other slot)
        counts = _check([full, thin], static, np.random.default_rng(k))
        for layer in ('conv1_2', 'conv2_2'):                   # not vacuous: the frames leave most of the wedge out
            kept, table = counts[layer]
            assert 0 < kept < 0.5 * table, (name, layer, kept, table)


def test_synthetic_frames():
    bp, cal = _calib()
    static = ops.bev_support_mask(bp, PAD)
    clouds = [synth.lidar_frame(s, f) for s, f in ((0, 0), (4, 2), (7, 5))]
    masks = [_frame_mask(c, cal) for c in clouds]
    for k, pair in enumerate(((0, 1), (2, 0))):
        counts = _check([masks[i] for i in pair], static, np.random.default_rng(10 + k))
        for layer in ('conv1_2', 'conv2_2'):
            kept, table = counts[layer]
            assert 0 < kept < 0.5 * table, (pair, layer, kept, table)


def test_empty_cloud_keeps_nothing():
    bp, cal = _calib()
    static = ops.bev_support_mask(bp, PAD)
    empty = np.zeros((PAD + 700, 800), np.uint8)       # (the oracle's voxeliser takes no empty cloud: its map is zero)
    counts = _check([empty, _frame_mask(synth.lidar_frame(1, 1), cal)], static)
    assert all(kept > 0 for kept, _ in counts.values())        # (the other slot's frame)
    counts = _check([empty], static)
    assert all(kept == 0 for kept, _ in counts.values())


def test_wedge_filling_cloud_keeps_the_static_table():
    """Every cell the voxeliser can write is non-zero: the per-frame tables are the static ones."""
    bp, _ = _calib()
    static = ops.bev_support_mask(bp, PAD)
    counts = _check([static, static], static, np.random.default_rng(3))
    assert all(kept == table for kept, table in counts.values())


def test_bad_arguments_are_refused():
    items = np.asarray([(0, 0, 0, 0)], np.int32)
    masks = np.zeros((1, 704, 800), np.uint8)
    with pytest.raises(ValueError):
        ops.frame_tables_host(masks, 16, 16, 16, items)
    with pytest.raises(ValueError):
        ops.frame_tables_host(masks, 0, 16, 16, np.asarray([(1, 0, 0, 0)], np.int32))
    with pytest.raises(ValueError):
        ops.frame_tables_host(np.zeros((1, 700, 800), np.uint8), 0, 16, 16, items)
