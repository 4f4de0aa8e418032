"""The device's point path on real clouds at full resolution: dodt_bev_slices -> occupancy bits ->
dodt_anchor_filter -> dodt_project_anchors_f64, chained on the device's own buffers, against what
the reference computed for 12 frames and 4 ego-motion pairs (digests in
tests/golden/all_frames.json, inputs in tests/golden/real_clouds_*.npz;
tests/golden/make_goldens_all_frames.py).  Needs an MI355X.

Every expectation is first tied to the reference: the oracle, run here on the shipped rows, has to
reproduce the record's digests; the device is then compared with the oracle's arrays word by word,
so that a difference names its words and the input rows behind them (tests/_real_clouds.py)."""
import numpy as np
import pytest

import _real_clouds as rc
from dodt_amd import device, ops, synth
from dodt_amd.core import anchor_filter as gpu_anchor_filter
from dodt_amd.core.anchor_generators import grid_anchor_3d_generator as gen

pytestmark = pytest.mark.gpu
C = rc.C
CASES = rc.SHIPPED_FRAMES + rc.SHIPPED_PAIRS
RECORDS = rc.records_by_tag()


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.fixture(scope='module')
def anchors(ctx):
    """The anchor grid, its filter cells, and both on the device (one upload for the module)."""
    boxes = gen.tile_anchors_3d(C['area_extents'], C['anchor_sizes'], C['anchor_stride'],
                                C['ground_plane'])
    a = gen.box_3d_to_anchor(boxes)
    assert np.array_equal(a, rc.anchor_grid())
    cells, nx, nz = gen.anchor_grid_cells(a, C['area_extents'], C['voxel_size'])
    return dict(anchors=a, nx=nx, nz=nz, d_anchors=ctx.array(a), d_cells=ctx.array(cells))


_ORACLE = {}


def _case(tag):
    """Shipped inputs of a frame / pair and the oracle's outputs for them, checked against the
    reference's digests (computed once per tag)."""
    if tag not in _ORACLE:
        g = rc.load_shipped(tag)
        out = rc.oracle_outputs(g['xyzi'], g['r0'], g['tr'], g['p2'], g['imwh'],
                                g.get('trans'), g.get('matrix'))
        rc.check_digests(out, RECORDS[tag])
        _ORACLE[tag] = (g, out)
    return _ORACLE[tag]


def _bev_params(g):
    bp = ops.make_bev_params(C, synth.velo_to_cam(g['r0'], g['tr']), g['p2'], g['imwh'])
    if 'trans' in g:
        bp = ops.with_ego_motion(bp, g['trans'], g['matrix'])
    return bp


def _run_bev(ctx, g, xyzi=None):
    """-> (map (700,800,6) float32, occupancy words (700,25), the device occupancy buffer)."""
    xyzi = g['xyzi'] if xyzi is None else xyzi
    d_out = ctx.empty((700, 800, 6), np.float32)
    d_occ = ctx.empty((700, 25), np.uint32)
    ops.bev_slices(ctx, ctx.array(np.ascontiguousarray(xyzi, dtype=np.float32)), len(xyzi),
                   _bev_params(g), d_out, d_occ)
    assert ops.bev_status(ctx) == 0
    return d_out.download(), d_occ.download(), d_occ


@pytest.mark.parametrize('tag', CASES)
def test_voxeliser_matches_reference(ctx, tag):
    g, want = _case(tag)
    rec = RECORDS[tag]
    assert len(g['xyzi']) == rec['n_subset'] <= 50000
    got, occ, _ = _run_bev(ctx, g)
    rc.compare_bev(got, want['stack'], g)
    rc.compare_occupancy(occ, want['occ'], g)
    assert np.array_equal(occ, gpu_anchor_filter.pack_occupancy(want['occ']))
    # and the same statement in the reference's own terms
    assert rc.bev_digest(got) == (rec['bev_nnz'], rec['bev_sha1'])


@pytest.mark.parametrize('tag', CASES)
def test_anchor_filter_and_projections_on_the_device_occupancy(ctx, anchors, tag):
    """dodt_anchor_filter reads the occupancy words dodt_bev_slices has just written (no golden in
    between), dodt_project_anchors_f64 the indices it kept; all kept rows are compared."""
    g, want = _case(tag)
    rec = RECORDS[tag]
    _, _, d_occ = _run_bev(ctx, g)
    n = len(anchors['anchors'])
    d_keep = ctx.empty((n,), np.int32)
    d_cnt = ctx.zeros((1,), np.int32)
    ops.anchor_filter(ctx, d_occ, anchors['nx'], anchors['nz'], anchors['d_cells'], n, d_keep,
                      d_cnt)
    cnt = int(d_cnt.download()[0])
    want_idx = np.nonzero(want['keep'])[0]
    assert rc.mask_digest(want['keep']) == (rec['anchors_kept'], rec['anchor_sha1'])
    assert cnt == rec['anchors_kept'] == len(want_idx)
    assert np.array_equal(d_keep.download()[:cnt], want_idx)

    d_bev = ctx.empty((cnt, 4), np.float32)
    d_img = ctx.empty((cnt, 4), np.float32)
    d_a32 = ctx.empty((cnt, 6), np.float32)
    ops.project_anchors_f64(ctx, anchors['d_anchors'], d_keep, cnt, d_cnt,
                            C['bev_extents'].reshape(-1), g['p2'], g['imwh'], d_bev, d_img, d_a32)
    assert rc.norm_digest(want['bev_norm']) == rec['bev_norm_sha1']
    assert rc.norm_digest(want['img_norm']) == rec['img_norm_sha1']
    for name, got, ref in (('bev', d_bev.download(), want['bev_norm'][:, [1, 0, 3, 2]]),
                           ('img', d_img.download(), want['img_norm'][:, [1, 0, 3, 2]]),
                           ('anchors', d_a32.download(), want['kept'].astype(np.float32))):
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, '%s: %d of %d values differ, first (kept row, column, got, want): %s' % (
            name, len(bad), ref.size,
            [(int(r), int(c), float(got[r, c]), float(ref[r, c])) for r, c in bad[:10]])

    # the host drop-in on the oracle's grid
    mask = gpu_anchor_filter.get_empty_anchor_filter_2d(
        anchors['anchors'], want['occ'], C['area_extents'], C['voxel_size'], ctx=ctx)
    assert np.array_equal(mask, want['keep'])


@pytest.mark.parametrize('tag', rc.PERMUTED)
def test_point_order_decides_heights_like_the_reference(ctx, tag):
    """Density and occupancy do not depend on the order of the rows; the heights do ("lowest
    y-bin, then lowest original index"), and have to follow the oracle on the permuted rows."""
    g, _ = _case(tag)
    a, occ_a, _ = _run_bev(ctx, g)
    perm = np.random.default_rng(20261016).permutation(len(g['xyzi']))
    xyzi = np.ascontiguousarray(g['xyzi'][perm])
    b, occ_b, _ = _run_bev(ctx, g, xyzi)
    assert np.array_equal(a[:, :, 5], b[:, :, 5])
    assert np.array_equal(occ_a, occ_b)
    assert np.array_equal(a != 0, b != 0)
    want = rc.oracle_outputs(xyzi, g['r0'], g['tr'], g['p2'], g['imwh'])
    assert np.count_nonzero(want['stack'].astype(np.float32) != a) > 100     # the order matters
    rc.compare_bev(b, want['stack'], dict(g, xyzi=xyzi))
    rc.compare_occupancy(occ_b, want['occ'], dict(g, xyzi=xyzi))
