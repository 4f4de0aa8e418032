"""The oracle's point path against the reference on EVERY real cloud the reference's tests
bundle -- 63 frames and 42 tau=2 pairs, as digests in tests/golden/all_frames.json
(tests/golden/make_goldens_all_frames.py) -- and the comparison helper the GPU tests share
(tests/_real_clouds.py).  No GPU.

Shipped inputs (12 frames, 4 pairs; "FOV + margin" rows at full resolution) are always checked.
The other clouds are read from the reference's test data when that tree is present
(_real_clouds.REFERENCE_KITTI, or DODT_REFERENCE_KITTI in the environment): calibration, image size
and OXTS lines come from the JSON, only the raw .bin from the tree."""
import os

import numpy as np
import pytest

import _real_clouds as rc
from dodt_amd.datasets.kitti import kitti_tracking_utils as ktu
from oracle import points as opoints

KITTI = rc.REFERENCE_KITTI
DOC = rc.load_records()
FRAMES = {r['tag']: r for r in DOC['frames']}
PAIRS = {r['tag']: r for r in DOC['pairs']}


def _check_transform(rec, trans=None, matrix=None):
    """Oxts + coordinate_transform on the two stored lines give the stored (trans, matrix, delta)
    bit for bit."""
    cur, nxt = (ktu.Oxts(line) for line in rec['oxts_lines'])
    t, m, delta = ktu.coordinate_transform(cur, nxt)
    assert np.array_equal(t, np.array(rec['trans'])), (t.tolist(), rec['trans'])
    assert np.array_equal(m, np.array(rec['matrix'])), (m.tolist(), rec['matrix'])
    assert delta == rec['delta']
    if trans is not None:
        assert np.array_equal(trans, t) and np.array_equal(matrix, m)
    return t, m


def _check_warps_agree(xyzi, trans, matrix):
    a = ktu.point_cloud_transform(xyzi, trans, matrix)
    b = opoints.point_cloud_transform(xyzi, trans, matrix)
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(a[:, 3], xyzi[:, 3])


# ---- the JSON itself -------------------------------------------------------------------------
def test_all_frames_json_is_complete():
    assert len(DOC['frames']) == 63 and len(DOC['pairs']) == 42
    assert len(FRAMES) == 63 and len(PAIRS) == 42                    # tags are unique
    for rec in DOC['frames'] + DOC['pairs']:
        assert rec['oracle_equal'] is True and rec['subset_equal'] is True, rec['tag']
        for key in ('bev_sha1', 'occ_sha1', 'anchor_sha1', 'bev_norm_sha1', 'img_norm_sha1'):
            assert len(rec[key]) == 40, (rec['tag'], key)
        assert rec['n_raw'] >= rec['n_subset'] >= rec['n_fov'] > 10000
        assert np.array(rec['p2']).shape == (3, 4) and np.array(rec['r0_rect']).shape == (3, 3)
        assert np.array(rec['tr_velodyne_to_cam']).shape == (3, 4)
    for rec in DOC['pairs']:
        assert rec['frames'][1] == rec['frames'][0] + 2 == rec['frame']
        # the occupancy / anchor side of a pair is the one of its second frame on its own
        single = FRAMES[rc.frame_tag(rec['split'], rec['video'], rec['frame'])]
        for key in ('occ_sha1', 'anchor_sha1', 'bev_norm_sha1', 'img_norm_sha1'):
            assert rec[key] == single[key], (rec['tag'], key)
        assert rec['n_fov_unwarped'] == single['n_fov']
        assert rec['bev_sha1'] != single['bev_sha1']
        assert 0.5 < np.linalg.norm(rec['trans']) < 2.5


def test_shipped_selection_is_exactly_the_fixed_one():
    index = rc.shipped_index()
    assert sorted(index) == sorted(rc.SHIPPED_FRAMES + rc.SHIPPED_PAIRS)
    assert len(rc.SHIPPED_FRAMES) == 12 and len(rc.SHIPPED_PAIRS) == 4
    for tag, files in index.items():
        assert len(files) == 1, (tag, files)
    by_tag = rc.records_by_tag()
    assert sorted(t for t, r in by_tag.items() if r['shipped']) == sorted(index)
    total = 0
    for path in rc.npz_files():
        total += os.path.getsize(path)
        assert os.path.getsize(path) <= 1 << 20, path
    assert total < 5 * 10 ** 6
    for tag in index:
        g, rec = rc.load_shipped(tag), by_tag[tag]
        r0, tr, p2, imwh = rc.calib_of(rec)
        assert g['xyzi'].dtype == np.float32 and g['xyzi'].shape == (rec['n_subset'], 4)
        assert np.array_equal(g['r0'], r0) and np.array_equal(g['tr'], tr)
        assert np.array_equal(g['p2'], p2) and tuple(g['imwh']) == imwh
        if tag in PAIRS:
            assert [str(s) for s in g['oxts_lines']] == rec['oxts_lines']
            assert np.array_equal(g['trans'], np.array(rec['trans']))
            assert np.array_equal(g['matrix'], np.array(rec['matrix']))


# ---- shipped inputs: never skip --------------------------------------------------------------
@pytest.mark.parametrize('tag', rc.SHIPPED_FRAMES)
def test_oracle_on_shipped_frame(tag):
    g = rc.load_shipped(tag)
    rc.check_digests(rc.oracle_outputs(g['xyzi'], g['r0'], g['tr'], g['p2'], g['imwh']),
                     FRAMES[tag])


@pytest.mark.parametrize('tag', rc.SHIPPED_PAIRS)
def test_oracle_on_shipped_pair(tag):
    g = rc.load_shipped(tag)
    _check_transform(PAIRS[tag], g['trans'], g['matrix'])
    _check_warps_agree(g['xyzi'], g['trans'], g['matrix'])
    rc.check_digests(rc.oracle_outputs(g['xyzi'], g['r0'], g['tr'], g['p2'], g['imwh'],
                                       g['trans'], g['matrix']), PAIRS[tag])


# ---- every bundled cloud, at full size, where the reference's test data is present -------------
def _raw_cloud(rec):
    path = rc.bin_path(KITTI, rec['split'], rec['video'], rec['frame'])
    if not os.path.exists(path):
        pytest.skip('the reference tree is not here: %s' % path)
    xyzi = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
    assert len(xyzi) == rec['n_raw']
    return xyzi


@pytest.mark.parametrize('tag', sorted(FRAMES))
def test_oracle_on_every_bundled_frame(tag):
    rec = FRAMES[tag]
    xyzi = _raw_cloud(rec)
    r0, tr, p2, imwh = rc.calib_of(rec)
    rc.check_digests(rc.oracle_outputs(xyzi, r0, tr, p2, imwh), rec)
    if rec['shipped']:          # what travels is the margin subset of this file, in file order
        assert np.array_equal(rc.load_shipped(tag)['xyzi'],
                              xyzi[rc.margin_mask(xyzi, r0, tr, p2, imwh)])


@pytest.mark.parametrize('tag', sorted(PAIRS))
def test_oracle_on_every_bundled_pair(tag):
    rec = PAIRS[tag]
    xyzi = _raw_cloud(rec)
    r0, tr, p2, imwh = rc.calib_of(rec)
    trans, matrix = _check_transform(rec)
    _check_warps_agree(xyzi, trans, matrix)
    rc.check_digests(rc.oracle_outputs(xyzi, r0, tr, p2, imwh, trans, matrix), rec)
    if rec['shipped']:
        m = rc.margin_mask(xyzi, r0, tr, p2, imwh) | \
            rc.margin_mask(xyzi, r0, tr, p2, imwh, trans, matrix)
        assert np.array_equal(rc.load_shipped(tag)['xyzi'], xyzi[m])


# ---- the comparison can fail -------------------------------------------------------------------
@pytest.fixture(scope='module')
def sample():
    tag = 'obj000006'
    g = rc.load_shipped(tag)
    return tag, g, rc.oracle_outputs(g['xyzi'], g['r0'], g['tr'], g['p2'], g['imwh'])


def test_one_ulp_in_one_height_fails(sample):
    tag, g, out = sample
    rc.check_digests(out, FRAMES[tag])
    rc.compare_bev(out['stack'].astype(np.float32), out['stack'], g)
    r, c, ch = (int(v[len(v) // 2]) for v in np.nonzero(out['stack'][:, :, :5]))
    f32 = out['stack'].astype(np.float32)
    f32[r, c, ch] = np.nextafter(f32[r, c, ch], np.float32(np.inf))
    with pytest.raises(AssertionError, match='bev_sha1'):
        rc.check_digests(dict(out, stack=f32), FRAMES[tag])
    with pytest.raises(AssertionError) as e:
        rc.compare_bev(f32, out['stack'], g)
    msg = str(e.value)
    assert '1 of %d words differ' % FRAMES[tag]['bev_nnz'] in msg
    assert '(row %d, col %d, channel %d)' % (r, c, ch) in msg
    # the message names the input rows of that cell and how close each is to a decision
    assert 'cell x=%d z=%d' % (c, 699 - r) in msg and 'nearest decision' in msg
    assert ' 0 rows' not in msg


def test_one_flipped_occupancy_bit_fails(sample):
    from dodt_amd.core.anchor_filter import pack_occupancy
    tag, g, out = sample
    rc.compare_occupancy(pack_occupancy(out['occ']), out['occ'], g)
    x, z = (int(v[len(v) // 2]) for v in np.nonzero(out['occ']))
    occ = out['occ'].copy()
    occ[x, z] = False
    with pytest.raises(AssertionError, match='occ_sha1'):
        rc.check_digests(dict(out, occ=occ), FRAMES[tag])
    with pytest.raises(AssertionError) as e:
        rc.compare_occupancy(pack_occupancy(occ), out['occ'], g)
    msg = str(e.value)
    assert '1 occupancy bits differ' in msg and '(x %d, z %d): got 0, want 1' % (x, z) in msg
    assert 'cell x=%d z=%d' % (x, z) in msg and ' 0 rows' not in msg


def test_swapping_two_rows_of_one_cell_and_y_bin_fails_on_a_height_only(sample):
    """Two rows that share a cell, a slice and the lowest y-bin of that cell: which one is first
    decides the height, nothing else."""
    tag, g, out = sample
    C = rc.C
    pts, uv = rc.camera_frame(g['xyzi'], g['r0'], g['tr'], g['p2'])
    w, h = (int(v) for v in g['imwh'])
    with np.errstate(invalid='ignore'):
        fov = (pts[:, 2] > 0) & (uv[0] > 0) & (uv[0] < w) & (uv[1] > 0) & (uv[1] < h)
    per = (C['height_hi'] - C['height_lo']) / C['num_slices']
    member = fov & opoints.slice_filter(pts.T, C['area_extents'], C['ground_plane'],
                                        C['height_lo'] + per, C['height_lo'] + 2 * per)
    rows = np.nonzero(member)[0]
    cell = np.floor(pts[rows] / C['voxel_size']).astype(np.int64)
    col = (cell[:, 0] + 400) * 700 + cell[:, 2]
    swap = None
    for k in np.unique(col):
        in_cell = rows[col == k]                       # ascending row index
        yb = cell[col == k, 1]
        low = in_cell[yb == yb.min()]
        if len(low) >= 2 and abs(pts[low[0], 1] - pts[low[1], 1]) > 1e-3:
            swap = (low[0], low[1])
            break
    assert swap is not None
    xyzi = g['xyzi'].copy()
    xyzi[[swap[0], swap[1]]] = xyzi[[swap[1], swap[0]]]
    got = rc.oracle_outputs(xyzi, g['r0'], g['tr'], g['p2'], g['imwh'])
    assert np.array_equal(got['stack'][:, :, 5], out['stack'][:, :, 5])
    assert np.array_equal(got['occ'], out['occ']) and np.array_equal(got['keep'], out['keep'])
    with pytest.raises(AssertionError, match='bev_sha1'):
        rc.check_digests(got, FRAMES[tag])
    with pytest.raises(AssertionError) as e:
        rc.compare_bev(got['stack'].astype(np.float32), out['stack'], g)
    assert 'per channel [0, 1, 0, 0, 0, 0]' in str(e.value)
    assert 'row %d xyz' % swap[0] in str(e.value) and 'row %d xyz' % swap[1] in str(e.value)
