"""dodt_bev_support_mask (host only): the BEV cells the voxeliser can ever write, which the fp32 BEV net's skip tables
rest on.  Every non-zero cell of the oracle's BEV maps must lie inside it -- real clouds, edge-case clouds, points on
the frustum's side planes, an ego-motion frame -- and its propagation through the net gives the share of each
layer's output tiles that no input reaches."""
import os

import numpy as np
import pytest

from dodt_amd import config, ops, synth
from oracle import pipeline as opipe

C = config.PYRAMID_DODT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PAD = 4


def _calib(p2=synth.P2, r0=synth.R0_RECT, tr=synth.TR_VELO_TO_CAM, imwh=synth.IMAGE_WH):
    p2, r0, tr = (np.asarray(a, np.float64) for a in (p2, r0, tr))
    bp = ops.make_bev_params(C, config.velo_to_cam(r0, tr), p2, tuple(imwh))
    return bp, (r0, tr, p2, tuple(imwh))


def _numpy_mask(p2, imwh):
    """The same rule restated: u at the 8 corners of each cell's box, w <= 0 counts as reachable, origin cell, margin."""
    vs = C['voxel_size']
    ext = np.asarray(C['area_extents'], np.float64)
    minx, maxx = np.floor(ext[0, 0] / vs), np.ceil(ext[0, 1] / vs - 1)
    minz, maxz = np.floor(ext[2, 0] / vs), np.ceil(ext[2, 1] / vs - 1)
    X, Z = int(maxx - minx + 1), int(maxz - minz + 1)
    xs = (np.arange(X) + minx) * vs
    zs = (np.arange(Z) + minz) * vs
    reach = np.zeros((Z, X), bool)
    umin = np.full((Z, X), np.inf)
    umax = np.full((Z, X), -np.inf)
    for dx in (0, vs):
        for y in ext[1]:
            for dz in (0, vs):
                x, z = xs[None, :] + dx, zs[:, None] + dz
                w = p2[2, 0] * x + p2[2, 1] * y + p2[2, 2] * z + p2[2, 3]
                u = (p2[0, 0] * x + p2[0, 1] * y + p2[0, 2] * z + p2[0, 3]) / np.where(w > 0, w, 1.0)
                reach |= ~(w > 0)
                umin, umax = np.minimum(umin, u), np.maximum(umax, u)
    cell = reach | ((umax > 0) & (umin < imwh[0]))
    cell[-int(minz), -int(minx)] = True           # (z index 0 - minz, x index 0 - minx)
    cell = cell[::-1]                             # row Z-1-z
    p = np.pad(cell, 1)
    out = np.zeros_like(cell)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + Z, dx:dx + X]
    return np.concatenate([np.zeros((PAD, X), np.uint8), out.astype(np.uint8)])


def _assert_inside(bev, mask):
    nz = np.any(bev != 0, axis=2)
    assert nz.shape == mask[PAD:].shape
    outside = nz & (mask[PAD:] == 0)
    assert not outside.any(), np.argwhere(outside)[:10]
    return int(nz.sum())


def _to_velo(cam, r0, tr):
    """(3, N) rectified camera frame -> (N, 4) float32 velodyne xyzi."""
    m = config.velo_to_cam(r0, tr).reshape(3, 4)
    v = np.linalg.solve(m[:, :3], np.asarray(cam, np.float64) - m[:, 3:4]).T
    return np.concatenate([v, np.full((len(v), 1), 0.5)], axis=1).astype(np.float32)


def test_mask_matches_numpy_restatement_and_geometry():
    bp, (r0, tr, p2, imwh) = _calib()
    m = ops.bev_support_mask(bp, PAD)
    assert m.shape == (PAD + 700, 800) and m.dtype == np.uint8
    assert np.array_equal(m, _numpy_mask(p2, imwh))
    assert not m[:PAD].any()
    # the two near-range triangles outside the camera wedge: a third of the map
    assert 0.32 < 1.0 - m[PAD:].mean() < 0.335
    g = np.load(os.path.join(GOLDEN, 'frames.npz'))
    for name in sorted({k[:-5] for k in g.files if k.endswith('_xyzi')}):
        bp, (r0, tr, p2, imwh) = _calib(g[name + '_p2'], g[name + '_r0'], g[name + '_tr'], g[name + '_imwh'])
        assert np.array_equal(ops.bev_support_mask(bp, PAD), _numpy_mask(p2, imwh)), name


def test_camera_frame_points_are_refused():
    from dodt_amd import _lib
    bp, _ = _calib()
    bp.point_format = _lib.PTS_CAM_3XN
    with pytest.raises(ValueError, match='frustum'):
        ops.bev_support_mask(bp, PAD)


def test_oracle_bev_lies_inside_the_mask_real_and_synthetic_clouds():
    g = np.load(os.path.join(GOLDEN, 'frames.npz'))
    for name in sorted({k[:-5] for k in g.files if k.endswith('_xyzi')}):
        bp, cal = _calib(g[name + '_p2'], g[name + '_r0'], g[name + '_tr'], g[name + '_imwh'])
        bev = opipe.frame_inputs(g[name + '_xyzi'], C, *cal)['bev']
        assert _assert_inside(bev, ops.bev_support_mask(bp, PAD)) > 1000, name
    bp, cal = _calib()
    mask = ops.bev_support_mask(bp, PAD)
    for seq, f in ((0, 0), (3, 2), (7, 5)):
        assert _assert_inside(opipe.frame_inputs(synth.lidar_frame(seq, f), C, *cal)['bev'], mask) > 1000


def test_oracle_bev_lies_inside_the_mask_ego_motion_frame():
    e = np.load(os.path.join(GOLDEN, 'egomotion.npz'))
    bp, cal = _calib(e['p2'], e['r0'], e['tr'], e['imwh'])
    bev = opipe.frame_inputs(e['xyzi'], C, *cal, ego_motion=(e['trans'], e['matrix']))['bev']
    assert _assert_inside(bev, ops.bev_support_mask(bp, PAD)) > 1000


def test_oracle_bev_lies_inside_the_mask_edge_clouds():
    """The edge-case clouds (extent edges, one point per slice, ties, dense random), carried to the velodyne frame
    so that the frustum filter sees them."""
    bp, cal = _calib()
    mask = ops.bev_support_mask(bp, PAD)
    d = np.load(os.path.join(GOLDEN, 'edge_clouds.npz'))
    for k in [k for k in d.files if k.endswith('_cloud')]:
        _assert_inside(opipe.frame_inputs(_to_velo(d[k], cal[0], cal[1]), C, *cal)['bev'], mask)


def test_oracle_bev_lies_inside_the_mask_wedge_boundary():
    """Points on the frustum's side planes (u = 0 and u = im_w, just inside and exactly on them), near and far,
    low and high, where the kept wedge meets the input-independent triangles."""
    bp, (r0, tr, p2, imwh) = _calib()
    mask = ops.bev_support_mask(bp, PAD)
    assert p2[2, 0] == 0 and p2[2, 1] == 0       # (KITTI's P2: w = z + p2[2, 3], u independent of y)
    pts = []
    for z in np.linspace(0.3, 69.9, 400):
        w = p2[2, 2] * z + p2[2, 3]
        for v in (1.0, imwh[1] / 2, imwh[1] - 1.0):
            y = (v * w - p2[1, 2] * z - p2[1, 3]) / p2[1, 1]
            if not -4.99 < y < 2.99:
                continue
            for u in (1e-9, 1e-6, 0.5, imwh[0] - 0.5, imwh[0] - 1e-6, imwh[0] - 1e-9, 0.0, float(imwh[0])):
                x = (u * w - p2[0, 1] * y - p2[0, 2] * z - p2[0, 3]) / p2[0, 0]
                pts.append((x, y, z))
    bev = opipe.frame_inputs(_to_velo(np.asarray(pts).T, r0, tr), C, r0, tr, p2, imwh)['bev']
    assert _assert_inside(bev, mask) > 500


def _dilate(m, r):
    h, w = m.shape
    p = np.pad(m, r)
    o = np.zeros_like(m)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            o |= p[dy:dy + h, dx:dx + w]
    return o


def _pool(m):
    h, w = m.shape[0] // 2, m.shape[1] // 2
    m = m[:2 * h, :2 * w]
    return m[0::2, 0::2] | m[0::2, 1::2] | m[1::2, 0::2] | m[1::2, 1::2]


def _up(m):
    return _dilate(np.repeat(np.repeat(m, 2, 0), 2, 1), 2)


def _independent_tiles(out, t):
    h, w = out.shape
    ty, tx = -(-h // t), -(-w // t)
    p = np.zeros((ty * t, tx * t), bool)
    p[:h, :w] = out
    return 1.0 - p.reshape(ty, t, tx, t).any(axis=(1, 3)).mean()


def layer_masks(mask):
    """The mask through the net's geometry: 3x3 convs dilate by 1, pools OR 2x2 windows, upconvs dilate by 2 at the
    output resolution, concat ORs.  Each layer's outputs that may depend on the input, at its output resolution."""
    x = np.asarray(mask).astype(bool)
    L = {}
    L['conv1_1'] = a = _dilate(x, 1)
    L['conv1_2'] = c12 = _dilate(a, 1)
    L['conv2_1'] = a = _dilate(_pool(c12), 1)
    L['conv2_2'] = c22 = _dilate(a, 1)
    L['conv3_1'] = a = _dilate(_pool(c22), 1)
    L['conv3_2'] = a = _dilate(a, 1)
    L['conv3_3'] = c33 = _dilate(a, 1)
    L['conv4_1'] = a = _dilate(_pool(c33), 1)
    L['conv4_2'] = a = _dilate(a, 1)
    L['conv4_3'] = c43 = _dilate(a, 1)
    L['upconv3'] = u3 = _up(c43)
    L['pyramid_fusion3'] = f3 = _dilate(c33 | u3, 1)
    L['upconv2'] = u2 = _up(f3)
    L['pyramid_fusion2'] = f2 = _dilate(c22 | u2, 1)
    L['upconv1'] = u1 = _up(f2)
    L['pyramid_fusion1'] = _dilate(c12 | u1, 1)
    return L


def tiles_reached(out, th, tw):
    """(tiles with an input-dependent output, all tiles) of a th x tw tiling of a layer's outputs."""
    h, w = out.shape
    ty, tx = -(-h // th), -(-w // tw)
    p = np.zeros((ty * th, tx * tw), bool)
    p[:h, :w] = out
    return int(p.reshape(ty, th, tx, tw).any(axis=(1, 3)).sum()), ty * tx


def test_layer_table():
    """Share of 16x16 output tiles (32x32 for upconvs) that no input reaches, in %."""
    bp, _ = _calib()
    L = layer_masks(ops.bev_support_mask(bp, PAD))
    got = {k: int(round(100 * _independent_tiles(v, 32 if k.startswith('up') else 16))) for k, v in L.items()}
    assert got == dict(conv1_1=30, conv1_2=30, conv2_1=27, conv2_2=26, conv3_1=22, conv3_2=21, conv3_3=20,
                       conv4_1=21, conv4_2=19, conv4_3=17, upconv3=12, pyramid_fusion3=13, upconv2=13,
                       pyramid_fusion2=12, upconv1=12, pyramid_fusion1=14)
