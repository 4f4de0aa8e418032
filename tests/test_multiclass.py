"""Configurations with several classes, host side: the people configurations, the per-class anchor grid and its
grid cells against what the reference's own code produced (tests/golden/make_goldens_multiclass.py).  CPU only."""
import hashlib
import os

import numpy as np
import pytest

from dodt_amd import config
from dodt_amd.core.anchor_generators import grid_anchor_3d_generator as gen
from oracle import anchors as oanchors
from oracle import points as opoints

C = config.PYRAMID_DODT


@pytest.fixture(scope='module')
def mc(golden_dir):
    return np.load(os.path.join(golden_dir, 'multiclass.npz'))


@pytest.fixture(scope='module')
def people_boxes(mc):
    return gen.tile_anchors_3d_classes(C['area_extents'], mc['anchor_sizes'], mc['anchor_strides'], C['ground_plane'])


def test_people_configurations():
    for cfg, extractor, dims in ((config.PYRAMID_PEOPLE, 'vgg_pyr', (360, 1200)),
                                 (config.AVOD_PEOPLE, 'vgg', (480, 1590))):
        assert cfg['classes'] == ('Pedestrian', 'Cyclist')
        assert cfg['model'] == 'avod_model' and cfg['frames_per_sample'] == 1
        assert cfg['extractor'] == extractor and cfg['img_dims'] == dims
        assert cfg['rpn_test_nms_size'] == 1024
        assert cfg['voxel_size'] == 0.10000000149011612          # float32-rounded like the car dicts
        assert cfg['height_hi'] == 2.299999952316284
        sizes, strides = config.class_anchor_params(cfg)
        assert len(sizes) == len(strides) == 2
        assert np.asarray(strides).tolist() == [[0.5, 0.5], [0.5, 0.5]]
        boxes = gen.tile_anchors_3d_classes(cfg['area_extents'], sizes, strides, cfg['ground_plane'])
        assert boxes.shape == (89600, 7)
    assert config.AVOD_PEOPLE['img_dims'] == config.CARS_EXAMPLE['img_dims']
    assert config.PYRAMID_DODT['classes'] == config.CARS_EXAMPLE['classes'] == ('Car',)


def test_car_configuration_takes_the_class_path_to_the_same_anchors():
    for cfg in (config.PYRAMID_DODT, config.CARS_EXAMPLE):
        sizes, strides = config.class_anchor_params(cfg)
        assert len(sizes) == 1
        got = gen.tile_anchors_3d_classes(cfg['area_extents'], sizes, strides, cfg['ground_plane'])
        want = gen.tile_anchors_3d(cfg['area_extents'], cfg['anchor_sizes'], cfg['anchor_stride'], cfg['ground_plane'])
        assert got.shape == (89600, 7) and got.dtype == want.dtype
        assert got.tobytes() == want.tobytes()


def test_pair_configuration_with_classes():
    cfg = dict(config.PYRAMID_DODT, classes=('Pedestrian', 'Cyclist'),
               anchor_sizes=config.PYRAMID_PEOPLE['anchor_sizes'], anchor_strides=config.PYRAMID_PEOPLE['anchor_strides'])
    sizes, strides = config.class_anchor_params(cfg)
    assert len(sizes) == 2 and cfg['frames_per_sample'] == 2
    with pytest.raises(ValueError):
        config.class_anchor_params(dict(cfg, classes=('Pedestrian',)))


def test_class_anchor_grid_matches_reference(mc, people_boxes):
    counts = mc['anchor_class_counts']
    assert people_boxes.shape == (int(counts.sum()), 7) == (89600, 7) and people_boxes.dtype == np.float64
    start = 0
    for c, n in enumerate(counts):                                  # class-major
        rows = people_boxes[start:start + n]
        assert np.array_equal(rows[:64], mc['anchor_first64_%d' % c])
        assert np.array_equal(rows[-64:], mc['anchor_last64_%d' % c])
        assert np.array_equal(rows[:, 3:6], np.broadcast_to(mc['anchor_sizes'][c][0], (n, 3)))
        start += n
    sha = hashlib.sha1(np.ascontiguousarray(people_boxes).tobytes()).digest()
    assert sha == mc['anchor_sha1'].tobytes()
    # the oracle's single-class function per class, concatenated: what the GPU pipeline test compares with
    want = np.concatenate([oanchors.tile_anchors_3d(C['area_extents'], s, st, C['ground_plane'])
                           for s, st in zip(mc['anchor_sizes'], mc['anchor_strides'])])
    assert np.array_equal(people_boxes, want)


def test_class_anchor_cells_reproduce_the_reference_filter(mc, people_boxes, golden_dir):
    """anchor_grid_cells of the two-class grid + the oracle's occupancy grid of the bundled cloud = the keep mask of
    the reference's get_empty_anchor_filter_2d: the counts the device kernel takes over [x1, x2) x [z1, z2)."""
    frames = np.load(os.path.join(golden_dir, 'frames.npz'))
    tag = 'obj000001'
    cloud = opoints.lidar_in_camera_view(frames[tag + '_xyzi'], frames[tag + '_r0'], frames[tag + '_tr'],
                                         frames[tag + '_p2'], frames[tag + '_imwh'])
    vox = oanchors.sliced_voxel_grid_2d(cloud, C['ground_plane'], C['area_extents'], C['voxel_size'])
    occ = (np.squeeze(vox.leaf_layout_2d) + 1).astype(np.int64)     # (X, Z)
    anchors = gen.box_3d_to_anchor(people_boxes)
    cells, nx, nz = gen.anchor_grid_cells(anchors, C['area_extents'], C['voxel_size'])
    assert (nx, nz) == occ.shape == (800, 700) and cells.shape == (89600, 4)
    sat = oanchors.summed_area_table(occ)
    x1, z1, x2, z2 = np.clip(cells, 0, [nx, nz, nx, nz]).T
    mask = (sat[x2, z2] + sat[x1, z1] - sat[x2, z1] - sat[x1, z2]) >= 1
    want = np.unpackbits(mc['filter_keep_bits'])[:len(mask)].astype(bool)
    assert np.array_equal(mask, want)
    assert int(mask.sum()) == int(mc['filter_n_kept'])
    n0 = int(mc['anchor_class_counts'][0])
    assert mask[:n0].any() and mask[n0:].any()                      # both classes keep anchors
