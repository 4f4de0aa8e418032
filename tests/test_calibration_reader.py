"""dodt_amd.datasets.kitti.calib.read_calibration on the calibration files the reference's test set bundles (copied as
data to tests/golden/: object frame 000000 and tracking video 0001), against the p2 / r0_rect / tr_velodyne_to_cam the
reference itself read from them (tests/golden/all_frames.json): every number equal.  The bundled tracking file spells
its keys like the object files; the tracking devkit's spelling (`R_rect`, `Tr_velo_cam`, with or without colons) is the
same file with those two keys renamed."""
import os

import numpy as np
import pytest

import _real_clouds as rc
from dodt_amd import config
from dodt_amd.datasets.kitti import calib as kcalib

OBJECT = os.path.join(rc.GOLDEN, 'calib_object_000000.txt')
TRACKING = os.path.join(rc.GOLDEN, 'calib_tracking_0001.txt')
RECORDS = rc.records_by_tag()


def _same(cal, record):
    r0, tr, p2, wh = rc.calib_of(record)
    assert isinstance(cal, config.Calibration)
    for got, want, shape in ((cal.p2, p2, (3, 4)), (cal.r0_rect, r0, (3, 3)), (cal.tr_velo_to_cam, tr, (3, 4))):
        assert got.dtype == np.float64 and got.shape == shape
        assert np.array_equal(got, want)
    assert cal.image_wh == wh and all(isinstance(v, int) for v in cal.image_wh)


def test_object_layout():
    rec = RECORDS['obj000000']
    _same(kcalib.read_calibration(OBJECT, (rec['w'], rec['h'])), rec)


def test_tracking_file_is_the_default_calibration():
    rec = RECORDS['trk0001_000000']
    cal = kcalib.read_calibration(TRACKING, (rec['w'], rec['h']))
    _same(cal, rec)
    assert cal.key() == config.KITTI_CALIBRATION.key()


@pytest.mark.parametrize('r_key, tr_key', [('R_rect', 'Tr_velo_cam'), ('R_rect:', 'Tr_velo_cam:'),
                                           ('R_rect', 'Tr_velo_cam:')])
def test_tracking_layout_keys(tmp_path, r_key, tr_key):
    with open(TRACKING) as f:
        text = f.read()
    assert 'R0_rect:' in text and 'Tr_velo_to_cam:' in text
    path = tmp_path / '0001.txt'
    path.write_text(text.replace('R0_rect:', r_key).replace('Tr_velo_to_cam:', tr_key))
    rec = RECORDS['trk0001_000000']
    _same(kcalib.read_calibration(str(path), (rec['w'], rec['h'])), rec)


def test_calibration_type():
    k = config.KITTI_CALIBRATION
    assert np.array_equal(k.p2, config.KITTI_P2) and np.array_equal(k.r0_rect, config.KITTI_R0_RECT)
    assert np.array_equal(k.tr_velo_to_cam, config.KITTI_TR_VELO_TO_CAM) and k.image_wh == config.KITTI_IMAGE_WH
    same = config.Calibration(k.p2.tolist(), k.r0_rect.copy(), k.tr_velo_to_cam.reshape(-1), [1242.0, 375.0])
    assert same.key() == k.key()
    other = config.Calibration(k.p2, k.r0_rect, k.tr_velo_to_cam, (1241, 376))
    assert other.key() != k.key()
    p2 = k.p2.copy()
    p2[0, 0] = np.nextafter(p2[0, 0], 1e9)
    assert config.Calibration(p2, k.r0_rect, k.tr_velo_to_cam, k.image_wh).key() != k.key()


def test_refusals():
    with open(OBJECT) as f:
        lines = f.read().splitlines()
    with pytest.raises(ValueError):
        kcalib.parse_calibration('\n'.join(l for l in lines if not l.startswith('R0_rect')), (1224, 370))
    with pytest.raises(ValueError):
        kcalib.parse_calibration('\n'.join(lines + [l for l in lines if l.startswith('P2:')]), (1224, 370))
    with pytest.raises(ValueError):
        kcalib.parse_calibration('\n'.join(l[:-20] if l.startswith('P2:') else l for l in lines), (1224, 370))
