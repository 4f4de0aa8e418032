"""KITTI calibration files -> config.Calibration (what wavedata's calib_utils.read_calibration /
read_tracking_calibration give the reference, kitti_tracking_utils.py:72-83): the left colour camera's projection and the
two matrices that take a velodyne point into the rectified camera frame.

Two layouts, told apart by their keys alone:
  object    one file per frame:  `P2:`, `R0_rect:`, `Tr_velo_to_cam:`
  tracking  one file per video:  `P2:`, `R_rect`, `Tr_velo_cam` (the devkit's files have no colon behind these two;
            re-exports add one)
The numbers are parsed by float(), so a value is the double nearest to its decimal text.  The image size is not in the
file: it is the shape of the sample's (first) image."""
import numpy as np

from dodt_amd.config import Calibration

_KEYS = {'P2': 'p2', 'R0_rect': 'r0_rect', 'R_rect': 'r0_rect', 'Tr_velo_to_cam': 'tr_velo_to_cam',
         'Tr_velo_cam': 'tr_velo_to_cam'}
_SHAPES = {'p2': (3, 4), 'r0_rect': (3, 3), 'tr_velo_to_cam': (3, 4)}


def parse_calibration(text, image_wh):
    """Calibration from the text of a calibration file of either layout."""
    found = {}
    for line in text.splitlines():
        fields = line.split()
        if not fields:
            continue
        name = _KEYS.get(fields[0][:-1] if fields[0].endswith(':') else fields[0])
        if name is None:
            continue
        if name in found:
            raise ValueError('calibration: %s given twice' % fields[0])
        shape = _SHAPES[name]
        if len(fields) - 1 != shape[0] * shape[1]:
            raise ValueError('calibration: %s has %d numbers, not %d' % (fields[0], len(fields) - 1, shape[0] * shape[1]))
        found[name] = np.array([float(v) for v in fields[1:]], dtype=np.float64).reshape(shape)
    missing = sorted(set(_SHAPES) - set(found))
    if missing:
        raise ValueError('calibration: no %s' % ', '.join(missing))
    return Calibration(found['p2'], found['r0_rect'], found['tr_velo_to_cam'], image_wh)


def read_calibration(path, image_wh):
    """Calibration of the file at `path` (object or tracking layout) for a sample whose images are image_wh = (w, h)."""
    with open(path) as f:
        return parse_calibration(f.read(), image_wh)
