"""Shared by tests/test_pipeline_geometry_trace.py and tests/test_bev_support_union.py: the stand-ins of
tests/_pipeline_trace.py, extended (by subclassing, the module itself is left alone) so that every launch that takes a
geometry argument shows WHICH calibration it was given, and the three real calibrations of tests/golden/all_frames.json."""
import types

import numpy as np

import _pipeline_trace as tr
import _real_clouds as rc
from dodt_amd import config
from dodt_amd import pipeline as pl


def real_calibrations():
    """A: the default (tracking video 0001, 1242 x 375), B: object frame 000006 (1238 x 374), C: object frame 000000
    (1224 x 370)."""
    out = []
    for tag in ('trk0001_000000', 'obj000006', 'obj000000'):
        r0, trm, p2, wh = rc.calib_of(rc.records_by_tag()[tag])
        out.append(config.Calibration(p2, r0, trm, wh))
    assert out[0].key() == config.KITTI_CALIBRATION.key()
    assert len({c.key() for c in out}) == 3 and len({c.image_wh for c in out}) == 3
    return out


def tag_of(calib):
    """What names a calibration in a logged launch: its focal length and translation, and its image size."""
    return (float(calib.p2[0, 0]), float(calib.tr_velo_to_cam[0, 3]), tuple(calib.image_wh))


class GeomOps(tr.Ops):
    """The bev parameters carry the tag of the calibration they were made from; M's 42 doubles are that calibration's
    translation 42 times."""

    def make_bev_params(self, cfg, velo_to_cam=None, p2=None, im_wh=None, **k):
        return types.SimpleNamespace(point_format=0, p2=np.array(p2, dtype=np.float64), im_wh=tuple(im_wh),
                                     velo_to_cam=np.array(velo_to_cam, dtype=np.float64))

    def with_ego_motion(self, bp, trans, matrix):
        return types.SimpleNamespace(**dict(vars(bp), ego_motion=True))

    def temporal_calib(self, r0_rect, tr_velo_to_cam):
        return np.full(42, float(np.asarray(tr_velo_to_cam)[0, 3]))


class GeomTracker(tr.Tracker):
    def track_records(self, d_records, d_counts, n_pairs, max_det, p2, image_wh, ctx=None):
        (ctx or self.ctx).log('track_records', [self.d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh])


def install(monkeypatch, ops=None):
    """tr.install() with the stand-ins above on top; uploads are kept with the length the trace had when they were
    made.  -> (build, uploads)."""
    build = tr.install(monkeypatch)
    monkeypatch.setattr(pl, 'ops', ops or GeomOps())
    monkeypatch.setattr(pl.tracking, 'Tracker', GeomTracker)
    uploads = []
    plain = tr.Array.upload

    def upload(self, host):
        owner = self.base.owner
        uploads.append((len(owner.trace) if owner is not None else -1, self.base, np.array(host)))
        return plain(self, host)
    monkeypatch.setattr(tr.Array, 'upload', upload)
    return build, uploads


def bp_matches(bp, calib):
    return (np.array_equal(bp.p2, calib.p2) and tuple(bp.im_wh) == tuple(calib.image_wh)
            and np.array_equal(bp.velo_to_cam, config.velo_to_cam(calib.r0_rect, calib.tr_velo_to_cam)))


def frame(pipe, calib):
    """One frame's (points, n_points, image) for a sample of `calib`: fresh arrays, the image of that sample's size."""
    w, h = calib.image_wh
    return tr.Array((pipe.n_points_max, 4)), 30000, tr.Array((h, w, 3), np.uint8)
