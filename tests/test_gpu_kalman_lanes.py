"""The Kalman-filter tracker's lanes on the device (dodt_kf_track_lanes, tracking.KalmanTrackerLanes): several videos
side by side, pair i of every step in lane i, each lane with its own state, calibration and ego motion.  The yardstick
is a single KalmanTracker fed the same pairs one track_records call each (tests/test_gpu_kalman.py pins that tracker
to the host module); one scenario is also held against the host module directly.  Synthetic records, no net; the case
bodies are tests/_kind_lanes_cases.py's, shared with the velocity tracker's lanes."""
import numpy as np
import pytest

import _kalman_cases as K
import _kind_lanes_cases as L
from dodt_amd import device
from dodt_amd import tracking as dev

pytestmark = pytest.mark.gpu
KIND = L.kalman()


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_lanes_against_single_trackers(ctx, dtype):
    L.lanes_against_singles(ctx, KIND, dtype)


def test_the_lanes_really_differ(ctx):
    L.lanes_really_differ(ctx, KIND)


def test_follow_scenario_in_lane_1_against_host(ctx):
    """K.follow_scenario() packed into records, in lane 1 of three: the tracks rebuilt from that lane's log are the host
    module's on the encoded keyframe lists, the case fair by the host's own matrices."""
    frames, stride, _ = K.follow_scenario()
    cal = L.cals()[0]
    recs, cnts = L.pack_frames(frames, 'scores')
    lists = L.encoded_lists(ctx, recs, cnts, cal)
    assert [len(x) for x in lists] == [len(f) - 1 for f in frames]       # (the encode drops the score-0.05 box)

    def build():
        return [[{'frame_id': k * stride, 'boxes3d': r[8:15].astype(np.float64), 'boxes2d': r[4:8].astype(np.float64),
                  'scores': float(r[15])} for r in rows] for k, rows in enumerate(lists)]
    frames_h, frames_d = build(), build()
    p = KIND.params
    want, matrices = K.host_run(K.moving, K.CALIB_KITTI, frames_h, stride, 10 ** 6, p['sigma_l'], p['iou_threshold'],
                                min_hits=p['min_hits'])
    K.assert_fair(matrices, p['iou_threshold'])
    assert len(want) == 3
    lanes = L.scenario_in_lane_1(ctx, KIND, recs, cnts, cal, lambda j: K.moving(stride * j, stride * j + stride))
    fin, log = lanes.lane(1).read()
    got = dev.kf_tracks_from_log(fin, log, stride, real_det=lambda k, i: frames_d[k][i])
    K.assert_same_tracks(got, frames_d, want, frames_h)


def test_an_inactive_lane_is_untouched(ctx):
    L.inactive_lane_is_untouched(ctx, KIND)


def test_more_lanes_than_one_chunk(ctx):
    L.more_lanes_than_a_chunk(ctx, KIND)


def test_limits_stay_in_their_lane(ctx):
    L.limits_stay_in_their_lane(ctx, KIND)


def test_the_row_limit_beside_a_lane_of_three(ctx):
    L.row_limit_beside_three(ctx, KIND)


def test_ending_one_lane(ctx):
    L.ending_one_lane(ctx, KIND)


def test_what_the_entries_refuse(ctx):
    L.entry_refusals(ctx, KIND)
