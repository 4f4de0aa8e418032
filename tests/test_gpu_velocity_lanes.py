"""The velocity-extrapolating IoU tracker's lanes on the device (dodt_vt_track_lanes, tracking.VelocityTrackerLanes):
several videos side by side, pair i of every step in lane i, each lane with its own state, calibration and ego motion.
The yardstick is a single VelocityTracker fed the same pairs one track_records call each (tests/test_gpu_velocity_track.py
pins that tracker to the host module); one scenario is also held against the host module directly.  Synthetic records,
no net; the case bodies are tests/_kind_lanes_cases.py's, shared with the Kalman tracker's lanes."""
import numpy as np
import pytest

import _kind_lanes_cases as L
import _velocity_cases as V
from dodt_amd import device
from dodt_amd import tracking as dev

pytestmark = pytest.mark.gpu
KIND = L.velocity()
OBJECTS = [(-6.0, 30.0, 0.02, 0.12, 1.5, 0.9, (0, 1, 2, 4, 5)),        # misses keyframe 3
           (2.0, 24.0, -0.01, 0.08, 1.55, 0.8, (0, 1, 2, 3, 4, 5)),
           (8.0, 40.0, 0.0, 0.1, -1.6, 0.95, (1, 2)),                  # appears late, vanishes for good
           (-1.0, 45.0, 0.0, 0.05, 1.6, 0.3, (0, 1, 2, 3, 4, 5))]      # below sigma_h


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_lanes_against_single_trackers(ctx, dtype):
    L.lanes_against_singles(ctx, KIND, dtype)


def test_the_lanes_really_differ(ctx):
    L.lanes_really_differ(ctx, KIND)


def test_seq_scenario_in_lane_1_against_host(ctx):
    """A V.seq scenario under the moving ego (an object that misses a keyframe, one that vanishes, one below sigma_h)
    packed into records, in lane 1 of three: the tracks rebuilt from that lane's log are the host module's on the encoded
    keyframe lists, the case fair by the host's own IoUs."""
    stride = KIND.params['stride']
    frames, _, frame_num = V.seq(OBJECTS, 6, stride, V.moving, V.CALIB_KITTI)()
    cal = L.cals()[0]
    recs, cnts = L.pack_frames(frames, 'score')
    lists = L.encoded_lists(ctx, recs, cnts, cal)
    assert [len(x) for x in lists] == [len(f) for f in frames]
    frames_h = [[{'frame_id': k * stride, 'info': np.array(['Car', '-1', '-1', '-10.0']),
                  'boxes2d': np.array(r[4:8], np.float32), 'boxes3d': np.array(r[8:15], np.float32),
                  'score': np.float32(r[15])} for r in rows] for k, rows in enumerate(lists)]
    p = {k: v for k, v in KIND.params.items() if k != 'stride'}
    want, groups = V.host_run(V.moving, V.CALIB_KITTI, frames_h, stride, frame_num, **p)
    V.assert_fair(groups, p['sigma_iou'])
    assert len(want) >= 2
    lanes = L.scenario_in_lane_1(ctx, KIND, recs, cnts, cal, lambda j: V.moving(stride * j, stride * j + stride))
    fin, log = lanes.lane(1).read()
    got = dev.vt_tracks_from_log(fin, log, stride, p['extend_len'], frame_num, classes=('Car',))
    V.assert_same_tracks(got, None, want, frames_h)


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
