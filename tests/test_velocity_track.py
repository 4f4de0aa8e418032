"""The velocity-extrapolating greedy IoU tracker on the host (dodt_amd.experiments.video_detection_iou) against runs of
the reference's own functions (tests/golden/velocity_track.npz, made by tests/golden/make_goldens_velocity_track.py), and
hand-built cases for each of its rules."""
import copy
import os

import numpy as np
import pytest

import _velocity_cases as V
from dodt_amd.datasets.kitti import kitti_tracking_utils as ktu
from dodt_amd.experiments import video_detection_iou as vit

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'velocity_track.npz'))
CALIB = (G['r0'], G['tr'])
SIGMA_L, SIGMA_H, SIGMA_IOU, T_MIN, EXTEND = (float(G['params'][0]), float(G['params'][1]), float(G['params'][2]),
                                              int(G['params'][3]), int(G['params'][4]))


def _ego():
    lines = [str(l) for l in G['oxts_lines']]

    def ego(fa, fb):
        return ktu.coordinate_transform(ktu.Oxts(lines[int(fa)]), ktu.Oxts(lines[int(fb)]))
    return ego


# ---- 1. the IoU ------------------------------------------------------------------------------------------------------
def test_iou_3d_matches_reference_and_swaps_l_and_h():
    """Bar: 0.01 absolute, the distance the maker keeps every decision from a threshold (the reference rasterises the
    bases at 1 cm, at most 0.0038 from the exact value over 1 078 calls).  Observed maximum here: 0.0030."""
    a, b = G['iou3d_a'], G['iou3d_b']
    got = np.asarray([vit.iou_3d(a[i], b[i]) for i in range(len(a))])
    back = np.asarray([vit.iou_3d(b[i], a[i]) for i in range(len(a))])
    print('iou_3d: worst difference %.4f' % max(np.abs(got - G['iou3d']).max(), np.abs(back - G['iou3d_swapped']).max()))
    assert np.count_nonzero(G['iou3d'] > 0.05) >= 20
    assert np.abs(got - G['iou3d']).max() <= 0.01 and np.abs(back - G['iou3d_swapped']).max() <= 0.01
    # box 1 enters with l and h swapped: exchanging the arguments changes the value, here and in the reference
    assert np.abs(got - back).max() > 0.01 and np.abs(G['iou3d'] - G['iou3d_swapped']).max() > 0.01
    # identical boxes do not give 1
    assert np.all(got[:4] < 0.5) and np.all(G['iou3d'][:4] < 0.5)
    # the (n, 7) form of the second argument
    assert np.array_equal(vit.iou_3d(a[0], b), np.asarray([vit.iou_3d(a[0], b[i]) for i in range(len(b))]))


def test_cal_transformed_ious_matches_reference():
    """Frames 2 -> 4 of tracking video 0.  Same bar; observed maximum 0.0021."""
    a, c = G['iou3d_a'], G['trans_b']
    ego = _ego()
    got = np.asarray([vit.cal_transformed_ious(ego, CALIB, {'dets': [{'frame_id': 2, 'boxes3d': a[i]}]},
                                               {'frame_id': 4, 'boxes3d': c[i]}) for i in range(len(a))])
    print('cal_transformed_ious: worst difference %.4f' % np.abs(got - G['trans_iou']).max())
    assert np.count_nonzero(G['trans_iou'] > 0) >= 10
    assert np.abs(got - G['trans_iou']).max() <= 0.01
    assert isinstance(got[0], np.float64) and isinstance(
        vit.cal_transformed_ious(ego, CALIB, {'dets': [{'frame_id': 2, 'boxes3d': a[0]}]},
                                 {'frame_id': 4, 'boxes3d': c[0]}), float)


# ---- 2. whole runs ---------------------------------------------------------------------------------------------------
def _frames(table, n_key):
    frames = [[] for _ in range(n_key)]
    serial = {}
    for r in table:
        d = {'video_id': 0, 'frame_id': int(r[2]), 'info': np.array(V.INFO),
             'boxes2d': np.array(r[11:15], dtype=np.float32), 'boxes3d': np.array(r[4:11], dtype=np.float32),
             'score': np.array(r[3], dtype=np.float32)}
        serial[id(d)] = int(r[0])
        frames[int(r[1])].append(d)
    return frames, serial


_RUNS = {}


def _run(stride):
    if stride not in _RUNS:
        frame_num = int(G['s%d_frame_num' % stride])
        frames, serial = _frames(G['s%d_table' % stride], (frame_num - 1) // stride + 1)
        tracks = vit.interpolate_by_track(_ego(), CALIB, frames, stride, frame_num, SIGMA_L, SIGMA_H, SIGMA_IOU,
                                          T_MIN, EXTEND)
        _RUNS[stride] = (tracks, frames, serial)
    return _RUNS[stride]


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_interpolate_by_track_matches_reference(stride):
    """Number and order of tracks, every entry's frame id and real detection, every bit of every box (interpolated,
    predicted and extended entries included), max_score and speed."""
    tracks, frames, serial = _run(stride)
    entries, heads = G['s%d_entries' % stride], G['s%d_heads' % stride]
    assert len(tracks) == len(heads) and len(heads) >= 5
    assert (entries[:, 2] < 0).any() and (entries[:, 2] >= 0).any()
    at = 0
    for t, trk in enumerate(tracks):
        n = int(heads[t, 4])
        assert len(trk['dets']) == n
        want = entries[at:at + n]
        assert np.all(want[:, 0] == t)
        assert [d['frame_id'] for d in trk['dets']] == [int(v) for v in want[:, 1]]
        assert [serial.get(id(d), -1) for d in trk['dets']] == [int(v) for v in want[:, 2]]
        for d, w in zip(trk['dets'], want):
            assert d['boxes3d'].dtype == np.float32 and d['boxes2d'].dtype == np.float32
            assert np.array_equal(d['boxes3d'], w[3:10].astype(np.float32)), (t, d['frame_id'])
            assert np.array_equal(d['boxes2d'], w[10:14].astype(np.float32)), (t, d['frame_id'])
        assert float(trk['max_score']) == heads[t, 0]
        assert np.array_equal(np.asarray(trk['speed'], np.float64), heads[t, 1:4])
        at += n
    assert at == len(entries)


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_convert_trajectory_to_kitti_format_matches_reference(stride):
    rows = vit.convert_trajectory_to_kitti_format(_run(stride)[0])
    want = G['s%d_kitti' % stride]
    assert rows.shape == want.shape and rows.shape[1] == 18
    assert np.array_equal(rows.astype(str), want)


# ---- 3. one rule each ------------------------------------------------------------------------------------------------
def _host(build, **params):
    frames, stride, frame_num = build()
    p = dict(V.PARAMS, **params)
    tracks = vit.interpolate_by_track(V.PARKED, V.CALIB_ID, frames, stride, frame_num, p['sigma_l'], p['sigma_h'],
                                      p['sigma_iou'], p['t_min'], p['extend_len'])
    return tracks, frames


def test_stride_1_keeps_speed_zero_and_coasting_entries_are_copies():
    tracks, frames = _host(V.seq([(0.0, 30.0, 0.0, 0.3, 1.5, 0.9, (0, 1, 3, 4))], 5, 1))
    (trk,) = tracks
    assert [d['frame_id'] for d in trk['dets']] == [0, 1, 2, 3, 4]
    assert list(trk['speed']) == [0.0, 0.0, 0.0] and trk['extend_len'] == 0
    assert trk['dets'][1] is frames[1][0] and trk['dets'][3] is frames[3][0]
    assert trk['dets'][2] is not frames[1][0]
    assert np.array_equal(trk['dets'][2]['boxes3d'], frames[1][0]['boxes3d'])
    assert np.array_equal(trk['dets'][2]['boxes2d'], frames[1][0]['boxes2d'])


def test_the_whole_gaps_displacement_is_added_per_predicted_frame():
    tracks, frames = _host(V.seq([(0.0, 30.0, 0.05, 0.2, 1.5, 0.9, (0, 1, 3))], 4, 2))
    (trk,) = tracks
    assert [d['frame_id'] for d in trk['dets']] == [0, 1, 2, 3, 4, 5, 6]
    a, b = frames[0][0]['boxes3d'], frames[1][0]['boxes3d']
    speed = b[[3, 5, 6]] - a[[3, 5, 6]]                 # float32, of two frames
    assert speed.dtype == np.float32 and abs(float(speed[1]) - 0.4) < 1e-5
    one = b.copy()
    one[[3, 5, 6]] += speed
    two = one.copy()
    two[[3, 5, 6]] += speed
    assert np.array_equal(trk['dets'][3]['boxes3d'], one) and np.array_equal(trk['dets'][4]['boxes3d'], two)
    assert np.array_equal(trk['dets'][4]['boxes2d'], frames[1][0]['boxes2d'])       # (a copy's 2-D box stays)
    assert trk['dets'][6] is frames[3][0] and trk['extend_len'] == 0
    # the match after the coast starts from the last PREDICTION
    assert np.array_equal(trk['speed'], frames[3][0]['boxes3d'][[3, 5, 6]] - two[[3, 5, 6]])
    mid = two.copy()
    mid[3:6] += 1 / 2 * (frames[3][0]['boxes3d'][3:6] - two[3:6])
    mid[6] += 1 / 2 * (frames[3][0]['boxes3d'][6] - two[6])
    assert np.array_equal(trk['dets'][5]['boxes3d'], mid)


def test_headings_of_opposite_sign_take_the_next_ones():
    def build():
        frames, stride, n = V.seq([(0.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1, 2))], 3, 2)()
        frames[1][0]['boxes3d'][6] = np.float32(1.5 - np.pi)
        return frames, stride, n
    tracks, frames = _host(build)
    (trk,) = tracks
    assert trk['dets'][1]['boxes3d'][6] == frames[1][0]['boxes3d'][6]      # +, - : the next one's
    assert trk['dets'][3]['boxes3d'][6] == frames[2][0]['boxes3d'][6]      # -, + : the next one's
    same = _host(V.seq([(0.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1))], 2, 2))[0][0]
    assert same['dets'][1]['boxes3d'][6] == np.float32(1.5)
    tracks, frames = _host(V.seq([(0.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1))], 2, 4))
    frames[1][0]['boxes3d'][6] = np.float32(1.7)            # (after the run: the interpolation read 1.5)
    assert [float(d['boxes3d'][6]) for d in tracks[0]['dets'][:4]] == [1.5] * 4


CUT = [(-8.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1)),           # finishes: 3 entries, 0.9
       (0.0, 30.0, 0.0, 0.1, 1.5, 0.9, (1,)),              # dropped by t_min: 1 entry
       (8.0, 30.0, 0.0, 0.1, 1.5, 0.3, (0, 1))]            # dropped by sigma_h


def test_extend_len_is_reached_in_the_middle_of_a_stride():
    """Stride 2, extend_len 3: keyframe 2 appends two predictions, keyframe 3 one and then cuts all three."""
    tracks, frames = _host(V.seq(CUT, 4, 2))
    (trk,) = tracks
    # [0, 1, 2] after the cut; extend_track_end then adds `stride` entries (without the cut: 6 + 2 entries)
    assert [d['frame_id'] for d in trk['dets']] == [0, 1, 2, 3, 4] and trk['dets'][2] is frames[1][0]
    assert trk['extend_len'] == 3 and trk['dets'][0] is frames[0][0]
    # one keyframe earlier the predictions are still there (and survive the end of the video)
    tracks, frames = _host(V.seq(CUT, 3, 2))
    assert [d['frame_id'] for d in tracks[0]['dets']] == [0, 1, 2, 3, 4] and tracks[0]['extend_len'] == 2
    # (there the second one finishes as well: one detection and two predictions make t_min, and extend_track_start
    #  puts two copies in front of it)
    assert len(tracks) == 2 and [d['frame_id'] for d in tracks[1]['dets']] == [0, 1, 2, 3, 4]
    assert tracks[1]['dets'][2] is frames[1][1]
    # with t_min = 1 the second one finishes too, behind the first (track order), sigma_h still drops the third
    tracks, frames = _host(V.seq(CUT, 4, 2), t_min=1)
    assert [len(t['dets']) for t in tracks] == [5, 1] and tracks[1]['dets'][0] is frames[1][1]


def test_predictions_survive_at_the_end_of_the_video():
    tracks, frames = _host(V.seq([(0.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1, 2))], 4, 2))
    (trk,) = tracks
    assert [d['frame_id'] for d in trk['dets']] == [0, 1, 2, 3, 4, 5, 6] and trk['extend_len'] == 2
    assert trk['dets'][4] is frames[2][0] and np.array_equal(trk['dets'][6]['boxes2d'], frames[2][0]['boxes2d'])


def _traj(first, n, x=0.0, z=30.0, speed=(0.1, 0.5, 0.0)):
    dets = [V.det(first + i, x + 0.1 * i, z + 0.5 * i) for i in range(n)]
    return {'dets': dets, 'direction': [1], 'max_score': np.float32(0.9), 'speed': np.array(speed, np.float32),
            'extend_len': 0}


def test_extend_track_start():
    (t,) = vit.extend_track_start([_traj(2, 3)], 5)
    assert [d['frame_id'] for d in t['dets']] == [0, 1, 2, 3, 4]                        # stops at frame 0
    step = t['dets'][3]['boxes3d'][[3, 5, 6]] - t['dets'][2]['boxes3d'][[3, 5, 6]]
    want = t['dets'][2]['boxes3d'].copy()
    want[[3, 5, 6]] -= step
    assert np.array_equal(t['dets'][1]['boxes3d'], want)
    (t,) = vit.extend_track_start([_traj(7, 3)], 2)
    assert [d['frame_id'] for d in t['dets']] == [5, 6, 7, 8, 9]
    assert len(vit.extend_track_start([_traj(0, 3)], 2)[0]['dets']) == 3                # first_id == 0
    assert len(vit.extend_track_start([_traj(4, 3, x=30.0, z=20.0)], 2)[0]['dets']) == 3    # outside the wedge
    assert len(vit.extend_track_start([_traj(4, 1)], 2)[0]['dets']) == 1                # a single entry


def test_extend_track_end():
    assert len(vit.extend_track_end([_traj(2, 3)], 2, 5)[0]['dets']) == 3               # ends at frame_num - 1
    (t,) = vit.extend_track_end([_traj(2, 3)], 2, 6)
    assert [d['frame_id'] for d in t['dets']] == [2, 3, 4, 5, 6]                        # (no upper bound)
    want = t['dets'][2]['boxes3d'].copy()
    want[[3, 5, 6]] += t['speed']
    assert np.array_equal(t['dets'][3]['boxes3d'], want)
    assert len(vit.extend_track_end([_traj(2, 3, x=30.0, z=20.0)], 2, 9)[0]['dets']) == 3


def test_wedge_and_direction():
    assert vit.inside(V.det(0, 0.0, 30.0)) and not vit.inside(V.det(0, 30.0, 20.0))
    assert not vit.inside(V.det(0, 0.0, 70.0)) and not vit.inside(V.det(0, 0.0, 0.0))
    assert abs(vit.get_boundary_dis(V.det(0, 0.0, 30.0)) - 30 / np.sqrt(2)) < 1e-6
    trk = {'direction': [1, 1, -1]}
    d = V.det(0, 0.0, 30.0, ry=-1.5)
    vit.update_dierection(trk, d)
    assert trk['direction'] == [1, 1, -1, -1] and d['boxes3d'][6] == np.float32(-1.5)    # the sum is 0: negative
    vit.update_dierection({'direction': [1, 1, 1]}, d)
    assert d['boxes3d'][6] == np.float32(1.5)


def test_inputs_are_not_written_to():
    frames, stride, frame_num = V.seq(CUT, 4, 2)()
    before = copy.deepcopy(frames)
    vit.interpolate_by_track(V.PARKED, V.CALIB_ID, frames, stride, frame_num, **V.PARAMS)
    for fa, fb in zip(frames, before):
        assert len(fa) == len(fb)
        for a, b in zip(fa, fb):
            assert np.array_equal(a['boxes3d'], b['boxes3d']) and np.array_equal(a['boxes2d'], b['boxes2d'])
