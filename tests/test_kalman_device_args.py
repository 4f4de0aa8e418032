"""What the device Kalman tracker's host side refuses and rebuilds without a GPU: the pipeline's tracker arguments, the
ego entries, kf_pipeline's frame ids, and the log -> Tracker reconstruction (dodt_amd.tracking.kf_tracks_from_log)."""
import numpy as np
import pytest

from dodt_amd import config, ops, tracking
from dodt_amd.pipeline import FramePairPipeline

C = config.PYRAMID_DODT
T3 = (np.zeros(3), np.eye(3), 0.0)


def _build(**tracker):
    return FramePairPipeline(None, C, None, None, tracker=tracker)


def test_tracker_arguments_are_refused_up_front():
    with pytest.raises(ValueError, match='lanes'):
        _build(kind='kalman', lanes=True)
    with pytest.raises(ValueError, match='unknown keys'):
        _build(kind='kalman', sigma_l=0.3, high_threshold=0.5)          # (an IoU tracker's key)
    with pytest.raises(ValueError, match='unknown keys'):
        _build(kind='kalman', sigma=0.3)
    with pytest.raises(ValueError, match='unknown keys'):
        _build(sigma_l=0.3)                                              # (kind defaults to 'iou')
    with pytest.raises(ValueError, match='kind'):
        _build(kind='particle')
    with pytest.raises(ValueError, match='stride'):
        _build(kind='kalman', stride=0)


def _bare(sequence=False, pairs=1, kalman=True):
    p = FramePairPipeline.__new__(FramePairPipeline)
    p.kalman, p.sequence, p.pairs = kalman, sequence, pairs
    return p


def test_ego_entries_need_the_yaw_delta():
    p = _bare(pairs=2)
    p._check_ego(None, None)
    p._check_ego([T3, None], [None, T3])
    with pytest.raises(ValueError, match='delta'):
        p._check_ego([T3, T3[:2]])
    with pytest.raises(ValueError, match='delta'):
        p._check_ego(None, [T3[:2], None])                               # (the look-ahead's)
    with pytest.raises(ValueError, match='one entry per pair'):
        p._check_ego([T3])
    with pytest.raises(ValueError, match='delta'):
        _bare(sequence=True)._check_ego([T3[:2]])
    _bare(kalman=False, pairs=2)._check_ego([T3[:2], T3])                # any other pipeline: as before


def _det(frame, x, z, score=0.9):
    return {'frame_id': frame, 'boxes3d': np.array([1.5, 1.6, 4.0, x, 1.6, z, 0.1]),
            'boxes2d': np.array([0., 0., 10., 10.]) + x, 'scores': score}


def test_kf_pipeline_refuses_a_bad_frame_id_and_too_many_rows():
    ego = lambda a, b: T3                                                # noqa: E731
    calib = (np.eye(3), np.hstack([np.eye(3), np.zeros((3, 1))]))
    with pytest.raises(ValueError, match='frame_id'):
        tracking.kf_pipeline(ego, calib, [[_det(0, 0, 20)], [_det(3, 0, 20)]], 2, 4, 0.3, 0.1)
    with pytest.raises(ValueError, match='128'):
        tracking.kf_pipeline(ego, calib, [[_det(0, i, 20) for i in range(129)]], 2, 2, 0.3, 0.1)
    assert tracking.kf_pipeline(ego, calib, [], 2, 0, 0.3, 0.1) == []


def test_ego_rows():
    rows = ops.kf_ego_rows([None, (np.array([1., 2., 3.]), np.arange(9.).reshape(3, 3), 0.5)])
    assert rows.shape == (2, 13)
    assert np.array_equal(rows[0], [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0])
    assert np.array_equal(rows[1], [1, 2, 3] + list(range(9)) + [0.5])


def _log(entries):
    log = np.zeros(len(entries), tracking.KF_LOG)
    for e, (tid, kf, kind, row, box) in zip(log, entries):
        e['id'], e['keyframe'], e['kind'], e['row'] = tid, kf, kind, row
        e['det'][:7] = box
        e['det'][7:11] = [0, 0, 10, 10]
        e['det'][11] = 0.9
    return log


def test_tracks_are_rebuilt_from_a_log():
    """Track 5: real at keyframes 0 and 1, coasting at 2 and 3 (stride 4, 12 frames: the last virtual detection is
    clamped to frame 11), in a log that interleaves another track."""
    box = lambda x, z: [1.5, 1.6, 4.0, x, 1.6, z, 0.1]                   # noqa: E731
    log = _log([(5, 0, 0, 1, box(0, 20)), (7, 0, 0, 0, box(9, 40)), (5, 1, 0, 0, box(4, 28)), (7, 1, 1, -1, box(9, 41)),
                (5, 2, 1, -1, box(8, 36)), (5, 3, 1, -1, box(12, 44))])
    fin = np.zeros(1, tracking.KF_TRACK)
    fin[0]['id'], fin[0]['hits'], fin[0]['no_losses'] = 5, 1, 2
    fin[0]['x'] = np.arange(8.0)
    fin[0]['P'] = np.arange(16.0).reshape(4, 2, 2)
    frames = [[_det(0, 9, 40), _det(0, 0, 20)], [_det(4, 4, 28)]]
    (trk,) = tracking.kf_tracks_from_log(fin, log, 4, frame_total=12, real_det=lambda k, i: frames[k][i])
    assert (trk.id, trk.hits, trk.no_losses) == (5, 1, 2)
    assert trk.x_state.shape == (8, 1) and np.array_equal(trk.x_state[:, 0], np.arange(8.0))
    assert trk.box == [0.0, 2.0, 4.0, 6.0]
    want_p = np.zeros((8, 8))
    for b in range(4):
        want_p[2 * b:2 * b + 2, 2 * b:2 * b + 2] = np.arange(16.0).reshape(4, 2, 2)[b]
    assert np.array_equal(trk.P, want_p)
    assert [d['frame_id'] for d in trk.dets] == list(range(0, 12))
    assert trk.dets[0] is frames[0][1] and trk.dets[4] is frames[1][0]
    assert [bool(d.get('is_virtual')) for d in trk.dets] == [False] + [True] * 3 + [False] + [True] * 7
    # between two keyframes: the last real one plus ONE increment of (difference / stride)
    assert np.allclose(trk.dets[2]['boxes3d'][[3, 5]], [1.0, 22.0])
    # a coasting entry: a copy of the entry before it at the logged position
    assert np.array_equal(trk.dets[8]['boxes3d'], box(8, 36)) and trk.dets[8]['scores'] == 0.9
    assert np.array_equal(trk.dets[11]['boxes3d'], box(12, 44)) and trk.dets[11]['frame_id'] == 11
    assert np.array_equal(frames[1][0]['boxes3d'], box(4, 28))          # the caller's dicts are not written to
    # without real_det the log's own boxes stand in
    (own,) = tracking.kf_tracks_from_log(fin, log, 4)
    assert [d['frame_id'] for d in own.dets] == list(range(0, 13))
    assert np.array_equal(own.dets[4]['boxes3d'], box(4, 28)) and own.dets[4]['frame_id'] == 4
