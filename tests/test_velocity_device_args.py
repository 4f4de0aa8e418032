"""What the device velocity tracker's host side refuses and rebuilds without a GPU: the pipeline's tracker arguments, the
ego entries, interpolate_by_track's arguments, and the log -> track dicts reconstruction
(dodt_amd.tracking.vt_tracks_from_log)."""
import numpy as np
import pytest

import _velocity_cases as V
from dodt_amd import config, tracking
from dodt_amd.pipeline import FramePairPipeline

C = config.PYRAMID_DODT
T3 = (np.zeros(3), np.eye(3), 0.0)


def _build(**tracker):
    return FramePairPipeline(None, C, None, None, tracker=tracker)


def test_tracker_arguments_are_refused_up_front():
    with pytest.raises(ValueError, match='lanes'):
        _build(kind='velocity', lanes=True)
    with pytest.raises(ValueError, match='unknown keys'):
        _build(kind='velocity', sigma_l=0.3, iou_threshold=0.5)         # (another tracker's key)
    with pytest.raises(ValueError, match='unknown keys'):
        _build(kind='velocity', max_sequence_dets=100)
    with pytest.raises(ValueError, match='unknown keys'):
        _build(kind='kalman', extend_len=3)
    with pytest.raises(ValueError, match='kind'):
        _build(kind='particle')
    with pytest.raises(ValueError, match='stride'):
        _build(kind='velocity', stride=0)
    with pytest.raises(ValueError, match='extend_len'):
        _build(kind='velocity', extend_len=0)
    with pytest.raises(ValueError, match='log_capacity'):
        _build(kind='velocity', log_capacity=0)
    with pytest.raises(ValueError, match='stride'):                      # (the device loop's bound, refused up front)
        _build(kind='velocity', stride=4097)
    with pytest.raises(ValueError, match='extend_len'):
        _build(kind='velocity', extend_len=4097)


def _bare(sequence=False, pairs=1, velocity=True):
    p = FramePairPipeline.__new__(FramePairPipeline)
    p.kalman, p.velocity, p.sequence, p.pairs = False, velocity, sequence, pairs
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
    _bare(velocity=False, pairs=2)._check_ego([T3[:2], T3])              # any other pipeline: as before


def test_sequence_methods_refuse_frame_ids():
    p = _bare()
    p.tracker = dict(kind='velocity', stride=2, extend_len=3, classes=('Car',))
    with pytest.raises(ValueError, match='frame_ids'):
        p._velocity_tracks([(0, 2)], None)


def test_interpolate_by_track_refusals():
    ego = lambda a, b: T3                                                # noqa: E731
    run = lambda frames, stride=2, extend_len=3: tracking.interpolate_by_track(     # noqa: E731
        ego, V.CALIB_ID, frames, stride, 10, 0.1, 0.5, 0.1, 3, extend_len)
    with pytest.raises(ValueError, match='frame_id'):
        run([[V.det(0, 0, 20)], [V.det(3, 0, 20)]])
    with pytest.raises(ValueError, match='128'):
        run([[V.det(0, i, 20) for i in range(129)]])
    with pytest.raises(ValueError, match='extend_len'):
        run([[V.det(0, 0, 20)]], extend_len=0)
    with pytest.raises(ValueError, match='stride'):
        run([[V.det(0, 0, 20)]], stride=0)
    with pytest.raises(ValueError, match='extend_len'):
        run([[V.det(0, 0, 20)]], extend_len=4097)
    with pytest.raises(ValueError, match='stride'):
        run([[V.det(0, 0, 20)]], stride=4097)
    assert run([]) == []
    rows, counts, box_f64, score_f64 = tracking._vt_check_detections([[V.det(0, 1, 20)], []], 2)
    assert rows.dtype == np.float32 and rows.shape == (2, 1, 16) and list(counts) == [1, 0]
    assert (box_f64, score_f64) == (False, False)
    assert np.array_equal(rows[0, 0, 8:15], V.det(0, 1, 20)['boxes3d']) and rows[0, 0, 15] == np.float32(0.9)
    rows, _, box_f64, score_f64 = tracking._vt_check_detections(
        [[V.det(0, 1, 20), V.det(0, 5, 20, dtype=np.float64)]], 2)
    assert rows.dtype == np.float64 and (box_f64, score_f64) == (True, True)
    # a float64 (or Python float) score beside float32 boxes: float32 arithmetic, float64 comparisons, float64 rows
    mixed = V.det(0, 1, 20)
    mixed['score'] = 0.9
    rows, _, box_f64, score_f64 = tracking._vt_check_detections([[mixed]], 2)
    assert rows.dtype == np.float64 and (box_f64, score_f64) == (False, True) and rows[0, 0, 15] == 0.9
    mixed = V.det(0, 1, 20, dtype=np.float64)
    mixed['score'] = np.float32(0.9)
    assert tracking._vt_check_detections([[mixed]], 2)[2:] == (True, False)


def _log(entries, dtype=np.float32):
    log = np.zeros(len(entries), tracking.VT_LOG)
    for e, (tid, kf, kind, row, x, z, ry) in zip(log, entries):
        e['id'], e['keyframe'], e['kind'], e['row'] = tid, kf, kind, row
        d = V.det(0, x, z, ry=ry, dtype=dtype)
        e['det'][:7], e['det'][7:11], e['det'][11] = d['boxes3d'], d['boxes2d'], d['score']
    return log


def _fin(tid, n_dets, extend_len, flags, speed=(0, 0, 0), max_score=np.float32(0.9)):
    f = np.zeros(1, tracking.VT_TRACK)
    f[0]['id'], f[0]['n_dets'], f[0]['extend_len'], f[0]['flags'] = tid, n_dets, extend_len, flags
    f[0]['speed'], f[0]['max_score'] = speed, max_score
    return f


def test_tracks_are_rebuilt_from_a_log():
    """Track 5 (stride 2): real at keyframes 1 and 2, predicted at frames 5 and 6, in a log that interleaves another
    track; the end extensions run under frame_num."""
    f32 = np.float32
    speed = (f32(0.5) - f32(0.0), f32(31.0) - f32(30.0), f32(1.5) - f32(-1.6))
    log = _log([(5, 1, 0, 1, 0.0, 30.0, -1.6), (7, 1, 0, 0, 9.0, 40.0, 1.5), (5, 2, 0, 0, 0.5, 31.0, 1.5),
                (7, 2, 1, -1, 9.0, 40.0, 1.5), (5, 3, 1, -1, 1.0, 32.0, 4.6), (5, 3, 1, -1, 1.5, 33.0, 7.7)])
    fin = _fin(5, 5, 2, tracking.VT_HAS_SPEED, speed)
    frames = [[], [V.det(2, 9.0, 40.0), V.det(2, 0.0, 30.0, ry=-1.6)], [V.det(4, 0.5, 31.0, score=0.7)]]
    (trk,) = tracking.vt_tracks_from_log(fin, log, 2, 3, 7, real_det=lambda k, i: frames[k][i])
    # extend_track_start: two copies in front (frames 1, 0), moved by -(dets[1] - dets[0]); the end is frame_num - 1
    assert [d['frame_id'] for d in trk['dets']] == [0, 1, 2, 3, 4, 5, 6]
    assert trk['dets'][2] is frames[1][1] and trk['dets'][4] is frames[2][0]
    assert trk['max_score'] == f32(0.9) and trk['extend_len'] == 2 and trk['direction'] == [-1]
    assert np.array_equal(trk['speed'], np.array(speed, f32)) and trk['speed'].dtype == f32
    mid = trk['dets'][3]['boxes3d']                      # interpolate_det: half way, the heading the next one's
    assert np.array_equal(mid[[3, 5]], f32([0.25, 30.5])) and mid[6] == f32(1.5)
    assert np.array_equal(trk['dets'][5]['boxes3d'][[3, 5, 6]], f32([1.0, 32.0, 4.6]))     # the logged x, z, ry
    assert np.array_equal(trk['dets'][6]['boxes2d'], frames[2][0]['boxes2d']) and trk['dets'][6]['score'] == f32(0.7)
    assert np.array_equal(frames[2][0]['boxes3d'], V.det(4, 0.5, 31.0)['boxes3d'])     # the caller's dicts are not written to
    # a record whose predictions were cut loses its last extend_len entries; the end extension follows (frame_num 9)
    cut = _fin(5, 3, 2, tracking.VT_HAS_SPEED | tracking.VT_CUT, speed)
    (trk,) = tracking.vt_tracks_from_log(cut, log, 2, 2, 9, real_det=lambda k, i: frames[k][i])
    assert [d['frame_id'] for d in trk['dets']] == [0, 1, 2, 3, 4, 5, 6]
    assert np.array_equal(trk['dets'][6]['boxes3d'][[3, 5]], f32([1.5, 33.0]))
    # the entry count is the device's: a log that does not give it is an error
    with pytest.raises(RuntimeError, match='entries'):
        tracking.vt_tracks_from_log(_fin(5, 4, 2, 0), log, 2, 3, 7)
    # without real_det the log's own boxes stand in, with 'info' from the class names
    (own,) = tracking.vt_tracks_from_log(fin, log, 2, 3, 7, classes=('Car', 'Van'))
    assert own['dets'][2]['frame_id'] == 2 and np.array_equal(own['dets'][2]['boxes3d'], frames[1][1]['boxes3d'])
    assert list(own['dets'][2]['info']) == ['Car', '-1', '-1', '-10.0'] and own['dets'][2]['boxes3d'].dtype == f32
    # a track that never matched across a gap keeps the list speed
    (still,) = tracking.vt_tracks_from_log(_fin(7, 2, 1, 0), log, 2, 3, 4)
    assert still['speed'] == [0.0, 0.0, 0.0] and [d['frame_id'] for d in still['dets']] == [0, 1, 2, 3]
