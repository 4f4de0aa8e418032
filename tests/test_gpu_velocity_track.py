"""The velocity-extrapolating greedy IoU tracker on the device (dodt_amd/csrc/velocity_track.hip): the association's
IoU matrix and the whole tracker against the host module (dodt_amd.experiments.video_detection_iou), the state carried
across calls, and the limits.

Fairness is asserted on the host's own IoUs: the device's cos / sin may differ from the host's in the last bits of a
double (float64 agreement <= 1e-9, test_gpu_temporal.py's bar), so no IoU may lie within 1e-6 of sigma_iou and every
argmax must win by 1e-6 (or every candidate be exactly 0).  Everything else is compared exactly: track order, frame
ids, which entries are the caller's own dicts, every bit of every box, max_score, speed, extend_len."""
import copy

import numpy as np
import pytest

import _velocity_cases as V
from dodt_amd import device, ops
from dodt_amd import tracking as dev
from dodt_amd.experiments import video_detection_iou as vit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


# ---- 1. the IoU matrix -----------------------------------------------------------------------------------------------
def test_iou_matrix_matches_host(ctx):
    """20 x 20 boxes under a moving ego and KITTI's calibration against cal_transformed_ious, float64: <= 1e-9."""
    rng = np.random.default_rng(5)
    n = 20
    cx, cz = rng.uniform(-10, 10, n), rng.uniform(10, 50, n)
    last = [V.det(0, cx[i], cz[i], ry=rng.uniform(-3, 3), dtype=np.float64) for i in range(n)]
    dets = [V.det(2, cx[i] + rng.normal(0, 0.5), cz[i] + rng.normal(0, 0.5) - 0.6, ry=rng.uniform(-3, 3),
                  dtype=np.float64) for i in rng.permutation(n)]
    for d in last + dets:
        d['boxes3d'][0:3] *= rng.uniform(0.8, 1.2, 3)
        d['boxes3d'][4] += rng.normal(0, 0.2)
    want = np.array([[vit.cal_transformed_ious(V.moving, V.CALIB_KITTI, {'dets': [a]}, b) for b in dets] for a in last])
    back = np.array([[vit.cal_transformed_ious(V.moving, V.CALIB_KITTI, {'dets': [dict(b, frame_id=0)]},
                                               dict(a, frame_id=2)) for b in dets] for a in last])
    d_out = ctx.zeros((n, n), np.float64)
    ops.vt_iou_matrix(ctx, ctx.array(np.array([d['boxes3d'] for d in last])), n,
                      ctx.array(np.array([d['boxes3d'] for d in dets])), n, ops.kf_ego_rows([V.moving(0, 2)])[0],
                      ops.temporal_calib(*V.CALIB_KITTI), d_out)
    got = d_out.download()
    assert np.count_nonzero(want > 0.02) >= n // 2
    assert np.abs(want - back).max() > 0.01                 # (the l/h swap is on the track's side)
    print('IoU matrix: worst difference %.3g' % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-9


# ---- 2. the whole tracker against the host ---------------------------------------------------------------------------
def _both(ctx, ego, calib, build, **params):
    """Host and device on two builds of the same scenario; the host's own IoUs decide whether the case is fair."""
    frames_h, stride, frame_num = build()
    frames_d, _, _ = build()
    p = dict(V.PARAMS, **params)
    want, groups = V.host_run(ego, calib, frames_h, stride, frame_num, **p)
    near, win = V.assert_fair(groups, p['sigma_iou'])
    got = dev.interpolate_by_track(ego, calib, frames_d, stride, frame_num, p['sigma_l'], p['sigma_h'], p['sigma_iou'],
                                   p['t_min'], p['extend_len'], ctx=ctx)
    V.assert_same_tracks(got, frames_d, want, frames_h)
    print('%d tracks, %d argmaxes, nearest IoU to sigma_iou %.3g, smallest contested win %.3g'
          % (len(want), len(groups), near, win))
    return want, frames_h, groups


OBJECTS = [(-6.0, 30.0, 0.02, 0.12, 1.5, 0.9, (0, 1, 2, 4, 5)),        # misses keyframe 3
           (2.0, 24.0, -0.01, 0.08, 1.55, 0.8, (0, 1, 2, 3, 4, 5)),
           (8.0, 40.0, 0.0, 0.1, -1.6, 0.95, (1, 2)),                  # appears late, vanishes for good
           (-1.0, 45.0, 0.0, 0.05, 1.6, 0.3, (0, 1, 2, 3, 4, 5))]      # below sigma_h


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('stride', [1, 2, 3])
@pytest.mark.parametrize('ego', ['parked', 'moving'])
def test_interpolate_by_track_equals_host(ctx, ego, stride, dtype):
    e, cal = (V.PARKED, V.CALIB_ID) if ego == 'parked' else (V.moving, V.CALIB_KITTI)
    want, frames_h, _ = _both(ctx, e, cal, V.seq(OBJECTS, 6, stride, e, cal, dtype))
    assert len(want) >= 2 and all(d['boxes3d'].dtype == dtype for t in want for d in t['dets'])
    assert any(V._where(d, frames_h) is None for t in want for d in t['dets'])      # predictions / interpolations


def test_the_earlier_track_wins_a_contended_detection(ctx):
    """Tracks 0 (x = 0) and 1 (x = 0.6); keyframe 1 brings one detection at x = 0.55: track 1's IoU is the higher one,
    track 0 is asked first and its IoU passes sigma_iou."""
    def build():
        return [[V.det(0, 0.0, 30.0), V.det(0, 0.6, 30.0)], [V.det(2, 0.55, 30.0)], [V.det(4, 0.55, 30.0)]], 2, 5
    want, frames_h, groups = _both(ctx, V.PARKED, V.CALIB_ID, build, t_min=1)
    first = groups[0][0]                                    # track 0 against the one detection of keyframe 1
    lone = vit.cal_transformed_ious(V.PARKED, V.CALIB_ID, {'dets': [frames_h[0][1]]}, frames_h[1][0])
    assert len(groups[0]) == 1 and first > V.PARAMS['sigma_iou'] and lone > first + 0.01
    # track 1 never sees a free detection: it coasts, is cut in keyframe 2 and finishes first, with its one entry
    assert [len(t['dets']) for t in want] == [1, 5]
    assert want[0]['dets'][0] is frames_h[0][1] and want[0]['extend_len'] == 3
    assert want[1]['dets'][0] is frames_h[0][0] and want[1]['dets'][2] is frames_h[1][0]


def test_coast_then_rematch(ctx):
    want, frames_h, _ = _both(ctx, V.PARKED, V.CALIB_ID, V.seq([(0.0, 30.0, 0.05, 0.2, 1.5, 0.9, (0, 1, 3))], 4, 2))
    assert [d['frame_id'] for d in want[0]['dets']] == [0, 1, 2, 3, 4, 5, 6] and want[0]['dets'][6] is frames_h[3][0]


CUT = [(-8.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1)), (0.0, 30.0, 0.0, 0.1, 1.5, 0.9, (1,)),
       (8.0, 30.0, 0.0, 0.1, 1.5, 0.3, (0, 1))]


def test_coast_until_the_cut_in_mid_stride(ctx):
    """Stride 2, extend_len 3 (test_velocity_track.py's case): one track finishes, one is dropped by t_min, one by
    sigma_h; with t_min = 1 two finish, in track order."""
    want, _, _ = _both(ctx, V.PARKED, V.CALIB_ID, V.seq(CUT, 4, 2))
    assert len(want) == 1 and want[0]['extend_len'] == 3 and len(want[0]['dets']) == 5
    want, _, _ = _both(ctx, V.moving, V.CALIB_KITTI, V.seq(CUT, 5, 2, V.moving, V.CALIB_KITTI), t_min=1)
    assert [len(t['dets']) for t in want] == [5, 1]


BELOW = 0.5 - 2.0 ** -26        # half a float32 ulp below sigma_h: float32 rounds it to 0.5


@pytest.mark.parametrize('boxes', [np.float32, np.float64])
def test_float64_scores_are_compared_as_float64(ctx, boxes):
    """Scores just below sigma_h and sigma_l that float32 would round onto them: a track that is cut in mid-sequence
    (the step's finish test), one that lives to the end of the video (the flush's) and a detection at sigma_l, with
    float64 and with float32 boxes beside the float64 scores; the same values as float32 scores pass both thresholds."""
    objs = [(-8.0, 30.0, 0.0, 0.1, 1.5, BELOW, (0, 1)), (0.0, 30.0, 0.0, 0.1, 1.5, BELOW, (0, 1, 2, 3)),
            (8.0, 30.0, 0.0, 0.1, 1.5, 0.9, (0, 1, 2, 3))]

    def build(score_type):
        def make():
            frames, stride, n = V.seq(objs, 4, 2, dtype=boxes)()
            frames[3].append(V.det(6, 14.0, 40.0, dtype=boxes))
            frames[3][-1]['score'] = 0.1 - 2.0 ** -29
            for f in frames:
                for d in f:         # (V.det has rounded a float32 detection's score already)
                    v = BELOW if np.float32(d['score']) == np.float32(0.5) else float(d['score'])
                    d['score'] = score_type(v)
            return frames, stride, n
        return make
    want, _, _ = _both(ctx, V.PARKED, V.CALIB_ID, build(np.float64), t_min=1)
    assert len(want) == 1 and np.float32(want[0]['max_score']) == np.float32(0.9)
    assert want[0]['dets'][0]['boxes3d'].dtype == boxes and isinstance(want[0]['max_score'], np.float64)
    # as float32 the two scores are 0.5: both tracks finish (the cut one first); the late detection opens a track
    want, _, _ = _both(ctx, V.PARKED, V.CALIB_ID, build(np.float32), t_min=1)
    assert len(want) == 3 and [float(t['max_score']) for t in want] == [0.5, 0.5, float(np.float32(0.9))]


A_ = (-5.0, 30.0, 0.02, 0.1, 1.5, 0.9)
B_ = (4.0, 20.0, -0.02, 0.08, 1.5, 0.9)


def test_empty_first_keyframe(ctx):
    want, _, _ = _both(ctx, V.PARKED, V.CALIB_ID, V.seq([A_ + (range(1, 5),), B_ + (range(1, 5),)], 5, 2))
    assert len(want) == 2 and want[0]['dets'][0]['frame_id'] == 0       # (extended backwards)


def test_empty_keyframe_in_the_middle(ctx):
    want, frames_h, _ = _both(ctx, V.moving, V.CALIB_KITTI,
                              V.seq([A_ + ((0, 1, 3, 4),), B_ + ((0, 1, 3, 4),)], 5, 2, V.moving, V.CALIB_KITTI))
    assert len(want) >= 2


def test_one_keyframe(ctx):
    want, _, _ = _both(ctx, V.PARKED, V.CALIB_ID, V.seq([A_ + ((0,),), B_ + ((0,),)], 1, 2), t_min=1)
    assert [len(t['dets']) for t in want] == [1, 1] and list(want[0]['speed']) == [0.0, 0.0, 0.0]


def test_more_tracks_than_detections_and_the_reverse(ctx):
    c = (0.0, 45.0, 0.0, 0.06, 1.5, 0.9)
    d = (9.0, 35.0, 0.02, 0.04, 1.5, 0.9)
    objs = [A_ + ((0, 2, 3),), B_ + ((0, 1, 2, 3),), c + ((0, 1, 2, 3),), d + ((0, 2, 3),),
            (-12.0, 50.0, 0.0, 0.0, 1.5, 0.9, (2, 3)), (14.0, 60.0, 0.0, 0.0, 1.5, 0.9, (2, 3))]
    want, _, _ = _both(ctx, V.moving, V.CALIB_KITTI, V.seq(objs, 4, 2, V.moving, V.CALIB_KITTI), t_min=2)
    assert len(want) == 6


def _grid(k, dz=0.0):
    """128 small boxes, all inside the wedge, no two touching."""
    return [{'frame_id': k, 'info': np.array(V.INFO),
             'boxes3d': np.array([1.0, 0.5, 0.5, -7.5 + (i % 16), 1.6, 30.0 + dz + (i // 16), 0.3], np.float32),
             'boxes2d': np.array([0., 0., 5., 5.], np.float32) + i, 'score': np.float32(0.5 + i / 1000.0)}
            for i in range(128)]


def test_128_detections_in_one_keyframe(ctx):
    def build():
        first = _grid(0)
        second = [copy.deepcopy(first[i]) for i in (100, 3, 57)]
        for s in second:
            s['frame_id'] = 2
            s['boxes3d'][3] += np.float32(0.05)
        return [first, second], 2, 3
    want, frames_h, groups = _both(ctx, V.PARKED, V.CALIB_ID, build, t_min=1)
    assert len(want) == 128 and len(groups) == 101      # (behind track 100 no detection is free)
    assert sorted(i for i, t in enumerate(want) if len(t['dets']) == 3 and t['extend_len'] == 0) == [3, 57, 100]


# ---- 3. the state carried across calls -------------------------------------------------------------------------------
def test_state_is_the_same_however_the_keyframes_are_split(ctx):
    n, stride = 20, 2
    objs = [(-6.0, 30.0, 0.01, 0.05, 1.5, 0.9, tuple(k for k in range(n) if k not in (5, 11, 12))),
            (3.0, 25.0, 0.0, 0.04, 1.5, 0.8, tuple(range(0, 9))),
            (9.0, 40.0, 0.0, 0.03, 1.6, 0.9, tuple(range(6, n)))]
    frames, _, frame_num = V.seq(objs, n, stride, V.moving, V.CALIB_KITTI)()
    rows, counts, _, _ = dev._vt_check_detections(frames, stride)
    assert rows.dtype == np.float32
    egos = [None] + [V.moving(k * stride - stride, k * stride) for k in range(1, n)]
    cal = ops.temporal_calib(*V.CALIB_KITTI)
    results = []
    for split in ([n], [16, 4], [1] * n):
        tr = dev.VelocityTracker(ctx, stride=stride, log_capacity=512, **V.PARAMS)
        at = 0
        for m in split:
            tr.track_keyframes(ctx.array(rows[at:at + m]), ctx.array(counts[at:at + m]), m, rows.shape[1],
                               egos[at:at + m], cal)
            at += m
        before = tr.used_bytes()
        tr.flush(cal)
        fin, log = tr.read()
        results.append((before, tr.used_bytes(), fin, log))
    assert results[0][0][0].view(np.int32)[0] > 0                     # live tracks before the flush
    for other in results[1:]:
        for a, b in zip(results[0][:2], other[:2]):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        assert np.array_equal(results[0][2], other[2]) and np.array_equal(results[0][3], other[3])
    assert len(results[0][2]) >= 3
    want, groups = V.host_run(V.moving, V.CALIB_KITTI, frames, stride, frame_num)
    V.assert_fair(groups, V.PARAMS['sigma_iou'])
    got = dev.vt_tracks_from_log(results[0][2], results[0][3], stride, V.PARAMS['extend_len'], frame_num,
                                 real_det=lambda k, i: frames[k][i])
    V.assert_same_tracks(got, frames, want, frames)


# ---- 4. limits -------------------------------------------------------------------------------------------------------
def test_a_log_capacity_that_is_too_small_raises_and_writes_nothing_outside(ctx):
    rows, counts, _, _ = dev._vt_check_detections([_grid(0), _grid(2)[:5]], 2)
    cal = ops.temporal_calib(*V.CALIB_ID)
    cap, guard = 100, 4096
    nbytes = ops.vt_state_bytes(cap)
    buf = ctx.array(np.full((guard + nbytes + guard,), 0xA5, np.uint8))
    tr = dev.VelocityTracker(ctx, stride=2, log_capacity=cap, d_state=buf.offset(guard, (nbytes,), np.uint8),
                             **V.PARAMS)
    tr.track_keyframes(ctx.array(rows), ctx.array(counts), 2, rows.shape[1], [None, None], cal)
    tr.flush(cal)
    with pytest.raises(RuntimeError, match='log capacity'):
        tr.read()
    h = tr.header()
    assert h['n_log'] > cap and h['log_cap'] == cap
    assert np.all(buf.offset(0, (guard,), np.uint8).download() == 0xA5)
    assert np.all(buf.offset(guard + nbytes, (guard,), np.uint8).download() == 0xA5)
    # with room for everything the same calls read back
    ok = dev.VelocityTracker(ctx, stride=2, log_capacity=1024, **V.PARAMS)
    ok.track_keyframes(ctx.array(rows), ctx.array(counts), 2, rows.shape[1], [None, None], cal)
    ok.flush(cal)
    fin, log = ok.read()
    assert len(log) == 128 + 5 + 2 * 123 and len(fin) == 128


def test_129_detections_are_refused_before_any_launch(ctx):
    with pytest.raises(ValueError, match='128'):
        dev.interpolate_by_track(V.PARKED, V.CALIB_ID, [_grid(0) + _grid(0)[:1]], 2, 1, ctx=ctx, **V.PARAMS)
    with pytest.raises(ValueError, match='extend_len'):
        dev.VelocityTracker(ctx, extend_len=0)
