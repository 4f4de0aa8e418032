"""The velocity-extrapolating IoU tracker as the pipeline's opt-in stage (FramePairPipeline(tracker=dict(kind='velocity',
...))): end_sequence() against the host's interpolate_by_track on the keyframe lists of the pipeline's own records, the
records against a pipeline without a tracker, tracks_so_far(), kitti_tracking_rows() and a second sequence.

The pipeline and the sizes are tests/test_gpu_kalman_pipeline.py's: every frame of every step is the same synthetic frame
with the same injected heads, so every keyframe holds the same detections and the (slowly) moving ego alone separates a
track's last box from its detection.  The fairness conditions are asserted on the host's own IoUs all the same."""
import numpy as np
import pytest

import _velocity_cases as V
from dodt_amd import config, device, ops, synth
from dodt_amd.experiments import video_detection_iou as vit
from dodt_amd.pipeline import MAX_DET, REC_COLS, FramePairPipeline

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
STRIDE, N_PAIRS, N_DETS = 2, 4, 12
SIGMA_IOU, T_MIN, EXTEND = 0.1, 2, 3
FRAME_NUM = N_PAIRS * STRIDE + 1


def slow(a, b):
    """A sixth of V.moving: 0.05 m and 1/600 rad per frame (the injected heads' boxes reach 70 m and are small)."""
    trans, _, yaw = V.moving(a, b)
    c, s = np.cos(yaw / 6), np.sin(yaw / 6)
    return trans / 6, np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), yaw / 6


def _ego(j):
    return slow(STRIDE * j, STRIDE * j + STRIDE)


def jumps(a, b):
    """slow, but the two pairs in the middle of the sequence bring a jump of 6 m to the side: no track overlaps any
    detection at keyframes 2 and 3, so every track of keyframes 0 and 1 coasts, is cut at keyframe 3 and finishes in
    mid-sequence."""
    if a in (STRIDE, 2 * STRIDE):
        return np.array([0.0, 6.0, 0.0]), np.eye(3), 0.0
    return slow(a, b)


def _run(pipe, ctx, frame, n_pairs, with_ego=True, ego=slow):
    """n_pairs pairs of the frame through `pipe` -> records (n_pairs, 2, MAX_DET, 17), counts."""
    ring = max(n_pairs, 2)
    rec_ring = ctx.zeros((ring, 1, 2, MAX_DET, REC_COLS), np.float32)
    cnt_ring = ctx.zeros((ring, 1, 2), np.int32)
    pipe.use_record_ring(rec_ring, cnt_ring)
    pipe.test_rings = (rec_ring, cnt_ring)          # (the pipeline writes there until it is given others)
    slots = [(pipe.step_idx + k) % ring for k in range(n_pairs)]    # step k of the pipeline fills slot k % ring
    pts, img, heads = frame
    for k in range(n_pairs):
        pipe.run([pts] * 2, [pts.shape[0]] * 2, [img] * 2, heads=[heads] * 2,
                 ego_motion=[ego(STRIDE * k, STRIDE * k + STRIDE)] if with_ego else None)
    pipe.finish()
    ctx.sync()
    return (rec_ring.download()[slots].reshape(n_pairs, 2, MAX_DET, REC_COLS),
            cnt_ring.download()[slots].reshape(n_pairs, 2))


def _keyframe_lists(ctx, recs, cnts, score_threshold=0.1):
    """The encoded keyframe-0 rows of every pair and the keyframe-1 rows of the last, as interpolate_by_track's
    detections: float32, 'info' from the class column."""
    n = len(recs)
    d_trk, d_k1 = ctx.empty((n, 128, 23), np.float32), ctx.empty((n, 128, 16), np.float32)
    d_cnt = ctx.empty((n, 4), np.int32)
    ops.track_encode(ctx, ctx.array(recs), ctx.array(cnts), n, MAX_DET, config.KITTI_P2, config.KITTI_IMAGE_WH,
                     score_threshold, d_trk, d_k1, d_cnt)
    trk, k1, cnt = d_trk.download(), d_k1.download(), d_cnt.download()
    lists = [trk[j, :cnt[j, 3], :16] for j in range(n)] + [k1[n - 1, :cnt[n - 1, 1]]]
    classes = tuple(C.get('classes', ('Car',)))
    return [[{'frame_id': k * STRIDE, 'info': np.array([classes[int(r[0])], '-1', '-1', '-10.0']),
              'boxes2d': np.array(r[4:8], np.float32), 'boxes3d': np.array(r[8:15], np.float32),
              'score': np.float32(r[15])} for r in rows] for k, rows in enumerate(lists)]


@pytest.fixture(scope='module')
def world():
    ctx = device.default_context()
    kw = dict(rpn_nms_size=1024)
    plain = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), **kw)
    pts = synth.lidar_frame(20, 0)
    frame = (ctx.array(pts), ctx.array(synth.image_frame(20, 0)),
             {k: ctx.array(v) for k, v in synth.head_outputs(20, 0, plain.n_all, plain.P).items()})
    recs, cnts = _run(plain, ctx, frame, N_PAIRS)
    # sigma_l: in the first gap of the first keyframe's sorted scores that leaves at least N_DETS detections -- a dozen
    # or two tracks keep the host's Python loop short; sigma_h the same value: every track that is kept may finish
    scores = np.sort([float(d['score']) for d in _keyframe_lists(ctx, recs, cnts)[0]])[::-1]
    cut = next(i for i in range(N_DETS, len(scores)) if scores[i - 1] > scores[i])
    assert cut <= 40
    sigma_l = float(scores[cut - 1] + scores[cut]) / 2
    tk = dict(kind='velocity', sigma_l=sigma_l, sigma_h=sigma_l, sigma_iou=SIGMA_IOU, t_min=T_MIN, extend_len=EXTEND,
              stride=STRIDE, log_capacity=4096)
    one = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), tracker=tk, reuse_streams_of=plain, **kw)
    yield dict(ctx=ctx, plain=plain, one=one, frame=frame, recs=recs, cnts=cnts, sigma_l=sigma_l)
    for p in (one, plain):
        p.close()


def _params(w):
    return dict(sigma_l=w['sigma_l'], sigma_h=w['sigma_l'], sigma_iou=SIGMA_IOU, t_min=T_MIN, extend_len=EXTEND)


def _expected(w, recs, cnts, ego=slow):
    frames_h = _keyframe_lists(w['ctx'], recs, cnts)
    frame_num = (len(frames_h) - 1) * STRIDE + 1
    want, groups = V.host_run(ego, V.CALIB_KITTI, frames_h, STRIDE, frame_num, **_params(w))
    near, win = V.assert_fair(groups, SIGMA_IOU)
    print('%d keyframes, %d tracks, %d argmaxes, nearest IoU to sigma_iou %.3g, smallest contested win %.3g'
          % (len(frames_h), len(want), len(groups), near, win))
    return want, frames_h


def test_end_sequence_equals_host(world):
    w = world
    recs, cnts = _run(w['one'], w['ctx'], w['frame'], N_PAIRS)
    # the detection records of those steps are what a pipeline without a tracker gives
    assert np.array_equal(recs, w['recs']) and np.array_equal(cnts, w['cnts'])
    want, frames_h = _expected(w, recs, cnts)
    assert len(want) >= N_DETS // 2 and len(frames_h) == N_PAIRS + 1
    # mid-sequence: the tracks finished so far (the last pair's keyframe 1 is not tracked yet) are the host's on the
    # first N_PAIRS keyframes -- here none: every track is still live (test_tracks_so_far_in_mid_sequence has some)
    so_far = w['one'].tracks_so_far()
    want_so_far, _ = V.host_run_so_far(slow, V.CALIB_KITTI, frames_h[:N_PAIRS], STRIDE, **_params(w))
    V.assert_same_tracks(so_far, None, want_so_far, frames_h)
    assert w['one'].track_state.header()['keyframe'] == N_PAIRS
    with pytest.raises(ValueError, match='frame_ids'):
        w['one'].tracks_so_far(frame_ids=[(0, 2)] * N_PAIRS)
    got = w['one'].end_sequence()
    V.assert_same_tracks(got, None, want, frames_h)
    assert all(list(d['info']) == list(x['info']) for g, t in zip(got, want) for d, x in zip(g['dets'], t['dets']))
    # the KITTI rows are the host converter's
    rows = w['one'].kitti_tracking_rows()
    assert rows.shape[1] == 18 and np.array_equal(rows.astype(str),
                                                  vit.convert_trajectory_to_kitti_format(want).astype(str))
    assert np.array_equal(w['one'].kitti_tracking_rows(got[:2]).astype(str),
                          vit.convert_trajectory_to_kitti_format(want[:2]).astype(str))
    # an explicit frame_total is extend_track_end's frame_num; a second sequence starts from id 0, the same tracks
    assert w['one'].track_state.header()['next_id'] == 0 and w['one'].track_state.header()['keyframe'] == 0
    recs2, _ = _run(w['one'], w['ctx'], w['frame'], N_PAIRS)
    assert np.array_equal(recs2, recs)
    again = w['one'].end_sequence(frame_total=FRAME_NUM)
    V.assert_same_tracks(again, None, want, frames_h)


def test_tracks_so_far_in_mid_sequence(world):
    """Two jumps of the ego end every track of the first two keyframes at keyframe 3: tracks_so_far() gives them, as the
    host does on the first N_PAIRS keyframes, and end_sequence() the whole sequence's."""
    w = world
    recs, cnts = _run(w['one'], w['ctx'], w['frame'], N_PAIRS, ego=jumps)
    want, frames_h = _expected(w, recs, cnts, ego=jumps)
    want_so_far, groups = V.host_run_so_far(jumps, V.CALIB_KITTI, frames_h[:N_PAIRS], STRIDE, **_params(w))
    V.assert_fair(groups, SIGMA_IOU)
    assert len(want_so_far) >= N_DETS // 2 and len(want_so_far) < len(want)
    so_far = w['one'].tracks_so_far()
    V.assert_same_tracks(so_far, None, want_so_far, frames_h)
    V.assert_same_tracks(w['one'].end_sequence(), None, want, frames_h)


def test_parked_steps_and_refusals(world):
    w = world
    pts, img, heads = w['frame']
    with pytest.raises(ValueError, match='delta'):      # a 2-tuple: refused before anything is enqueued
        w['one'].run([pts] * 2, [pts.shape[0]] * 2, [img] * 2, heads=[heads] * 2, ego_motion=[_ego(0)[:2]])
    assert w['one'].pending is None
    recs, cnts = _run(w['one'], w['ctx'], w['frame'], 2, with_ego=False)
    want, frames_h = _expected(w, recs, cnts, ego=V.PARKED)
    # a longer video: extend_track_end adds `stride` entries behind every track that ends inside the wedge
    got = w['one'].end_sequence(frame_total=100)
    longer = vit.extend_track_end(want, STRIDE, 100)
    V.assert_same_tracks(got, None, longer, frames_h)
    assert any(t['dets'][-1]['frame_id'] == 2 * STRIDE + STRIDE for t in got)
