"""The Kalman-filter tracker as the pipeline's opt-in stage (FramePairPipeline(tracker=dict(kind='kalman', ...))):
end_sequence() against tracking.kf_pipeline and the host's kf_pipeline on the keyframe lists of the pipeline's own
records, the records against a pipeline without a tracker, a second sequence, and pairs_per_step = 2.

Every frame of every step is the same synthetic frame with the same injected heads, so every keyframe holds the same
detections and the (slowly) moving ego alone separates a track's last box from its detection: the IoU matrices are
dominated by their diagonal, which is what makes the optimum unique -- asserted on the host's own matrices all the
same."""
import numpy as np
import pytest

import _kalman_cases as K
from dodt_amd import config, device, ops, synth
from dodt_amd import tracking as dev
from dodt_amd.pipeline import MAX_DET, REC_COLS, FramePairPipeline

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
STRIDE, N_PAIRS, N_DETS = 2, 4, 12
GATE, MIN_HITS = 0.1, 2


def slow(a, b):
    """A sixth of K.moving: 0.05 m and 1/600 rad per frame.  The injected heads' boxes reach 70 m and are as small as
    they come; under K.moving some of them leave their own track's box from one keyframe to the next, and a track
    without any overlap makes the optimum ambiguous."""
    trans, _, yaw = K.moving(a, b)
    c, s = np.cos(yaw / 6), np.sin(yaw / 6)
    return trans / 6, np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), yaw / 6


def _ego(j):
    return slow(STRIDE * j, STRIDE * j + STRIDE)


def _run(pipe, ctx, frame, n_pairs, with_ego):
    """n_pairs pairs of the frame through `pipe`, pairs_per_step at a time -> records (n_pairs, 2, MAX_DET, 17), counts."""
    per = pipe.pairs
    steps = n_pairs // per
    ring = max(steps, 2)
    rec_ring = ctx.zeros((ring, per, 2, MAX_DET, REC_COLS), np.float32)
    cnt_ring = ctx.zeros((ring, per, 2), np.int32)
    pipe.use_record_ring(rec_ring, cnt_ring)
    pipe.test_rings = (rec_ring, cnt_ring)          # (the pipeline writes there until it is given others)
    slots = [(pipe.step_idx + k) % ring for k in range(steps)]      # step k of the pipeline fills slot k % ring
    pts, img, heads = frame
    for k in range(steps):
        ego = [_ego(k * per + q) for q in range(per)] if with_ego else None
        pipe.run([pts] * (2 * per), [pts.shape[0]] * (2 * per), [img] * (2 * per), heads=[heads] * (2 * per),
                 ego_motion=ego)
    pipe.finish()
    ctx.sync()
    return (rec_ring.download()[slots].reshape(n_pairs, 2, MAX_DET, REC_COLS),
            cnt_ring.download()[slots].reshape(n_pairs, 2))


def _keyframe_lists(ctx, recs, cnts, score_threshold=0.1):
    """The encoded keyframe-0 rows of every pair and the keyframe-1 rows of the last, as kf_pipeline's detections."""
    n = len(recs)
    d_trk, d_k1 = ctx.empty((n, 128, 23), np.float32), ctx.empty((n, 128, 16), np.float32)
    d_cnt = ctx.empty((n, 4), np.int32)
    ops.track_encode(ctx, ctx.array(recs), ctx.array(cnts), n, MAX_DET, config.KITTI_P2, config.KITTI_IMAGE_WH,
                     score_threshold, d_trk, d_k1, d_cnt)
    trk, k1, cnt = d_trk.download(), d_k1.download(), d_cnt.download()
    lists = [trk[j, :cnt[j, 3], :16] for j in range(n)] + [k1[n - 1, :cnt[n - 1, 1]]]
    return [[{'frame_id': k * STRIDE, 'boxes3d': r[8:15].astype(np.float64), 'boxes2d': r[4:8].astype(np.float64),
              'scores': float(r[15])} for r in rows] for k, rows in enumerate(lists)]


@pytest.fixture(scope='module')
def world():
    ctx = device.default_context()
    kw = dict(rpn_nms_size=1024)
    plain = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), **kw)
    pts = synth.lidar_frame(20, 0)
    frame = (ctx.array(pts), ctx.array(synth.image_frame(20, 0)),
             {k: ctx.array(v) for k, v in synth.head_outputs(20, 0, plain.n_all, plain.P).items()})
    recs, cnts = _run(plain, ctx, frame, N_PAIRS, with_ego=True)
    # sigma_l: in the first gap of the first keyframe's sorted scores (3 decimals: there are ties) that leaves at least
    # N_DETS detections -- a dozen or two tracks keep the host's Python loop short
    scores = np.sort([d['scores'] for d in _keyframe_lists(ctx, recs, cnts)[0]])[::-1]
    cut = next(i for i in range(N_DETS, len(scores)) if scores[i - 1] > scores[i])
    assert cut <= 40
    sigma_l = float(scores[cut - 1] + scores[cut]) / 2
    tk = dict(kind='kalman', sigma_l=sigma_l, iou_threshold=GATE, max_age=3, min_hits=MIN_HITS, stride=STRIDE,
              max_sequence_dets=4096)
    one = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), tracker=tk, reuse_streams_of=plain, **kw)
    two = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), tracker=tk, pairs_per_step=2, **kw)
    yield dict(ctx=ctx, plain=plain, one=one, two=two, frame=frame, recs=recs, cnts=cnts, sigma_l=sigma_l)
    for p in (one, plain, two):
        p.close()


def _expected(w, recs, cnts):
    ctx = w['ctx']
    frames_h, frames_d = _keyframe_lists(ctx, recs, cnts), _keyframe_lists(ctx, recs, cnts)
    want, matrices = K.host_run(slow, K.CALIB_KITTI, frames_h, STRIDE, 10 ** 6, w['sigma_l'], GATE,
                                min_hits=MIN_HITS)
    gap = K.assert_fair(matrices, GATE)
    print('%d keyframes, %d tracks, smallest gap %.3g' % (len(frames_h), len(want), gap))
    assert len(want) >= N_DETS // 2 and len(matrices) == N_PAIRS
    got = dev.kf_pipeline(slow, K.CALIB_KITTI, frames_d, STRIDE, 10 ** 6, w['sigma_l'], GATE, min_hits=MIN_HITS,
                          ctx=ctx)
    K.assert_same_tracks(got, frames_d, want, frames_h)
    return want, frames_h


def test_end_sequence_equals_kf_pipeline_and_host(world):
    w = world
    recs, cnts = _run(w['one'], w['ctx'], w['frame'], N_PAIRS, with_ego=True)
    # the detection records of those steps are what a pipeline without a tracker gives
    assert np.array_equal(recs, w['recs']) and np.array_equal(cnts, w['cnts'])
    want, frames_h = _expected(w, recs, cnts)
    assert w['one'].tracks_so_far() == []               # nothing has finished: every track is still live
    got = w['one'].end_sequence()
    K.assert_same_tracks(got, None, want, frames_h)
    assert all(isinstance(t.x_state, np.ndarray) and t.x_state.shape == (8, 1) for t in got)
    with pytest.raises(ValueError):
        w['one'].kitti_tracking_rows()
    # a second sequence starts from id 0 and gives the same tracks
    assert w['one'].track_state.header()['next_id'] == 0
    recs2, cnts2 = _run(w['one'], w['ctx'], w['frame'], N_PAIRS, with_ego=True)
    assert np.array_equal(recs2, recs)
    again = w['one'].end_sequence()
    assert min(t.id for t in again) == 0
    K.assert_same_tracks(again, None, want, frames_h)


def test_two_pairs_per_step_equal_one(world):
    w = world
    recs, cnts = _run(w['two'], w['ctx'], w['frame'], N_PAIRS, with_ego=True)
    assert np.array_equal(recs, w['recs']) and np.array_equal(cnts, w['cnts'])
    want, frames_h = _expected(w, recs, cnts)
    K.assert_same_tracks(w['two'].end_sequence(), None, want, frames_h)


def test_parked_steps_and_refusals(world):
    w = world
    pts, img, heads = w['frame']
    with pytest.raises(ValueError, match='delta'):      # a 2-tuple: refused before anything is enqueued
        w['one'].run([pts] * 2, [pts.shape[0]] * 2, [img] * 2, heads=[heads] * 2, ego_motion=[_ego(0)[:2]])
    assert w['one'].pending is None
    recs, cnts = _run(w['one'], w['ctx'], w['frame'], 2, with_ego=False)
    frames_h = _keyframe_lists(w['ctx'], recs, cnts)
    want, matrices = K.host_run(K.PARKED, K.CALIB_KITTI, frames_h, STRIDE, 10 ** 6, w['sigma_l'], GATE, min_hits=MIN_HITS)
    K.assert_fair(matrices, GATE)
    K.assert_same_tracks(w['one'].end_sequence(), None, want, frames_h)
    # a pipeline with another tracker takes a 3-tuple and ignores its delta
    recs3, _ = _run(w['plain'], w['ctx'], w['frame'], 1, with_ego=True)
    assert np.array_equal(recs3[0], w['recs'][0])
