"""Shared by tests/test_gpu_kalman_lanes_pipeline.py and tests/test_gpu_velocity_lanes_pipeline.py:
FramePairPipeline(tracker=dict(kind=..., lanes=True)) on the device, modelled on tests/test_gpu_tracker_lanes_pipeline.py
(its configuration, N_POINTS, injected head outputs, the synthetic videos' ids and calibrations).

A video here is ONE synthetic frame repeated, as in tests/test_gpu_kalman_pipeline.py: every keyframe of a video holds
the same detections and the lane's ego motion alone separates a track's last box from its detection, which is what
makes a case fair for these two trackers (a unique optimum / a clear argmax) -- asserted on the host's own matrices all
the same.  Two videos with different calibrations and image sizes run side by side for ten steps: lane 0 parked, lane 1
moving (the kind's `motion`: K.moving, for the Kalman tracker `slow`); lane 1 pauses for a step; lane 0's video ends
after six steps with end_sequence(lane=0) and a third video starts there.  Each lane's tracks are held against a one-pair-per-step pipeline with the single tracker of the
kind over the same video (exactly), and against the host module on the pipeline's own records of the lane's active
steps."""
import numpy as np
import pytest

import _kalman_cases as K
import _tracking_cases as tc
import _velocity_cases as V
from dodt_amd import config, ops, synth
from dodt_amd.pipeline import MAX_DET, REC_COLS, FramePairPipeline

CFG = config.PYRAMID_DODT
N_POINTS = 30000
TEMPORAL = dict(n_frames=3, threshold=0.1, on_conflict='next_best')
STRIDE = 2                      # (tau of TEMPORAL: what tracker=dict(stride=None) takes)
N_DETS = 12
GATE = 0.1
CALS = tc.calibrations()
VIDEOS = dict(A=(20, CALS['default']), B=(30, CALS['object_000006']), C=(40, CALS['object_file']))
STEPS, END_A, IDLE = 10, 6, 4   # lane 0: video A for END_A steps, then C; lane 1: video B, idle at step IDLE


def slow(a, b):
    """A sixth of K.moving: 0.05 m and 1/600 rad per frame (tests/test_gpu_kalman_pipeline.py's motion and reason: the
    injected heads' boxes reach 70 m and are small; under K.moving some of them leave their own track's box from one
    keyframe to the next, and a track without any overlap makes the Kalman tracker's optimum ambiguous)."""
    trans, _, yaw = K.moving(a, b)
    c, s = np.cos(yaw / 6), np.sin(yaw / 6)
    return trans / 6, np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), yaw / 6


def _rt(cal):
    return np.asarray(cal.r0_rect, np.float64), np.asarray(cal.tr_velo_to_cam, np.float64)


class Kalman(object):
    name = 'kalman'
    videos = VIDEOS
    # lane 1's ego motion: K.moving at a sixth of its speed.  Under K.moving itself video B is not fair by K.assert_fair
    # (a track without any overlap, a second best 0 away)
    motion = staticmethod(lambda a, b: slow(a, b))

    def tracker(self, sigma_l):
        self.sigma_l = sigma_l
        return dict(kind='kalman', sigma_l=sigma_l, iou_threshold=GATE, max_age=3, min_hits=2, max_sequence_dets=4096)

    def dets(self, k, rows):
        return [{'frame_id': k * STRIDE, 'boxes3d': r[8:15].astype(np.float64), 'boxes2d': r[4:8].astype(np.float64),
                 'scores': float(r[15])} for r in rows]

    def host(self, ego, cal, frames_h):
        want, matrices = K.host_run(ego, _rt(cal), frames_h, STRIDE, 10 ** 6, self.sigma_l, GATE, min_hits=2)
        print('kalman: %d keyframes, %d tracks, smallest gap %.3g' % (len(frames_h), len(want),
                                                                      K.assert_fair(matrices, GATE)))
        return want

    def same_as_host(self, got, want, frames_h):
        K.assert_same_tracks(got, None, want, frames_h)

    def same_exactly(self, got, want, what):
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            assert (g.id, g.hits, g.no_losses) == (w.id, w.hits, w.no_losses), what
            assert np.array_equal(g.x_state, w.x_state) and np.array_equal(g.P, w.P) and list(g.box) == list(w.box), what
            assert [d['frame_id'] for d in g.dets] == [d['frame_id'] for d in w.dets], what
            for a, b in zip(g.dets, w.dets):
                assert bool(a.get('is_virtual')) == bool(b.get('is_virtual')) and a['scores'] == b['scores'], what
                assert np.array_equal(a['boxes3d'], b['boxes3d']) and np.array_equal(a['boxes2d'], b['boxes2d']), what


class Velocity(object):
    name = 'velocity'
    videos = VIDEOS
    motion = staticmethod(K.moving)         # lane 1's ego motion

    def tracker(self, sigma_l):
        self.params = dict(sigma_l=sigma_l, sigma_h=sigma_l, sigma_iou=GATE, t_min=2, extend_len=3)
        return dict(kind='velocity', log_capacity=4096, **self.params)

    def dets(self, k, rows):
        return [{'frame_id': k * STRIDE, 'info': np.array(['Car', '-1', '-1', '-10.0']),
                 'boxes2d': np.array(r[4:8], np.float32), 'boxes3d': np.array(r[8:15], np.float32),
                 'score': np.float32(r[15])} for r in rows]

    def host(self, ego, cal, frames_h):
        want, groups = V.host_run(ego, _rt(cal), frames_h, STRIDE, (len(frames_h) - 1) * STRIDE + 1, **self.params)
        print('velocity: %d keyframes, %d tracks, nearest IoU to sigma_iou %.3g, smallest contested win %.3g'
              % ((len(frames_h), len(want)) + V.assert_fair(groups, GATE)))
        return want

    def same_as_host(self, got, want, frames_h):
        V.assert_same_tracks(got, None, want, frames_h)

    def same_exactly(self, got, want, what):
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            assert [d['frame_id'] for d in g['dets']] == [d['frame_id'] for d in w['dets']], what
            for a, b in zip(g['dets'], w['dets']):
                assert np.array_equal(a['boxes3d'], b['boxes3d']) and np.array_equal(a['boxes2d'], b['boxes2d']), what
                assert a['score'] == b['score'] and list(a['info']) == list(b['info']), what
            assert g['max_score'] == w['max_score'] and g['extend_len'] == w['extend_len'], what
            assert np.array_equal(np.asarray(g['speed']), np.asarray(w['speed'])), what


class Video(object):
    """One synthetic frame, cut to the calibration's image size, with its injected head outputs: every pair of the
    video is that frame twice."""

    def __init__(self, ctx, name, spec, n_all, n_prop):
        self.name = name
        self.seq, self.cal = spec
        w, h = self.cal.image_wh
        pts = synth.lidar_frame(self.seq, 0, N_POINTS)
        self.pts, self.n = ctx.array(pts), len(pts)
        self.img = ctx.array(np.ascontiguousarray(synth.image_frame(self.seq, 0)[:h, :w]))
        self.heads = {k: ctx.array(v) for k, v in synth.head_outputs(self.seq, 0, n_all, n_prop).items()}


def run(pipe, videos, **kw):
    """One step: a pair of videos[p] in slot p."""
    n = 2 * len(videos)
    pipe.run(sum([[v.pts] * 2 for v in videos], []), sum([[v.n] * 2 for v in videos], []),
             sum([[v.img] * 2 for v in videos], []), heads=sum([[v.heads] * 2 for v in videos], []),
             calib=[v.cal for v in videos], **kw)
    assert n == 2 * pipe.pairs


def ego_of(motion, j):
    """Pair j's own motion (None: parked)."""
    return None if motion is None else motion(STRIDE * j, STRIDE * j + STRIDE)


def keyframe_rows(ctx, recs, cnts, cal):
    """(n, 2, MAX_DET, 17) records of one lane's pairs -> the encoded keyframe-0 rows of every pair and the keyframe-1
    rows of the last, under the lane's calibration."""
    n = len(recs)
    d_trk, d_k1 = ctx.empty((n, 128, 23), np.float32), ctx.empty((n, 128, 16), np.float32)
    d_cnt = ctx.empty((n, 4), np.int32)
    ops.track_encode(ctx, ctx.array(np.ascontiguousarray(recs)), ctx.array(np.ascontiguousarray(cnts)), n, MAX_DET,
                     cal.p2, cal.image_wh, 0.1, d_trk, d_k1, d_cnt)
    trk, k1, cnt = d_trk.download(), d_k1.download(), d_cnt.download()
    return [trk[j, :cnt[j, 3], :16] for j in range(n)] + [k1[n - 1, :cnt[n - 1, 1]]]


def pick_sigma_l(ctx, plain, video):
    """In the first gap of the video's sorted keyframe scores that leaves at least N_DETS detections: a dozen or two
    tracks keep the host's Python loops short."""
    rec = ctx.zeros((2, 1, 2, MAX_DET, REC_COLS), np.float32)
    cnt = ctx.zeros((2, 1, 2), np.int32)
    plain.use_record_ring(rec, cnt)
    slot = plain.step_idx % 2
    run(plain, [video])
    plain.finish()
    ctx.sync()
    rows = keyframe_rows(ctx, rec.download()[slot], cnt.download()[slot], video.cal)[0]
    scores = np.sort(rows[:, 15])[::-1]
    cut = next(i for i in range(N_DETS, len(scores)) if scores[i - 1] > scores[i])
    assert cut <= 40
    return float(scores[cut - 1] + scores[cut]) / 2


def make_world(ctx, kind):
    kw = dict(rpn_nms_size=1024, n_points_max=N_POINTS)
    plain = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), **kw)
    vid = {n: Video(ctx, n, spec, plain.n_all, plain.P) for n, spec in kind.videos.items()}
    tk = kind.tracker(pick_sigma_l(ctx, plain, vid['B']))
    lanes = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), pairs_per_step=2, temporal=TEMPORAL,
                              tracker=dict(tk, lanes=True), reuse_streams_of=plain, **kw)
    single = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), pairs_per_step=1, temporal=TEMPORAL, tracker=tk,
                               reuse_streams_of=plain, **kw)
    return dict(ctx=ctx, kind=kind, tk=tk, plain=plain, lanes=lanes, single=single, vid=vid)


def close_world(w):
    for p in (w['lanes'], w['single'], w['plain']):
        p.close()


def _single_tracks(w, video, n_pairs, motion):
    """The video alone through the one-pair-per-step pipeline with the kind's single tracker."""
    single = w['single']
    assert not single.lanes
    for j in range(n_pairs):
        run(single, [video], ego_motion=[ego_of(motion, j)])
    single.finish()
    return single.end_sequence()


def two_videos_side_by_side(w):
    ctx, kind, pipe, vid = w['ctx'], w['kind'], w['lanes'], w['vid']
    assert pipe.lanes and pipe.track_state.n_lanes == 2
    rec_ring = ctx.zeros((STEPS, 2, 2, MAX_DET, REC_COLS), np.float32)
    cnt_ring = ctx.zeros((STEPS, 2, 2), np.int32)
    pipe.use_record_ring(rec_ring, cnt_ring)
    first = pipe.step_idx
    b_pair = 0                                  # lane 1's own pair number
    for k in range(STEPS):
        lane0 = vid['A'] if k < END_A else vid['C']
        if k == IDLE:                           # lane 1 pauses: its slot filled all the same, its ego entry ignored
            run(pipe, [lane0, vid['B']], ego_motion=[None, ego_of(kind.motion, 77)], active=[True, False])
        else:
            run(pipe, [lane0, vid['B']], ego_motion=[None, ego_of(kind.motion, b_pair)])
            b_pair += 1
        if k == END_A - 1:                      # video A is over: lane 0 ends, lane 1 goes on
            pipe.finish()
            lane1_before = pipe.track_state.lane(1).used_bytes()
            got_a = pipe.end_sequence(lane=0)
            assert pipe.tracks_so_far(lane=0) == [] and pipe.last_sequence_tracks[1] is None
            assert pipe.track_state.lane(0).header()['keyframe'] == 0
            after = pipe.track_state.lane(1).used_bytes()
            assert all(np.array_equal(x, y) for x, y in zip(lane1_before, after))
    pipe.finish()
    assert [pipe.track_state.lane(i).header()['keyframe'] for i in range(2)] == [STEPS - END_A, STEPS - 1]
    got_c = pipe.end_sequence(lane=0)
    got_b = pipe.end_sequence(lane=1, frame_total=None)
    ctx.sync()
    slots = [(first + k) % STEPS for k in range(STEPS)]
    recs, cnts = rec_ring.download()[slots], cnt_ring.download()[slots]
    b_steps = [k for k in range(STEPS) if k != IDLE]
    cases = [('lane 0, video A', got_a, vid['A'], list(range(END_A)), 0, None),
             ('lane 0, video C', got_c, vid['C'], list(range(END_A, STEPS)), 0, None),
             ('lane 1, video B', got_b, vid['B'], b_steps, 1, kind.motion)]
    for what, got, video, steps, lane, motion in cases:
        # the host module on the pipeline's own records of the lane's active steps, under the lane's calibration
        lists = keyframe_rows(ctx, recs[steps, lane], cnts[steps, lane], video.cal)
        frames_h = [kind.dets(k, rows) for k, rows in enumerate(lists)]
        want = kind.host(K.PARKED if motion is None else motion, video.cal, frames_h)
        assert len(want) >= N_DETS // 2, what
        kind.same_as_host(got, want, frames_h)
        # the video alone, one pair per step, the kind's single tracker
        kind.same_exactly(got, _single_tracks(w, video, len(steps), motion), what + ' against one pair per step')
    # the idle slot was computed all the same
    assert cnts[IDLE, 1].sum() > 0 and np.array_equal(cnts[IDLE, 1], cnts[IDLE - 1, 1])
    # the lanes differ in what decides their tracks: video B's records under video A's calibration and ego are not fair
    # game for the same tracks
    other = kind.dets(0, keyframe_rows(ctx, recs[b_steps, 1], cnts[b_steps, 1], vid['A'].cal)[0])
    mine = kind.dets(0, keyframe_rows(ctx, recs[b_steps, 1], cnts[b_steps, 1], vid['B'].cal)[0])
    assert [d['boxes2d'].tobytes() for d in other] != [d['boxes2d'].tobytes() for d in mine]
    return got_a, got_b, got_c


def refusals(w):
    ctx, kind, pipe, vid = w['ctx'], w['kind'], w['lanes'], w['vid']
    weights = synth.pipeline_weights(CFG)
    with pytest.raises(ValueError, match='lanes'):
        FramePairPipeline(ctx, CFG, **weights, sequence=True, tracker=dict(w['tk'], lanes=True))
    with pytest.raises(ValueError, match='pairs_per_step >= 2'):
        FramePairPipeline(ctx, CFG, **weights, tracker=dict(w['tk'], lanes=True))
    with pytest.raises(ValueError, match='unknown keys'):
        FramePairPipeline(ctx, CFG, **weights, pairs_per_step=2, tracker=dict(w['tk'], lanes=True, lane=1))
    step, hdr = pipe.step_idx, [pipe.track_state.lane(i).header() for i in range(2)]
    for wrong in ([True], [True, False, True]):
        with pytest.raises(ValueError):
            run(pipe, [vid['A'], vid['B']], active=wrong)
    with pytest.raises(ValueError, match='delta'):
        run(pipe, [vid['A'], vid['B']], ego_motion=[None, ego_of(K.moving, 0)[:2]])
    assert pipe.step_idx == step and pipe.pending is None
    for call in (pipe.end_sequence, pipe.tracks_so_far):
        with pytest.raises(ValueError):              # no lane=
            call()
        with pytest.raises(ValueError):
            call(lane=2)
        with pytest.raises(ValueError, match='frame_ids'):
            call(lane=0, frame_ids=[(0, 2)])
    with pytest.raises(ValueError):
        w['single'].end_sequence(lane=0)
    with pytest.raises(ValueError):
        run(w['single'], [vid['A']], active=[True])
    assert [pipe.track_state.lane(i).header() for i in range(2)] == hdr
