"""FramePairPipeline(tracker=dict(lanes=True)) on the device: two videos side by side, pair p of every step in lane p,
each lane's tracks against the host module (dodt_amd.core.dt_evaluator_utils) run on that lane's ACTIVE steps of the
pipeline's own records with that lane's calibration, and against a one-pair-per-step pipeline with the single tracker;
and what a lanes pipeline refuses."""
import numpy as np
import pytest

import _tracking_cases as tc
from dodt_amd import config, device, synth
from dodt_amd.core import dt_evaluator_utils as host
from dodt_amd.pipeline import MAX_DET, REC_COLS, FramePairPipeline

pytestmark = pytest.mark.gpu
CFG = config.PYRAMID_DODT
N_POINTS = 30000
TEMPORAL = dict(n_frames=3, threshold=0.1, on_conflict='next_best')
TRACKER = dict(score_threshold=0.1, high_threshold=0.3, iou_threshold=0.005, t_min=1, classes=('Car',),
               max_sequence_dets=1 << 13)
PARAMS = (0.1, 0.3, 0.005, 1)
CALS = tc.calibrations()
# the synthetic sequence ids of the three videos (dodt_amd.synth; each video cycles over three pairs, frames 0 and 2 of
# ids v, v + 1, v + 2) and their calibrations; chosen on the device so that every ended sequence has tracks
VIDEOS = dict(A=(20, CALS['default']), B=(30, CALS['object_000006']), C=(40, CALS['object_file']))


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


class _Video(object):
    """The inputs of one video: pair j is frames (0, 2) of synthetic sequence id + j % 3, images of its calibration's
    size, injected head outputs."""

    def __init__(self, ctx, name, n_all, n_prop):
        self.seq, self.cal = VIDEOS[name]
        w, h = self.cal.image_wh
        self.steps = []
        for b in range(3):
            frames = [(self.seq + b, f) for f in (0, 2)]
            pts = [synth.lidar_frame(s, f, N_POINTS) for s, f in frames]
            self.steps.append(dict(
                pts=[ctx.array(p) for p in pts], n=[len(p) for p in pts],
                imgs=[ctx.array(np.ascontiguousarray(synth.image_frame(s, f)[:h, :w])) for s, f in frames],
                heads=[{k: ctx.array(v) for k, v in synth.head_outputs(s, f, n_all, n_prop).items()}
                       for s, f in frames]))

    def pair(self, j):
        return self.steps[j % 3]


def _run(pipe, pairs, **kw):
    """One step of the given (video, pair number) per lane."""
    parts = [v.pair(j) for v, j in pairs]
    pipe.run(sum([p['pts'] for p in parts], []), sum([p['n'] for p in parts], []), sum([p['imgs'] for p in parts], []),
             heads=sum([p['heads'] for p in parts], []), calib=[v.cal for v, _ in pairs], **kw)


def _host_pairs(recs, cnts, steps, lane):
    """The ring's slots `steps` of lane `lane` -> the host's [(frame_0, frame_1, records)], pair j of the lane's own
    numbering at frames (2j, 2j + 2) (tau = 2)."""
    out = []
    for j, k in enumerate(steps):
        rows = [recs[k, lane, f, :cnts[k, lane, f]] for f in range(2)]
        assert all(np.all(r[:, 16] == f) for f, r in enumerate(rows))
        out.append((2 * j, 2 * j + 2, np.concatenate(rows)))
    return out


def _want(host_pairs, cal):
    assert sum(len(p[2]) for p in host_pairs) > 0
    want = tc.host_tracks(host_pairs, cal, PARAMS)
    assert len(want) > 0
    return want


# ---- (f) -------------------------------------------------------------------------------------------------------------
def test_two_videos_side_by_side(ctx):
    steps = 10
    pipe = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), rpn_nms_size=1024, n_points_max=N_POINTS,
                             pairs_per_step=2, temporal=TEMPORAL, tracker=dict(TRACKER, lanes=True))
    vid = {n: _Video(ctx, n, pipe.n_all, pipe.P) for n in VIDEOS}
    rec_ring = ctx.zeros((steps, 2, 2, MAX_DET, REC_COLS), np.float32)
    cnt_ring = ctx.zeros((steps, 2, 2), np.int32)
    pipe.use_record_ring(rec_ring, cnt_ring)
    idle = 4                                    # lane 1 idles at this step, its slot filled with its previous pair
    b_pair = 0                                  # lane 1's own pair number
    for k in range(steps):
        lane0 = (vid['A'], k) if k < 6 else (vid['C'], k - 6)
        if k == idle:
            _run(pipe, [lane0, (vid['B'], b_pair - 1)], active=[True, False])
        else:
            _run(pipe, [lane0, (vid['B'], b_pair)])
            b_pair += 1
        if k == 5:                              # video A is over: lane 0 ends, lane 1 goes on
            pipe.finish()
            got_a = pipe.end_sequence(lane=0)
            rows_a = pipe.kitti_tracking_rows(lane=0)
            assert pipe.tracks_so_far(lane=0) == []
            assert pipe.last_sequence_tracks[1] is None
    pipe.finish()
    got_c = pipe.end_sequence(lane=0)
    got_b = pipe.end_sequence(lane=1)
    ctx.sync()
    recs, cnts = rec_ring.download(), cnt_ring.download()
    want_a = _want(_host_pairs(recs, cnts, range(6), 0), vid['A'].cal)
    want_c = _want(_host_pairs(recs, cnts, range(6, 10), 0), vid['C'].cal)
    b_steps = [k for k in range(steps) if k != idle]
    want_b = _want(_host_pairs(recs, cnts, b_steps, 1), vid['B'].cal)
    tc.same_tracks(got_a, want_a, 'lane 0, video A')
    tc.same_tracks(got_c, want_c, 'lane 0, video C')
    tc.same_tracks(got_b, want_b, 'lane 1, video B')
    assert np.array_equal(rows_a, host.convert_trajectory_to_kitti_format(want_a))
    assert np.array_equal(pipe.kitti_tracking_rows(lane=0), host.convert_trajectory_to_kitti_format(want_c))
    assert np.array_equal(pipe.kitti_tracking_rows(lane=1), host.convert_trajectory_to_kitti_format(want_b))
    # the idle slot was computed all the same: the records of lane 1's previous pair
    assert cnts[idle, 1].sum() > 0 and np.array_equal(cnts[idle, 1], cnts[idle - 1, 1])
    # the calibration matters: video B's records under the default give other tracks
    other = tc.host_tracks(_host_pairs(recs, cnts, b_steps, 1), CALS['default'], PARAMS)
    assert [[d['boxes2d'].tobytes() for d in t['trajectory']] for t in other] != \
        [[d['boxes2d'].tobytes() for d in t['trajectory']] for t in want_b]
    # video B alone, one pair per step, today's tracker
    single = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), rpn_nms_size=1024, n_points_max=N_POINTS,
                               pairs_per_step=1, temporal=TEMPORAL, tracker=TRACKER, reuse_streams_of=pipe)
    assert not single.lanes
    for j in range(len(b_steps)):
        _run(single, [(vid['B'], j)])
    single.finish()
    tc.same_tracks(got_b, single.end_sequence(), 'lane 1 against one pair per step')
    single.close()
    pipe.close()


# ---- (g) -------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    weights = synth.pipeline_weights(CFG)
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, CFG, **weights, sequence=True, tracker=dict(TRACKER, lanes=True))
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, CFG, **weights, pairs_per_step=2, tracker=dict(TRACKER, lanes=True, lane=1))
    pipe = FramePairPipeline(ctx, CFG, **weights, rpn_nms_size=1024, n_points_max=N_POINTS, pairs_per_step=2,
                             tracker=dict(TRACKER, lanes=True))
    vid = {n: _Video(ctx, n, pipe.n_all, pipe.P) for n in ('A', 'C')}
    for wrong in ([True], [True, False, True]):
        with pytest.raises(ValueError):
            _run(pipe, [(vid['A'], 0), (vid['C'], 0)], active=wrong)
    assert pipe.step_idx == 0 and pipe.pending is None
    _run(pipe, [(vid['A'], 0), (vid['C'], 0)])
    with pytest.raises(ValueError):              # lane 0's calibration changes without end_sequence(lane=0)
        _run(pipe, [(vid['C'], 1), (vid['C'], 1)])
    with pytest.raises(ValueError):              # a step is pending
        pipe.end_sequence(lane=0)
    assert pipe.step_idx == 1 and pipe.pending is not None and pipe.pending.step == 0
    pipe.finish()
    with pytest.raises(ValueError):              # no lane=
        pipe.end_sequence()
    with pytest.raises(ValueError):
        pipe.tracks_so_far()
    with pytest.raises(ValueError):
        pipe.end_sequence(lane=2)
    h = [pipe.track_state.lane(i).header() for i in range(2)]
    assert [x['seq_pair'] for x in h] == [1, 1]  # one step was tracked, nothing else reached a lane
    assert pipe.end_sequence(lane=0) is not None
    _run(pipe, [(vid['C'], 1), (vid['C'], 1)])   # now lane 0 may take video C
    pipe.finish()
    assert [pipe.track_state.lane(i).header()['seq_pair'] for i in range(2)] == [1, 2]
    pipe.close()
