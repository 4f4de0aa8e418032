"""Lanes of the Kalman and the velocity tracker without a GPU: the stride entries of the library, the pipeline's argument
checks, its plumbing of tracker=dict(kind=..., lanes=True) over recording stand-ins of the two lanes classes (in this
file, on top of tests/_geometry_trace.py) -- every lanes launch carries, per lane, the calibration and the ego entry ITS
step brought for that lane and that step's `active`; end_sequence(lane=) flushes and resets that lane alone with that
lane's calibration --, and the per-lane pending_ego bookkeeping of the real classes with their ops calls stubbed."""
import numpy as np
import pytest

import _geometry_trace as gt
import _pipeline_trace as tr
from dodt_amd import ops
from dodt_amd import pipeline as pl
from dodt_amd import tracking as dev

A, B, C = gt.real_calibrations()
KINDS = ('kalman', 'velocity')
STRIDE = 256


def _ego(tag):
    """An ego entry that names itself."""
    return (np.full(3, float(tag)), np.eye(3), 0.001 * tag)


# ---- the library ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_lanes_stride(kind):
    stride_of, bytes_of = ((ops.kf_lanes_stride, ops.kf_state_bytes) if kind == 'kalman'
                           else (ops.vt_lanes_stride, ops.vt_state_bytes))
    last = 0
    for cap in (1, 2, 3, 7, 100, 4096, 65536):
        stride, nbytes = stride_of(cap), bytes_of(cap)
        assert stride % 256 == 0 and nbytes <= stride < nbytes + 256 and stride >= last
        last = stride
    with pytest.raises(Exception):
        stride_of(0)
    assert ops.KIND_LANES_CHUNK == 8


# ---- the recording stand-ins --------------------------------------------------------------------------------------------
class _Lane(object):
    """A lane's single tracker over its slice: reset / flush logged on the context they are given, nothing tracked."""

    def __init__(self, ctx, d_state, kind):
        self.ctx, self.d_state, self.kind, self.pending_ego = ctx, d_state, kind, None
        self.reset()

    def reset(self, ctx=None):
        (ctx or self.ctx).log('lane_reset', [self.d_state])
        self.pending_ego = None

    def flush(self, calib42, ctx=None):
        (ctx or self.ctx).log('lane_flush', [self.d_state, np.array(calib42), self.pending_ego])
        self.pending_ego = None

    def header(self):
        return dict(keyframe=0)

    def read(self):
        t, lg = (dev.KF_TRACK, dev.KF_LOG) if self.kind == 'kalman' else (dev.VT_TRACK, dev.VT_LOG)
        return np.zeros(0, t), np.zeros(0, lg)


def _lanes_class(kind):
    class Lanes(object):
        def __init__(self, ctx=None, n_lanes=1, *args, **kw):
            self.ctx, self.n_lanes, self.stride, self.made_with = ctx, int(n_lanes), STRIDE, (args, kw)
            self.d_states = ctx.empty((self.n_lanes * STRIDE,), np.uint8)
            self.lanes = [_Lane(ctx, self.d_states.offset(i * STRIDE, (64,), np.uint8), kind)
                          for i in range(self.n_lanes)]

        def lane(self, i):
            return self.lanes[i]

        def track_records(self, d_records, d_counts, max_det, p2s, image_whs, egos, calibs, active=None, ctx=None):
            (ctx or self.ctx).log('kind_lanes', [self.d_states, d_records, d_counts, max_det, list(p2s), list(image_whs),
                                                 list(egos), [np.array(c) for c in calibs],
                                                 None if active is None else tuple(active)])
            for ln, a, e in zip(self.lanes, active or [True] * self.n_lanes, egos):
                if a:
                    ln.pending_ego = e
    return Lanes


def _install(monkeypatch, kind):
    build, uploads = gt.install(monkeypatch)
    name = 'KalmanTrackerLanes' if kind == 'kalman' else 'VelocityTrackerLanes'
    monkeypatch.setattr(pl.tracking, name, _lanes_class(kind))
    return build


def _inputs(pipe, cals):
    frames = [gt.frame(pipe, cal) for cal in cals for _ in range(pipe.fps)]
    return [list(a) for a in zip(*frames)]


def _launches(trace, start=0):
    return [t for t in trace[start:] if not t.get('event') and t['op'] == 'kind_lanes']


# ---- the argument checks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_argument_checks(monkeypatch, kind):
    build = _install(monkeypatch, kind)
    with pytest.raises(ValueError, match='lanes'):                  # one lane is the plain tracker
        build(tracker=dict(kind=kind, lanes=True))
    with pytest.raises(ValueError, match='pairs_per_step >= 2'):
        build(pairs_per_step=1, tracker=dict(kind=kind, lanes=True))
    with pytest.raises(ValueError, match='lanes'):
        build(sequence=True, tracker=dict(kind=kind, lanes=True))
    with pytest.raises(ValueError, match='unknown keys'):
        build(pairs_per_step=2, tracker=dict(kind=kind, lanes=True, lane=1))
    with pytest.raises(ValueError, match='unknown keys'):            # (the IoU tracker's key)
        build(pairs_per_step=2, tracker=dict(kind=kind, lanes=True, high_threshold=0.5))
    # the refusal stands in front of anything that touches the context
    with pytest.raises(ValueError, match='lanes'):
        pl.FramePairPipeline(None, pl._config.PYRAMID_DODT, None, None, tracker=dict(kind=kind, lanes=True))
    pipe, trace, _ = build(pairs_per_step=2, tracker=dict(kind=kind, lanes=True, stride=2, sigma_l=0.3))
    assert pipe.lanes and pipe.track_state.n_lanes == 2 and pipe.last_sequence_tracks == [None, None]
    assert (pipe.kalman, pipe.velocity) == (kind == 'kalman', kind == 'velocity')
    for n in (3, 5):
        assert build(pairs_per_step=n, tracker=dict(kind=kind, lanes=True))[0].track_state.n_lanes == n


# ---- the plumbing -------------------------------------------------------------------------------------------------------
# (calibrations of the step's pairs, active, ego entries); lane 0: B, then -- behind end_sequence(lane=0) after step 3 --
# C; lane 1: A, idle at steps 2 and 5 with "any valid frames" of another calibration in its slot
STEPS = [([B, A], (True, True), [_ego(1), None]), ([B, A], (True, True), [_ego(2), _ego(3)]),
         ([B, C], (True, False), [None, _ego(4)]), ([B, A], None, None),
         ([C, A], (True, True), [_ego(5), _ego(6)]), ([C, B], (True, False), [_ego(7), _ego(8)]),
         ([C, A], (True, True), [None, _ego(9)])]


def _same_ego(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize('kind', KINDS)
def test_lanes_launch_carries_its_steps_calibrations_egos_and_active(monkeypatch, kind):
    build = _install(monkeypatch, kind)
    pipe, trace, _ = build(head_params=tr.HP, pairs_per_step=2, temporal=dict(n_frames=3),
                           tracker=dict(kind=kind, lanes=True), image_wh_max=(1242, 375))
    ins = [_inputs(pipe, cals) for cals, _, _ in STEPS]
    launches = []
    for k, (cals, active, egos) in enumerate(STEPS):
        la = None
        if k in (1, 5):             # announced one call early, with its ego motion and calibrations
            la = tuple(ins[k + 1]) + (STEPS[k + 1][2], STEPS[k + 1][0])
        n = len(trace)
        kw = {} if active is None else dict(active=active)
        pipe.run(*ins[k], ego_motion=egos, lookahead=la, calib=cals, recover=tr._recover(pipe, k % 2 == 1), **kw)
        launches += [(t, 'run %d' % k) for t in _launches(trace, n)]
        if k == 3:
            n = len(trace)
            pipe.finish()
            launches += [(t, 'finish 3') for t in _launches(trace, n)]
            n = len(trace)
            lane0, lane1 = pipe.track_state.lane(0), pipe.track_state.lane(1)
            pend = lane0.pending_ego            # (step 3 brought no ego motion: parked)
            assert pend is None and _same_ego(lane1.pending_ego, None)
            with pytest.raises(ValueError, match='frame_ids'):
                pipe.end_sequence(lane=0, frame_ids=[(0, 2)])
            assert pipe.end_sequence(lane=0) == []
            # lane 0's slice alone is flushed -- with lane 0's calibration -- and reset, on the image stream
            got = [(t['op'], t['stream'], t['arrays'][0].ptr) for t in trace[n:] if not t.get('event')]
            assert got == [('lane_flush', 'img', lane0.d_state.ptr), ('lane_reset', 'img', lane0.d_state.ptr)]
            flush = [t for t in trace[n:] if not t.get('event')][0]
            assert np.array_equal(flush['args'][1], pl.ops.temporal_calib(B.r0_rect, B.tr_velo_to_cam))
            assert not np.array_equal(flush['args'][1], pl.ops.temporal_calib(A.r0_rect, A.tr_velo_to_cam))
            assert pipe.track_geoms[0] is None and pipe.track_geoms[1] is not None
            assert pipe.last_sequence_tracks[1] is None and pipe.last_sequence_tracks[0] == []
    n = len(trace)
    pipe.finish()
    launches += [(t, 'finish') for t in _launches(trace, n)]
    # one launch per step, in step order, each enqueued by the call AFTER its step (the late tail), on the image stream
    assert [who for _, who in launches] == ['run 1', 'run 2', 'run 3', 'finish 3', 'run 5', 'run 6', 'finish']
    for (t, who), (cals, active, egos) in zip(launches, STEPS):
        _, _, _, max_det, p2s, whs, got_egos, c42s, act = t['args']
        assert t['stream'] == 'img' and max_det == gt.pl.MAX_DET, who
        assert all(np.array_equal(p, c.p2) and tuple(w) == tuple(c.image_wh) for p, w, c in zip(p2s, whs, cals)), who
        assert all(np.array_equal(x, pl.ops.temporal_calib(c.r0_rect, c.tr_velo_to_cam)) for x, c in zip(c42s, cals)), who
        assert len({x.tobytes() for x in c42s}) == 2, who           # (every step's two pairs differ in calibration)
        assert act == tuple(active or (True, True)), who
        assert all(_same_ego(g, w) for g, w in zip(got_egos, egos or [None, None])), who
    # the records the launch reads are the slot of ITS step
    assert [t['args'][1] is pipe.rec2[k % len(pipe.rec2)] for k, (t, _) in enumerate(launches)] == [True] * len(STEPS)
    assert not tr.races(pipe, trace)
    # per-lane readers
    with pytest.raises(ValueError):
        pipe.tracks_so_far()
    with pytest.raises(ValueError):
        pipe.end_sequence()
    with pytest.raises(ValueError):
        pipe.end_sequence(lane=2)
    with pytest.raises(ValueError, match='frame_ids'):
        pipe.tracks_so_far(lane=1, frame_ids=[(0, 2)])
    assert pipe.tracks_so_far(lane=1) == []
    n = len(trace)
    assert pipe.end_sequence(lane=1, frame_total=40) == []
    flush = [t for t in trace[n:] if not t.get('event')][0]
    assert flush['op'] == 'lane_flush' and flush['arrays'][0].ptr == pipe.track_state.lane(1).d_state.ptr
    assert np.array_equal(flush['args'][1], pl.ops.temporal_calib(A.r0_rect, A.tr_velo_to_cam))
    assert _same_ego(flush['args'][2], _ego(9))                      # lane 1's pending ego: its last active pair's
    if kind == 'velocity':
        assert pipe.kitti_tracking_rows(lane=1) is not None
        with pytest.raises(ValueError):
            pipe.kitti_tracking_rows()


@pytest.mark.parametrize('kind', KINDS)
def test_refusals_log_nothing(monkeypatch, kind):
    build = _install(monkeypatch, kind)
    pipe, trace, _ = build(pairs_per_step=2, tracker=dict(kind=kind, lanes=True))
    heads = tr._heads(pipe) * 2
    n = len(trace)
    for wrong in ((True,), (True, False, True), []):
        with pytest.raises(ValueError):
            pipe.run(*_inputs(pipe, [A, A]), heads=heads, active=wrong)
    with pytest.raises(ValueError, match='delta'):                   # _check_ego applies as on a single tracker
        pipe.run(*_inputs(pipe, [A, A]), heads=heads, ego_motion=[_ego(1)[:2], None])
    with pytest.raises(ValueError, match='one entry per pair'):
        pipe.run(*_inputs(pipe, [A, A]), heads=heads, ego_motion=[_ego(1)])
    assert len(trace) == n and pipe.step_idx == 0 and pipe.track_geoms == [None, None]
    pipe.run(*_inputs(pipe, [B, C]), heads=heads, calib=[B, C], active=(True, False))
    pipe.run(*_inputs(pipe, [B, A]), heads=heads, calib=[B, A])
    n = len(trace)
    with pytest.raises(ValueError):                  # lane 0's calibration changes mid-sequence
        pipe.run(*_inputs(pipe, [C, A]), heads=heads, calib=[C, A])
    with pytest.raises(ValueError):                  # a step is pending
        pipe.end_sequence(lane=0)
    assert len(trace) == n and pipe.step_idx == 2


# ---- the real classes' bookkeeping ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_pending_ego_per_lane(monkeypatch, kind):
    """The ego row handed to step k of a lane is the motion of that lane's previous ACTIVE pair (parked at a lane's first
    pair and behind a reset); an inactive lane's entry is dropped and its pending one kept."""
    calls = []
    pre = 'kf' if kind == 'kalman' else 'vt'
    monkeypatch.setattr(dev.ops, pre + '_reset', lambda ctx, d_state, cap: calls.append(('reset', d_state.ptr)))
    monkeypatch.setattr(dev.ops, pre + '_flush',
                        lambda ctx, d_state, ego, c42, params: calls.append(('flush', d_state.ptr, ego)))

    def track(ctx, d_states, stride, n_lanes, d_records, d_counts, max_det, p2s, whs, ego_rows, calibs, thr, params,
              active=None):
        calls.append(('lanes', np.array(ego_rows), tuple(active), stride, n_lanes))
    monkeypatch.setattr(dev.ops, pre + '_track_lanes', track)
    ctx = tr.Ctx('main', [])
    cls = dev.KalmanTrackerLanes if kind == 'kalman' else dev.VelocityTrackerLanes
    lanes = cls(ctx, 3, log_capacity=64)
    stride = (ops.kf_lanes_stride if kind == 'kalman' else ops.vt_lanes_stride)(64)
    assert lanes.stride == stride and lanes.d_states.nbytes == 3 * stride
    assert [c[0] for c in calls] == ['reset'] * 3
    assert [c[1] - lanes.d_states.ptr for c in calls] == [0, stride, 2 * stride]
    single = dev.KalmanTracker if kind == 'kalman' else dev.VelocityTracker
    assert all(isinstance(lanes.lane(i), single) for i in range(3))
    parked = ops.kf_ego_rows([None])[0]

    def row(tag):
        return ops.kf_ego_rows([_ego(tag)])[0]

    def step(egos, active=None):
        lanes.track_records(None, None, 8, [A.p2] * 3, [A.image_wh] * 3, egos, [np.zeros(42)] * 3, active=active)
        return calls[-1]
    _, rows, act, _, _ = step([_ego(1), None, _ego(2)])
    assert act == (True, True, True) and all(np.array_equal(r, parked) for r in rows)
    _, rows, act, _, _ = step([_ego(3), _ego(4), _ego(5)], active=[True, False, True])
    assert act == (True, False, True)
    assert np.array_equal(rows[0], row(1)) and np.array_equal(rows[1], parked) and np.array_equal(rows[2], row(2))
    assert lanes.lane(1).pending_ego is None                        # (its own last pair was parked; entry 4 is dropped)
    _, rows, _, _, _ = step([None, _ego(6), _ego(7)], active=[0, 1, 1])
    assert np.array_equal(rows[0], parked) and np.array_equal(rows[1], parked) and np.array_equal(rows[2], row(5))
    assert _same_ego(lanes.lane(0).pending_ego, _ego(3))            # kept over the step it sat out
    # ending lane 2: its flush takes ITS pending ego; behind the reset its next keyframe is parked again
    lanes.lane(2).flush(np.zeros(42))
    assert calls[-1][0] == 'flush' and calls[-1][1] == lanes.lane(2).d_state.ptr and np.array_equal(calls[-1][2], row(7))
    lanes.lane(2).reset()
    _, rows, _, _, _ = step([_ego(8), _ego(9), _ego(10)])
    assert np.array_equal(rows[0], row(3)) and np.array_equal(rows[1], row(6)) and np.array_equal(rows[2], parked)
    for wrong in ([None] * 2, [None] * 4):
        with pytest.raises(ValueError):
            step(wrong)
    with pytest.raises(ValueError):
        step([None] * 3, active=[True])
    assert _same_ego(lanes.lane(2).pending_ego, _ego(10))           # (what was refused moved nothing)
