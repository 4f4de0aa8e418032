"""Tracker lanes without a GPU: the stride entry of the library, the cases the device tests use (held to what they are
chosen for with the host module alone), and the pipeline's plumbing of tracker=dict(lanes=True) over the recording
stand-ins (tests/_lanes_trace.py): every lanes launch carries, per lane, the calibration ITS step brought for that lane
and that step's `active` -- the step whose tail the call enqueues, one call after the step itself --, what is refused
logs nothing, and nothing races."""
import numpy as np
import pytest

import _geometry_trace as gt
import _lanes_trace as lt
import _pipeline_trace as tr
import _tracking_cases as tc
from dodt_amd import ops

A, B, C = gt.real_calibrations()


# ---- the library ------------------------------------------------------------------------------------------------------
def test_lanes_stride():
    last = 0
    for cap in (1, 2, 3, 7, 8, 9, 100, 4096, 65536, 1 << 20):
        stride, nbytes = ops.track_lanes_stride(cap), ops.track_state_bytes(cap)
        assert stride % 256 == 0 and nbytes <= stride < nbytes + 256
        assert stride >= last
        last = stride
    assert ops.track_lanes_stride(1 << 20) > ops.track_lanes_stride(1)
    with pytest.raises(Exception):
        ops.track_lanes_stride(0)


# ---- the cases of the device tests ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('params', [tc.REFERENCE, tc.LOOSE])
def test_lane_cases_are_not_trivial(params):
    """Every lane of case (a) long enough to finish a track of six detections does so, and at least five tracks.  (A
    sequence of ONE pair finishes nothing under either parameter set: a track made in the only pair has length 1, below
    t_min = 2 or 3.  That lane is there for its state -- header, active list, previous rows --, compared with a single
    tracker's on the device.)"""
    cals = tc.calibrations()
    assert cals['tracking_file'].key() == cals['default'].key()
    assert [c['n_pairs'] for c in tc.LANES_A] == [48, 31, 17, 1, 0]
    assert len({c['seed'] for c in tc.LANES_A}) == 5 and all(c['n_obj'] <= 20 for c in tc.LANES_A)
    assert len({cals[c['cal']].key() for c in tc.LANES_A}) == 3
    assert sum(c['special'] for c in tc.LANES_A) == 1
    for i, c in enumerate(tc.LANES_A):
        pairs = tc.lane_a(i)
        assert len(pairs) == c['n_pairs']
        if c['n_pairs'] >= 6:
            assert c['empty'] and all(len(pairs[j][2]) == 0 for j in c['empty'])
            want = tc.lane_a_tracks(i, params)
            assert len(want) >= 5 and max(len(t['trajectory']) for t in want) >= 6, i
        elif c['n_pairs']:
            assert tc.lane_a_tracks(i, params) == [] and len(pairs[0][2]) > 0
    # the lane with the special rows: its image size decides what the truncation rules keep
    i = [c['special'] for c in tc.LANES_A].index(True)
    other = tc.host_tracks(tc.lane_a(i), cals['default'], params)
    mine = tc.lane_a_tracks(i, params)
    assert [[d['boxes2d'].tobytes() for d in t['trajectory']] for t in other] != \
        [[d['boxes2d'].tobytes() for d in t['trajectory']] for t in mine]


def test_live_parts_layout():
    from dodt_amd import tracking
    assert tc.FIN_OFF == tracking._FIN_OFF and tracking._HDR[9:11] == ('prev_nL', 'prev_n1')
    assert tracking._HDR[0] == 'n_active' and tracking._HDR[2:4] == ('n_log', 'n_fin') and tracking._HDR[7] == 'has_prev'


# ---- the pipeline's plumbing ------------------------------------------------------------------------------------------
def _inputs(pipe, cals):
    frames = [gt.frame(pipe, cal) for cal in cals for _ in range(pipe.fps)]
    return [list(a) for a in zip(*frames)]


def _lanes_launches(trace, start=0, end=None):
    return [t for t in trace[start:end] if not t.get('event') and t['op'] == 'track_lanes']


def _carries(t, cals, active):
    p2s, whs, act = t['args'][4], t['args'][5], t['args'][6]
    assert len(p2s) == len(whs) == len(cals)
    assert all(np.array_equal(p, c.p2) and tuple(w) == tuple(c.image_wh) for p, w, c in zip(p2s, whs, cals))
    assert act == tuple(active)
    return True


# (calibrations of the step's pairs, active); lane 0: B, then -- behind end_sequence(lane=0) after step 3 -- C; lane 1: A,
# idle at steps 2 and 5 with "any valid frames" of another calibration in its slot
STEPS = [([B, A], (True, True)), ([B, A], (True, True)), ([B, C], (True, False)), ([B, A], None),
         ([C, A], (True, True)), ([C, B], (True, False)), ([C, A], (True, True))]


@pytest.mark.parametrize('host', [False, True], ids=['device', 'from_host'])
def test_lanes_launch_carries_its_steps_calibrations_and_active(monkeypatch, host):
    build, _ = lt.install(monkeypatch)
    pipe, trace, _ = build(head_params=tr.HP, pairs_per_step=2, temporal=dict(n_frames=3), tracker=dict(lanes=True),
                           image_wh_max=(1242, 375))
    assert isinstance(pipe.track_state, lt.TrackerLanes) and pipe.track_state.n_lanes == 2
    assert pipe.last_sequence_tracks == [None, None]
    run = pipe.run_from_host if host else pipe.run
    ins = [_inputs(pipe, cals) for cals, _ in STEPS]
    if host:
        ins = [[[object() for _ in p], n, [object() for _ in i]] for p, n, i in ins]
    launches = []                   # (the launch, the call that enqueued it)
    for k, (cals, active) in enumerate(STEPS):
        la = None
        if k in (1, 5):             # announced one call early, with its calibrations
            la = tuple(ins[k + 1]) + (None, STEPS[k + 1][0])
        n = len(trace)
        kw = {} if active is None else dict(active=active)
        if not host:
            kw['recover'] = tr._recover(pipe, k % 2 == 1)
        run(*ins[k], lookahead=la, calib=cals, **kw)
        launches += [(t, 'run %d' % k) for t in _lanes_launches(trace, n)]
        if k == 3:
            n = len(trace)
            pipe.finish()
            launches += [(t, 'finish 3') for t in _lanes_launches(trace, n)]
            n = len(trace)
            assert pipe.end_sequence(lane=0) == []
            # lane 0's slice alone is flushed and reset, on the image stream
            ops_ = [(t['op'], t['stream'], t['arrays'][0].ptr) for t in trace[n:] if not t.get('event')]
            lane0 = pipe.track_state.lane(0).d_state.ptr
            assert ops_ == [('track_flush', 'img', lane0), ('track_reset', 'img', lane0)]
            assert pipe.track_geoms[0] is None and pipe.track_geoms[1] is not None
    n = len(trace)
    pipe.finish()
    launches += [(t, 'finish') for t in _lanes_launches(trace, n)]
    # one launch per step, in step order, each enqueued by the call AFTER its step (the late tail), on the image stream
    assert [who for _, who in launches] == ['run 1', 'run 2', 'run 3', 'finish 3', 'run 5', 'run 6', 'finish']
    for (t, who), (cals, active) in zip(launches, STEPS):
        assert t['stream'] == 'img' and t['args'][3] == gt.pl.MAX_DET
        assert _carries(t, cals, active or (True, True)), who
    # the records the launch reads are the slot of ITS step
    assert [t['args'][1] is pipe.rec2[k % len(pipe.rec2)] for k, (t, _) in enumerate(launches)] == [True] * len(STEPS)
    assert not tr.races(pipe, trace)


def test_lanes_refusals_log_nothing(monkeypatch):
    build, _ = lt.install(monkeypatch)
    with pytest.raises(ValueError):
        build(sequence=True, tracker=dict(lanes=True))
    with pytest.raises(ValueError):
        build(pairs_per_step=2, tracker=dict(lanes=True, lane=3))
    pipe, trace, _ = build(pairs_per_step=2, tracker=dict(lanes=True))
    heads = tr._heads(pipe) * 2
    n = len(trace)
    for wrong in ((True,), (True, False, True), []):
        with pytest.raises(ValueError):
            pipe.run(*_inputs(pipe, [A, A]), heads=heads, active=wrong)
    assert len(trace) == n and pipe.step_idx == 0 and pipe.track_geoms == [None, None]
    pipe.run(*_inputs(pipe, [B, C]), heads=heads, calib=[B, C], active=(True, False))
    assert pipe.track_geoms[0] is not None and pipe.track_geoms[1] is None      # the idle lane has not begun
    pipe.run(*_inputs(pipe, [B, A]), heads=heads, calib=[B, A])                 # lane 1 begins, under A
    n = len(trace)
    with pytest.raises(ValueError):                  # lane 0's calibration changes mid-sequence
        pipe.run(*_inputs(pipe, [C, A]), heads=heads, calib=[C, A])
    with pytest.raises(ValueError):                  # lane 1's
        pipe.run(*_inputs(pipe, [B, B]), heads=heads, calib=[B, B])
    with pytest.raises(ValueError):                  # no lane=
        pipe.end_sequence()
    with pytest.raises(ValueError):
        pipe.tracks_so_far()
    with pytest.raises(ValueError):
        pipe.end_sequence(lane=2)
    with pytest.raises(ValueError):                  # a step is pending
        pipe.end_sequence(lane=0)
    with pytest.raises(ValueError):
        pipe.kitti_tracking_rows(lane=0)             # no sequence of lane 0 has ended
    assert len(trace) == n and pipe.step_idx == 2
    pipe.run(*_inputs(pipe, [B, C]), heads=heads, calib=[B, C], active=(True, False))    # idle: any calibration
    pipe.finish()
    pipe.end_sequence(lane=0)
    pipe.run(*_inputs(pipe, [C, A]), heads=heads, calib=[C, A])
    assert pipe.kitti_tracking_rows(lane=0) is not None
    # a pipeline without lanes takes neither `active` nor lane=
    plain, ptrace, _ = build(pairs_per_step=2, tracker={})
    assert isinstance(plain.track_state, gt.GeomTracker) and plain.last_sequence_tracks is None
    n = len(ptrace)
    with pytest.raises(ValueError):
        plain.run(*_inputs(plain, [A, A]), heads=heads, active=(True, True))
    with pytest.raises(ValueError):
        plain.end_sequence(lane=0)
    with pytest.raises(ValueError):
        plain.tracks_so_far(lane=0)
    assert len(ptrace) == n


def test_without_lanes_the_launches_are_todays(monkeypatch):
    """tracker={} and tracker=dict(lanes=False): the same launches, through tracking.Tracker."""
    texts = []
    for tk in ({}, dict(lanes=False)):
        build, _ = lt.install(monkeypatch)
        pipe, trace, _ = build(head_params=tr.HP, pairs_per_step=2, tracker=tk)
        extra = dict(inputs=[])
        for k in range(3):
            ins = _inputs(pipe, [A, A])
            extra['inputs'].append(ins)
            pipe.run(*ins)
        pipe.finish()
        pipe.end_sequence()
        assert [t['op'] for t in trace if not t.get('event')].count('track_records') == 3
        assert not _lanes_launches(trace)
        texts.append(tr.canonical(pipe, trace, extra))
    assert texts[0] == texts[1]
