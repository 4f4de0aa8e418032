"""Tracker lanes on the device (dodt_track_lanes, dodt_amd.tracking.TrackerLanes): several sequences advance by one pair
each per call, every lane on a state, a calibration and an image size of its own -- against the host module
(dodt_amd.core.dt_evaluator_utils) and against single Trackers fed the same pairs one dodt_track_pairs call each.
Every comparison is exact.  The records are synthetic (tests/_tracking_cases.py); no net runs here."""
import numpy as np
import pytest

import _tracking_cases as tc
from dodt_amd import device
from dodt_amd import tracking as dev

pytestmark = pytest.mark.gpu
CALS = tc.calibrations()


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _single(ctx, pairs, cal, params, cap, max_det):
    """A Tracker of its own fed `pairs` one track_records call each (not flushed)."""
    score, high, iou, t_min = params
    tr = dev.Tracker(ctx, cap, high, iou, t_min, score)
    recs, counts = tc.pack(pairs, max_det)
    for j in range(len(pairs)):
        tr.track_records(ctx.array(recs[j:j + 1]), ctx.array(counts[j:j + 1]), 1, max_det, cal.p2, cal.image_wh)
    return tr


def _run_lanes(ctx, lanes, seqs, cals, max_det, steps=None, filler=None):
    """One track_records call per step: lane i takes pair k of seqs[i] while it has one and is inactive afterwards, its
    slot then holding `filler`'s pair (valid records that must not reach it)."""
    packed = [tc.pack(s, max_det) for s in seqs]
    fill = tc.pack(filler, max_det) if filler else None
    n = len(seqs)
    for k in range(max(len(s) for s in seqs) if steps is None else steps):
        recs = np.zeros((n, 2, max_det, 17), np.float32)
        counts = np.zeros((n, 2), np.int32)
        active = [k < len(s) for s in seqs]
        for i in range(n):
            if active[i]:
                recs[i], counts[i] = packed[i][0][k], packed[i][1][k]
            elif fill is not None:
                recs[i], counts[i] = fill[0][k % len(filler)], fill[1][k % len(filler)]
        lanes.track_records(ctx.array(recs), ctx.array(counts), max_det, [c.p2 for c in cals],
                            [c.image_wh for c in cals], active=active)


def _state(tr, cap):
    nbytes = dev.ops.track_state_bytes(cap)
    return tr.d_state.offset(0, (nbytes,), np.uint8).download()


def _same_as_single(ctx, lane, pairs, cal, params, cap, max_det, what):
    """Lane against a single tracker of the same pairs: the live parts of the state byte for byte, then -- both flushed
    -- header() and read()."""
    one = _single(ctx, pairs, cal, params, cap, max_det)
    assert tc.live_parts(_state(lane, cap), cap) == tc.live_parts(_state(one, cap), cap), what
    lane.flush()
    one.flush()
    assert lane.header() == one.header(), what
    tc.same_read(lane.read(), one.read(), what)
    return one


# ---- (a) five lanes, three calibrations, against the host module and single trackers --------------------------------------
@pytest.mark.parametrize('params', [tc.REFERENCE, tc.LOOSE], ids=['reference', 'loose'])
def test_lanes_match_host_and_single_trackers(ctx, params):
    """Lanes of 48, 31, 17, 1 and 0 pairs; the last is never active and its slot holds lane 0's records throughout.  The
    lane of one pair finishes no track under either parameter set (a track made in the only pair has length 1): it is
    compared through its state and header.  The calibration file of tracking video 0001 holds the default's numbers, so
    the third geometry is object frame 000006's (tests/_tracking_cases.py)."""
    score, high, iou, t_min = params
    seqs = [tc.lane_a(i) for i in range(5)]
    cals = [CALS[c['cal']] for c in tc.LANES_A]
    max_det, cap = tc.max_rows(*seqs), 4096
    lanes = dev.TrackerLanes(ctx, 5, cap, high, iou, t_min, score)
    assert lanes.stride == dev.ops.track_lanes_stride(cap)
    _run_lanes(ctx, lanes, seqs, cals, max_det, filler=seqs[0])
    for i in range(5):
        lane = lanes.lane(i)
        assert lane.header()['seq_pair'] == len(seqs[i])        # (its own pair numbering)
        _same_as_single(ctx, lane, seqs[i], cals[i], params, cap, max_det, 'lane %d' % i)
        got = dev.tracks_from_log(lane.read(), tc.frame_ids, tc.CLASSES)
        tc.same_tracks(got, tc.lane_a_tracks(i, params), 'lane %d' % i)
    h = lanes.lane(4).header()                                  # never active: as its reset left it
    assert h.pop('log_cap') == cap and not any(h.values())


# ---- (b) an inactive lane is untouched ---------------------------------------------------------------------------------
def test_inactive_lane_is_untouched(ctx):
    params, cap = tc.REFERENCE, 512
    seqs = [tc.sequence(31 + i, 6, n_obj=10) for i in range(3)]
    cals = [CALS['default'], CALS['object_file'], CALS['object_000006']]
    max_det = tc.max_rows(*seqs)
    lanes = dev.TrackerLanes(ctx, 3, cap, *params[1:], score_threshold=params[0])
    guard = ctx.zeros((4096,), np.uint8)                       # (allocated after the states)
    _run_lanes(ctx, lanes, seqs, cals, max_det, steps=4)
    before = lanes.d_states.download()
    recs, counts = zip(*[tc.pack(s[4:5], max_det) for s in seqs])
    assert all(c.sum() > 0 for c in counts)
    lanes.track_records(ctx.array(np.concatenate(recs)), ctx.array(np.concatenate(counts)), max_det,
                        [c.p2 for c in cals], [c.image_wh for c in cals], active=[1, 0, 1])
    after = lanes.d_states.download()
    s = lanes.stride
    assert before.shape == (3 * s,)
    assert np.array_equal(after[s:2 * s], before[s:2 * s])
    for i in (0, 2):
        assert not np.array_equal(after[i * s:(i + 1) * s], before[i * s:(i + 1) * s])
        assert lanes.lane(i).header()['seq_pair'] == 5
    assert lanes.lane(1).header()['seq_pair'] == 4
    assert not guard.download().any()
    # and the lane goes on from there as if the step had not been
    lanes.track_records(ctx.array(np.concatenate(recs)), ctx.array(np.concatenate(counts)), max_det,
                        [c.p2 for c in cals], [c.image_wh for c in cals], active=[0, 1, 0])
    _same_as_single(ctx, lanes.lane(1), seqs[1][:5], cals[1], params, cap, max_det, 'lane 1')


# ---- (c) the chunk seam ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_lanes', [17, 33])
def test_chunk_seam(ctx, n_lanes):
    params, cap = (0.1, 0.3, 0.005, 1), 256
    seqs = [tc.sequence(400 + i, 4, n_obj=4) for i in range(n_lanes)]
    names = ('default', 'object_file', 'object_000006')
    cals = [CALS[names[i % 3]] for i in range(n_lanes)]
    max_det = tc.max_rows(*seqs)
    lanes = dev.TrackerLanes(ctx, n_lanes, cap, *params[1:], score_threshold=params[0])
    _run_lanes(ctx, lanes, seqs, cals, max_det)
    for i in (0, 15, 16, 32):
        if i < n_lanes:
            assert sum(len(p[2]) for p in seqs[i]) > 0
            _same_as_single(ctx, lanes.lane(i), seqs[i], cals[i], params, cap, max_det, 'lane %d of %d' % (i, n_lanes))
            got = dev.tracks_from_log(lanes.lane(i).read(), tc.frame_ids, tc.CLASSES)
            want = tc.host_tracks(seqs[i], cals[i], params)
            assert len(want) > 0
            tc.same_tracks(got, want, 'lane %d of %d' % (i, n_lanes))


# ---- (d) one lane ends and starts again mid-stream -----------------------------------------------------------------------
def test_lane_ends_and_restarts_mid_stream(ctx):
    params, cap = tc.LOOSE, 2048
    long0, long2 = tc.sequence(51, 20, n_obj=12, empty=(7,)), tc.sequence(52, 20, n_obj=12)
    first, second = tc.sequence(53, 10, n_obj=12), tc.sequence(54, 8, n_obj=12, empty=(2,))
    cals = [CALS['default'], CALS['object_file'], CALS['object_000006']]
    second_cal = CALS['default']                               # the lane's next video comes with another calibration
    max_det = tc.max_rows(long0, long2, first, second)
    lanes = dev.TrackerLanes(ctx, 3, cap, *params[1:], score_threshold=params[0])
    packed = {n: tc.pack(s, max_det) for n, s in (('0', long0), ('2', long2), ('a', first), ('b', second))}
    ended = None
    for k in range(20):
        if k == 10:                 # lane 1's video is over: its tracks are read and the lane starts again
            lane = lanes.lane(1)
            lane.flush()
            ended = dev.tracks_from_log(lane.read(), tc.frame_ids, tc.CLASSES)
            lane.reset()
        src, j = ('a', k) if k < 10 else ('b', k - 10)
        on = k < 10 or j < len(second)
        recs = np.stack([packed['0'][0][k], packed[src][0][j if on else 0], packed['2'][0][k]])
        counts = np.stack([packed['0'][1][k], packed[src][1][j if on else 0], packed['2'][1][k]])
        lanes.track_records(ctx.array(recs), ctx.array(counts), max_det,
                            [cals[0].p2, (cals[1] if k < 10 else second_cal).p2, cals[2].p2],
                            [cals[0].image_wh, (cals[1] if k < 10 else second_cal).image_wh, cals[2].image_wh],
                            active=[True, on, True])
    want = [tc.host_tracks(long0, cals[0], params), tc.host_tracks(first, cals[1], params),
            tc.host_tracks(second, second_cal, params), tc.host_tracks(long2, cals[2], params)]
    assert all(len(w) > 0 for w in want)
    tc.same_tracks(ended, want[1], 'lane 1, first sequence')
    for i, w, what in ((0, want[0], 'lane 0'), (1, want[2], 'lane 1, second sequence'), (2, want[3], 'lane 2')):
        lanes.lane(i).flush()
        tc.same_tracks(dev.tracks_from_log(lanes.lane(i).read(), tc.frame_ids, tc.CLASSES), w, what)


# ---- (e) overflow stays in its lane --------------------------------------------------------------------------------------
def test_overflow_stays_in_its_lane(ctx):
    params, cap = (0.1, 0.0, 0.005, 1), 8
    big, small = tc.sequence(4, 20), tc.sequence(61, 2, n_obj=2)
    assert 0 < sum(len(p[2]) for p in small) <= cap            # (every detection of it may enter the log)
    cals = [CALS['default'], CALS['object_file']]
    max_det = tc.max_rows(big, small)
    lanes = dev.TrackerLanes(ctx, 2, cap, *params[1:], score_threshold=params[0])
    guard = ctx.zeros((4096,), np.uint8)
    _run_lanes(ctx, lanes, [big, small], cals, max_det, filler=big)
    lanes.lane(0).flush()
    with pytest.raises(RuntimeError, match='capacity'):
        lanes.lane(0).read()
    h = lanes.lane(0).header()
    assert h['n_log'] > cap and h['status'] & dev.STATUS_OVERFLOW
    # the status word is the single tracker's
    one = _single(ctx, big, cals[0], params, cap, max_det)
    one.flush()
    assert one.header() == h
    want = tc.host_tracks(small, cals[1], params)
    assert len(want) > 0
    _same_as_single(ctx, lanes.lane(1), small, cals[1], params, cap, max_det, 'lane 1')
    assert lanes.lane(1).header()['status'] == 0
    tc.same_tracks(dev.tracks_from_log(lanes.lane(1).read(), tc.frame_ids, tc.CLASSES), want, 'lane 1')
    assert not guard.download().any()


def test_arguments(ctx):
    lanes = dev.TrackerLanes(ctx, 2, 64)
    recs, counts = ctx.zeros((2, 2, 4, 17), np.float32), ctx.zeros((2, 2), np.int32)
    p2s, whs = [CALS['default'].p2] * 2, [CALS['default'].image_wh] * 2
    with pytest.raises(ValueError):
        lanes.track_records(recs, counts, 4, p2s, whs, active=[1])
    with pytest.raises(ValueError):
        lanes.track_records(recs, counts, 4, p2s[:1], whs)
    with pytest.raises(Exception):
        lanes.track_records(recs, counts, 129, p2s, whs)
    with pytest.raises(ValueError):
        dev.Tracker(ctx, 64, d_state=ctx.empty((64,), np.uint8))
    lanes.track_records(recs, counts, 4, p2s, whs)             # both keyframes empty: the skip rule, per lane
    assert [lanes.lane(i).header()['seq_pair'] for i in range(2)] == [1, 1]
    assert [lanes.lane(i).header()['frame_num'] for i in range(2)] == [0, 0]
