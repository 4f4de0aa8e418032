"""Shared by the lanes tests of the Kalman and the velocity tracker (tests/test_gpu_kalman_lanes.py,
tests/test_gpu_velocity_lanes.py): the two kinds behind one small description, the lanes' calibrations and ego motions,
synthetic records (tests/_tracking_cases.py's generator, at most 10 objects), the drivers -- a single tracker fed one
pair per call, the yardstick, and a lanes object fed one step per call after a plan -- and the two comparisons of a lane
with a single tracker.  The test bodies are here, one function per numbered case, so that both kinds run the same
checks.  No GPU is needed to import it."""
import numpy as np
import pytest

import _kalman_cases as K
import _tracking_cases as tc
from dodt_amd import config, ops
from dodt_amd import tracking as dev

MAX_DET = 16            # rows per keyframe of the packed records (the sequences have at most 10 objects)
GAP = 6                 # frames between a pair's keyframes as the ego motions see it: K.moving(0, 6) is 1.8 m and 0.06 rad,
                        # enough to decide a gate (see lanes_really_differ)
CAP = 1024


class Kind(object):
    """One tracker kind: its single class, its lanes class and the parameters the tests run it with."""

    def __init__(self, name, single, lanes, params, stride, state_bytes, track_lanes):
        self.name, self._single, self._lanes, self.params = name, single, lanes, params
        self.stride, self.state_bytes, self.track_lanes = stride, state_bytes, track_lanes

    def single(self, ctx, cap=CAP, d_state=None):
        return self._single(ctx, log_capacity=cap, d_state=d_state, **self.params)

    def lanes(self, ctx, n, cap=CAP, d_states=None):
        return self._lanes(ctx, n, log_capacity=cap, d_states=d_states, **self.params)


def kalman():
    return Kind('kalman', dev.KalmanTracker, dev.KalmanTrackerLanes, dict(sigma_l=0.3, iou_threshold=0.1, min_hits=2),
                ops.kf_lanes_stride, ops.kf_state_bytes, ops.kf_track_lanes)


def velocity():
    return Kind('velocity', dev.VelocityTracker, dev.VelocityTrackerLanes,
                dict(sigma_l=0.25, sigma_h=0.5, sigma_iou=0.1, t_min=2, extend_len=3, stride=2),
                ops.vt_lanes_stride, ops.vt_state_bytes, ops.vt_track_lanes)


class Cal(object):
    """A lane's calibration: p2 and image size for the encode, (R0_rect, Tr_velo_to_cam) for the association."""

    def __init__(self, p2, wh, rt):
        self.p2, self.wh, self.rt = np.asarray(p2, np.float64), tuple(wh), rt
        self.c42 = ops.temporal_calib(*rt)


def cals():
    """CALIB_KITTI, CALIB_ID (both under KITTI's projection and image size) and object frame 000006's."""
    o6 = tc.calibrations()['object_000006']
    return [Cal(config.KITTI_P2, config.KITTI_IMAGE_WH, K.CALIB_KITTI),
            Cal(config.KITTI_P2, config.KITTI_IMAGE_WH, K.CALIB_ID),
            Cal(o6.p2, o6.image_wh, (np.asarray(o6.r0_rect, np.float64), np.asarray(o6.tr_velo_to_cam, np.float64)))]


def sideways(a, b):
    """Another motion than K.moving: to the side and up, turning the other way."""
    n = b - a
    yaw = -0.015 * n
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([0.05 * n, 0.2 * n, 0.01 * n]), np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), yaw


def ego_of(motion, j):
    """Pair j's own motion under `motion` (None: parked)."""
    return None if motion is None else motion(GAP * j, GAP * j + GAP)


def records(seed, n_pairs, n_obj=8):
    """-> (recs (n_pairs, 2, MAX_DET, 17) float32, counts (n_pairs, 2))."""
    pairs = tc.sequence(seed, n_pairs, n_obj=n_obj)
    assert tc.max_rows(pairs) <= MAX_DET
    return tc.pack(pairs, MAX_DET)


def feed_single(ctx, tracker, seq, cal, motion, first=0, dtype=np.float32):
    """The yardstick: `tracker` fed the pairs of `seq` one track_records call each; pair j of the call is pair first + j
    of the tracker's sequence (for its ego motion)."""
    recs, counts = seq
    for j in range(len(recs)):
        tracker.track_records(ctx.array(recs[j:j + 1].astype(dtype)), ctx.array(counts[j:j + 1]), 1, recs.shape[2],
                              cal.p2, cal.wh, [ego_of(motion, first + j)], cal.c42)
    return tracker


def step_lanes(ctx, lanes, slots, lane_cals, egos, active, dtype=np.float32):
    """One lanes call: slots[i] = (records (2, max_det, 17), counts (2,)) of lane i's slot."""
    recs = np.stack([s[0] for s in slots]).astype(dtype)
    cnts = np.stack([s[1] for s in slots]).astype(np.int32)
    lanes.track_records(ctx.array(recs), ctx.array(cnts), recs.shape[2], [c.p2 for c in lane_cals],
                        [c.wh for c in lane_cals], egos, [c.c42 for c in lane_cals], active=active)


def run_plan(ctx, lanes, seqs, lane_cals, motions, plan, filler, dtype=np.float32, pass_all_true=False):
    """plan[k][i]: the pair of seqs[i] lane i takes at step k, or None -- the lane is inactive and its slot holds
    filler[k] = (records, counts) of some valid pair."""
    for k, row in enumerate(plan):
        slots = [filler[k] if j is None else (seqs[i][0][j], seqs[i][1][j]) for i, j in enumerate(row)]
        egos = [ego_of(K.moving, 99) if j is None else ego_of(motions[i], j) for i, j in enumerate(row)]
        active = [j is not None for j in row]
        step_lanes(ctx, lanes, slots, lane_cals, egos, None if all(active) and not pass_all_true else active, dtype)


def same_bytes(a, b, what):
    """used_bytes() of a lane equals used_bytes() of the single tracker byte for byte."""
    xa, xb = a.used_bytes(), b.used_bytes()
    assert len(xa) == len(xb), what
    for i, (x, y) in enumerate(zip(xa, xb)):
        assert x.tobytes() == y.tobytes(), '%s: part %d of the used bytes differs' % (what, i)


def same_flushed(a, b, cal, what):
    """After both are flushed, header() and read() are equal."""
    a.flush(cal.c42)
    b.flush(cal.c42)
    assert a.header() == b.header(), what
    for x, y in zip(a.read(), b.read()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), what


def both(a, b, cal, what):
    same_bytes(a, b, what)
    same_flushed(a, b, cal, what)


def fresh_header(cap):
    return dict(n_live=0, next_id=0, n_log=0, n_fin=0, keyframe=0, status=0, log_cap=cap, n_k1=-1)


# ---- 1 -----------------------------------------------------------------------------------------------------------------
LANE_PAIRS = (12, 7, 1, 0)
LANE_MOTIONS = (K.moving, None, sideways, None)


def lanes_against_singles(ctx, kind, dtype):
    """Four lanes of 12, 7, 1 and 0 pairs under three calibrations and three ego motions; the last lane is never active
    and its slot holds lane 0's records throughout."""
    C = cals()
    lane_cals = [C[0], C[1], C[2], C[0]]
    seqs = [records(200 + i, n) for i, n in enumerate(LANE_PAIRS)]
    lanes = kind.lanes(ctx, 4)
    plan = [[k if k < n else None for n in LANE_PAIRS] for k in range(max(LANE_PAIRS))]
    filler = [(seqs[0][0][k], seqs[0][1][k]) for k in range(len(plan))]
    run_plan(ctx, lanes, seqs, lane_cals, LANE_MOTIONS, plan, filler, dtype)
    assert lanes.lane(3).header() == fresh_header(CAP)
    assert [lanes.lane(i).header()['keyframe'] for i in range(4)] == list(LANE_PAIRS)
    assert lanes.lane(0).header()['n_log'] > 12 and lanes.lane(0).header()['n_live'] > 0
    for i in range(4):
        single = feed_single(ctx, kind.single(ctx), seqs[i], lane_cals[i], LANE_MOTIONS[i], dtype=dtype)
        both(lanes.lane(i), single, lane_cals[i], 'lane %d' % i)
    assert lanes.lane(3).header() == fresh_header(CAP)          # (a flush of nothing: as reset left it)
    assert max(lanes.lane(i).header()['n_fin'] for i in range(3)) > 0      # (tracks were followed, not only begun)


# ---- 2 -----------------------------------------------------------------------------------------------------------------
def lanes_really_differ(ctx, kind):
    """A property of the INPUTS of case 1: lane 0's pairs under lane 1's ego motion, and under lane 1's calibration,
    leave other state bytes on a single tracker than under lane 0's own -- the motions and calibrations decide
    associations.  Without this, case 1 would pass with the lane index ignored."""
    C = cals()
    seq = records(200, LANE_PAIRS[0])

    def state(cal, motion):
        return b''.join(x.tobytes() for x in feed_single(ctx, kind.single(ctx), seq, cal, motion).used_bytes())
    own = state(C[0], LANE_MOTIONS[0])
    assert own == state(C[0], LANE_MOTIONS[0])                  # (the same history: the same bytes)
    assert own != state(C[0], LANE_MOTIONS[1])
    assert own != state(C[1], LANE_MOTIONS[0])
    # and lane 2's inputs from lane 0's: its projection and image size change what the encode keeps
    assert own != state(C[2], LANE_MOTIONS[0])


# ---- 3 -----------------------------------------------------------------------------------------------------------------
def pack_frames(frames, score_key):
    """Keyframe lists of detection dicts (boxes3d [h,w,l,x,y,z,ry]) -> the records of their overlapping pairs: pair j is
    keyframes (j, j + 1), the shifted box of a keyframe-0 row its own box."""
    n = len(frames) - 1
    recs, cnts = np.zeros((n, 2, MAX_DET, 17), np.float32), np.zeros((n, 2), np.int32)
    for j in range(n):
        for f in range(2):
            for i, d in enumerate(frames[j + f]):
                h, w, l, x, y, z, ry = (float(v) for v in d['boxes3d'])
                recs[j, f, i, :9] = [x, y, z, l, w, h, ry, float(d[score_key]), 0]
                recs[j, f, i, 9:16] = recs[j, f, i, :7]
                recs[j, f, i, 16] = f
            cnts[j, f] = len(frames[j + f])
    return recs, cnts


def encoded_lists(ctx, recs, cnts, cal, score_threshold=0.1):
    """What the trackers see of those records: every pair's encoded keyframe-0 rows and the last pair's keyframe-1 rows,
    (k, 16) float32 each."""
    n = len(recs)
    d_trk, d_k1 = ctx.empty((n, 128, 23), np.float32), ctx.empty((n, 128, 16), np.float32)
    d_cnt = ctx.empty((n, 4), np.int32)
    ops.track_encode(ctx, ctx.array(recs), ctx.array(cnts), n, recs.shape[2], cal.p2, cal.wh, score_threshold, d_trk, d_k1,
                     d_cnt)
    trk, k1, cnt = d_trk.download(), d_k1.download(), d_cnt.download()
    return [trk[j, :cnt[j, 3], :16] for j in range(n)] + [k1[n - 1, :cnt[n - 1, 1]]]


def scenario_in_lane_1(ctx, kind, recs, cnts, cal, ego):
    """The scenario's pairs in lane 1 of three, lanes 0 and 2 busy with videos of their own (lane 2's ends early);
    ego(j): pair j's own motion.  -> the lanes object (which owns the buffer), lane 1 flushed."""
    C = cals()
    n = len(recs)
    side = [records(700, n), records(701, n - 2)]
    lanes = kind.lanes(ctx, 3)
    for k in range(n):
        on2 = k < n - 2
        slots = [(side[0][0][k], side[0][1][k]), (recs[k], cnts[k]),
                 (side[1][0][k], side[1][1][k]) if on2 else (recs[k], cnts[k])]
        step_lanes(ctx, lanes, slots, [C[2], cal, C[1]], [ego_of(sideways, k), ego(k), None], [True, True, on2])
    assert [lanes.lane(i).header()['keyframe'] for i in range(3)] == [n, n, n - 2]
    lanes.lane(1).flush(cal.c42)
    return lanes


# ---- 4 -----------------------------------------------------------------------------------------------------------------
def inactive_lane_is_untouched(ctx, kind):
    C = cals()
    lane_cals = [C[0], C[1], C[2]]
    motions = [K.moving, sideways, K.moving]
    seqs = [records(300 + i, 5) for i in range(3)]
    stride, guard = kind.stride(CAP), 4096
    buf = ctx.zeros((3 * stride + guard,), np.uint8)
    lanes = kind.lanes(ctx, 3, d_states=buf)
    assert lanes.stride == stride and lanes.d_states is buf
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[k, k, k] for k in range(4)], None)
    before = buf.download()
    pending = lanes.lane(1).pending_ego
    assert pending is not None and pending is not lanes.lane(0).pending_ego
    # valid records in every slot, lane 1's its own next pair
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[4, None, 4]], [(seqs[1][0][4], seqs[1][1][4])])
    after = buf.download()
    cut = [slice(i * stride, (i + 1) * stride) for i in range(3)]
    assert np.array_equal(after[cut[1]], before[cut[1]])
    assert not np.array_equal(after[cut[0]], before[cut[0]]) and not np.array_equal(after[cut[2]], before[cut[2]])
    assert not after[3 * stride:].any()
    assert lanes.lane(1).pending_ego is pending
    assert lanes.lane(0).pending_ego[0].tobytes() == ego_of(K.moving, 4)[0].tobytes()
    # the paused lane goes on as if the step had not been
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[None, 4, None]], [(seqs[0][0][4], seqs[0][1][4])])
    for i in range(3):
        single = feed_single(ctx, kind.single(ctx), seqs[i], lane_cals[i], motions[i])
        both(lanes.lane(i), single, lane_cals[i], 'lane %d' % i)
    assert not buf.download()[3 * stride:].any()


# ---- 5 -----------------------------------------------------------------------------------------------------------------
def more_lanes_than_a_chunk(ctx, kind):
    """2 chunk + 1 lanes of 3 pairs each, a seed per lane, lane i inactive at step i mod 3 (four steps).  Then, beyond
    that shape, ONE more step in which the middle chunk has no active lane while the lanes of the other two chunks take
    a fourth pair: an all-inactive chunk between two working ones is the case in which "launches nothing, changes
    nothing" can be told from "the call did nothing" -- so the lanes outside the middle chunk end with 4 pairs, and every
    lane is compared with a single tracker fed exactly the pairs the lane took."""
    chunk = ops.KIND_LANES_CHUNK
    n = 2 * chunk + 1
    C = cals()
    lane_cals = [C[i % 3] for i in range(n)]
    motions = [(K.moving, None, sideways)[(i // 3) % 3] for i in range(n)]
    seqs = [records(400 + i, 4, n_obj=6) for i in range(n)]
    lanes = kind.lanes(ctx, n, cap=512)
    # ragged: lane i is inactive at step i mod 3, so four steps bring every lane three pairs
    plan, at = [], [0] * n
    for k in range(4):
        row = []
        for i in range(n):
            if k % 3 == i % 3 and k < 3:
                row.append(None)
            else:
                row.append(at[i])
                at[i] += 1
        plan.append(row)
    assert all(sorted(j for j in (row[i] for row in plan) if j is not None) == [0, 1, 2] for i in range(n))
    filler = [(seqs[0][0][0], seqs[0][1][0])] * 5
    run_plan(ctx, lanes, seqs, lane_cals, motions, plan, filler)
    # a step whose middle chunk has no active lane: nothing of that chunk's states changes
    before = lanes.d_states.download()
    mid = slice(chunk * lanes.stride, 2 * chunk * lanes.stride)
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[None if chunk <= i < 2 * chunk else 3 for i in range(n)]], filler)
    after = lanes.d_states.download()
    assert np.array_equal(after[mid], before[mid]) and not np.array_equal(after, before)
    # no active lane at all: nothing is launched, nothing changes, no pending ego moves
    pend = [ln.pending_ego for ln in lanes.lanes]
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[None] * n], filler)
    assert np.array_equal(lanes.d_states.download(), after)
    assert all(a is b for a, b in zip(pend, (ln.pending_ego for ln in lanes.lanes)))
    for i in range(n):
        fed = 3 if chunk <= i < 2 * chunk else 4
        single = feed_single(ctx, kind.single(ctx, 512), (seqs[i][0][:fed], seqs[i][1][:fed]), lane_cals[i], motions[i])
        both(lanes.lane(i), single, lane_cals[i], 'lane %d' % i)


# ---- 6 -----------------------------------------------------------------------------------------------------------------
def limits_stay_in_their_lane(ctx, kind):
    C = cals()
    lane_cals = [C[0], C[1], C[2]]
    motions = [K.moving, None, sideways]
    seqs = [records(500 + i, 6) for i in range(3)]
    lanes = kind.lanes(ctx, 3)
    small = 16
    lanes.lanes[0] = kind.single(ctx, small, d_state=lanes.lane(0).d_state)     # lane 0's state again, with a small log
    assert lanes.lane(0).header()['log_cap'] == small
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[k, k, k] for k in range(6)], None)
    assert lanes.lane(0).header()['n_log'] > small
    assert [lanes.lane(i).header()['status'] for i in (1, 2)] == [0, 0]
    with pytest.raises(RuntimeError, match='log capacity'):
        lanes.lane(0).read()
    for i in (1, 2):
        single = feed_single(ctx, kind.single(ctx), seqs[i], lane_cals[i], motions[i])
        both(lanes.lane(i), single, lane_cals[i], 'lane %d beside the overflowing one' % i)


def grid_records(n, shift=0.0):
    """One pair: n small boxes in keyframe 0 (no two touching, all inside KITTI's image), the same ones a little further
    in keyframe 1."""
    recs = np.zeros((1, 2, 128, 17), np.float32)
    for f in range(2):
        for i in range(n):
            recs[0, f, i, :9] = [-7.5 + (i % 16), 1.6, 30.0 + (i // 16) + shift + 0.1 * f, 0.5, 0.5, 1.0, 0.3,
                                 0.5 + i / 1000.0, 0]
            recs[0, f, i, 9:16] = recs[0, f, i, :7]
            recs[0, f, i, 16] = f
    return recs, np.array([[n, n]], np.int32)


def row_limit_beside_three(ctx, kind):
    """A lane fed 128 detections in a keyframe, the row limit, beside a lane fed 3."""
    C = cals()
    lane_cals = [C[0], C[0]]
    motions = [None, None]
    full = [grid_records(128), grid_records(128, 0.05)]
    three = [grid_records(3), grid_records(3, 0.05)]
    seqs = [tuple(np.concatenate(x) for x in zip(*full)), tuple(np.concatenate(x) for x in zip(*three))]
    lanes = kind.lanes(ctx, 2, cap=4096)
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[0, 0], [1, 1]], None)
    h = [lanes.lane(i).header() for i in range(2)]
    assert h[0]['n_log'] >= 256 and h[0]['n_k1'] == 128 and h[1]['n_k1'] == 3 and h[0]['status'] == h[1]['status'] == 0
    for i in range(2):
        single = feed_single(ctx, kind.single(ctx, 4096), seqs[i], lane_cals[i], motions[i])
        both(lanes.lane(i), single, lane_cals[i], 'lane %d' % i)


# ---- 7 -----------------------------------------------------------------------------------------------------------------
def ending_one_lane(ctx, kind):
    C = cals()
    lane_cals = [C[0], C[1], C[2]]
    motions = [K.moving, sideways, None]
    seqs = [records(600 + i, 6) for i in range(3)]
    second = records(650, 3)
    lanes = kind.lanes(ctx, 3)
    run_plan(ctx, lanes, seqs, lane_cals, motions, [[k, k, k] for k in range(3)], None)
    # lane 1's video ends in the middle of the run: it is what a single tracker makes of those three pairs
    first = feed_single(ctx, kind.single(ctx), (seqs[1][0][:3], seqs[1][1][:3]), lane_cals[1], motions[1])
    both(lanes.lane(1), first, lane_cals[1], 'lane 1, first video')
    lanes.lane(1).reset()
    assert lanes.lane(1).header() == fresh_header(CAP) and lanes.lane(1).pending_ego is None
    # its next video starts at id 0 and keyframe 0, under another calibration; the other lanes go on
    lane_cals[1], motions[1] = C[0], K.moving
    mixed = [seqs[0], second, seqs[2]]
    run_plan(ctx, lanes, mixed, lane_cals, motions, [[3 + k, k, 3 + k] for k in range(3)], None)
    for i in (0, 2):
        same_bytes(lanes.lane(i), feed_single(ctx, kind.single(ctx), seqs[i], lane_cals[i], motions[i]), 'lane %d' % i)
    fresh = feed_single(ctx, kind.single(ctx), second, lane_cals[1], motions[1])
    assert lanes.lane(1).header()['keyframe'] == 3
    both(lanes.lane(1), fresh, lane_cals[1], 'lane 1, second video')


# ---- 8 -----------------------------------------------------------------------------------------------------------------
def entry_refusals(ctx, kind):
    C = cals()
    n = 3
    stride, nbytes = kind.stride(CAP), kind.state_bytes(CAP)
    assert stride % 256 == 0 and nbytes <= stride < nbytes + 256
    lanes = kind.lanes(ctx, n)
    before = lanes.d_states.download()
    recs, cnts = ctx.zeros((n, 2, MAX_DET, 17), np.float32), ctx.zeros((n, 2), np.int32)
    good = dict(p2s=[C[0].p2] * n, whs=[C[0].wh] * n, egos=ops.kf_ego_rows([None] * n), c42=[C[0].c42] * n)

    def call(stride=stride, max_det=MAX_DET, active=None, **over):
        a = dict(good, **over)
        kind.track_lanes(ctx, lanes.d_states, stride, n, recs, cnts, max_det, a['p2s'], a['whs'], a['egos'], a['c42'],
                         0.1, lanes.params, active=active)
    for bad in (dict(stride=64), dict(stride=kind.state_bytes(1) - 8), dict(max_det=0), dict(max_det=129),
                dict(p2s=[C[0].p2] * (n - 1)), dict(whs=[C[0].wh] * (n + 1)), dict(egos=ops.kf_ego_rows([None] * 2)),
                dict(c42=[C[0].c42] * 2), dict(active=[True] * (n + 1))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        lanes.track_records(recs, cnts, MAX_DET, good['p2s'], good['whs'], [None] * (n - 1), good['c42'])
    with pytest.raises(ValueError):
        lanes.track_records(recs, cnts, MAX_DET, good['p2s'], good['whs'], [None] * n, good['c42'], active=[1, 0])
    assert np.array_equal(lanes.d_states.download(), before)
    with pytest.raises(ValueError):
        kind.lanes(ctx, 0)
    with pytest.raises(ValueError):
        kind.lanes(ctx, 2, d_states=ctx.zeros((stride,), np.uint8))
    call()                                                      # (what is not refused: three empty pairs)
    assert [lanes.lane(i).header()['keyframe'] for i in range(n)] == [1] * n
