"""The IoU tracker of the temporal module on the device, with the host module's own interfaces
(dodt_amd.core.dt_evaluator_utils encode_tracking_dets, track_through_ious): numpy and dicts in, the same lists
of dicts out, the encoding and the tracking in HIP (dodt_amd/csrc/tracking.hip).

Tracker owns one sequence's device state.  The pipeline runs the same kernels on its detection records in place
(FramePairPipeline(tracker=...), tracks_so_far(), end_sequence()); these wrappers are what the tests compare with
the host module and the reference's goldens.

KalmanTracker / kf_pipeline: the Kalman-filter variant (dodt_amd.experiments.video_detection_kf.kf_pipeline) the same
way -- the IoU matrix, the optimal assignment, the filter and the track lists in HIP (dodt_amd/csrc/kalman.hip), the
host function's arguments in and its list of kalman_tracker.Tracker objects out.
VelocityTracker / interpolate_by_track: the velocity-extrapolating greedy IoU tracker
(dodt_amd.experiments.video_detection_iou.interpolate_by_track) the same way -- the IoU matrix, the greedy walk, the
predictions and the track lists in HIP (dodt_amd/csrc/velocity_track.hip), the host function's arguments in and its list of
track dicts out.
KalmanTrackerLanes / VelocityTrackerLanes: several sequences of those two trackers side by side, as TrackerLanes for
the IoU tracker -- one state per lane in one buffer, every lane one pair further per call.
"""
import numpy as np

from dodt_amd import device, ops

MAX_ROWS = 128                  # rows per encoded list (dodt_track_*: max_det <= 128)
TRK_COLS, K1_COLS = 23, 16      # encoded track item (KITTI row + offsets), keyframe-1 row
STATUS_OVERFLOW = 1

# the state buffer (tracking.hip: Header, Active, prev_off, prev_k1, Finished[cap], LogEntry[cap])
_HDR = ('n_active', 'n_slots', 'n_log', 'n_fin', 'frame_num', 'seq_pair', 'status', 'has_prev',
        'prev_pair', 'prev_nL', 'prev_n1', 'log_cap')
_HDR_BYTES = 64
_FIN_OFF = _HDR_BYTES + 2 * MAX_ROWS * 32 + 2 * MAX_ROWS * 7 * 4 + MAX_ROWS * K1_COLS * 4
_FIN_WORDS, _LOG_WORDS = 4, 28


class Tracker(object):
    """One sequence's tracker state on the device (track_through_ious' tracks_active / tracks_finished, and a log
    of every detection that entered a track).  log_capacity bounds the log and the finished list; running past it
    raises when the tracks are read.  Every launch goes on `ctx` (default: the state's context).  d_state: None -- the
    tracker allocates its state --, or a view of ops.track_state_bytes(log_capacity) bytes that holds it (a lane of
    TrackerLanes)."""

    def __init__(self, ctx=None, log_capacity=65536, high_threshold=0.5, iou_threshold=0.005, t_min=3,
                 score_threshold=0.1, d_state=None):
        self.ctx = ctx or device.default_context()
        self.cap = int(log_capacity)
        if self.cap < 1:
            raise ValueError('log_capacity must be >= 1')
        self.high, self.iou, self.t_min = float(high_threshold), float(iou_threshold), int(t_min)
        self.score_threshold = float(score_threshold)
        nbytes = ops.track_state_bytes(self.cap)
        assert nbytes == _FIN_OFF + self.cap * 4 * (_FIN_WORDS + _LOG_WORDS), 'state layout'
        if d_state is not None and d_state.nbytes < nbytes:
            raise ValueError('d_state: %d bytes, the state needs %d' % (d_state.nbytes, nbytes))
        self.d_state = self.ctx.empty((nbytes,), np.uint8) if d_state is None else d_state
        self.reset()

    def reset(self, ctx=None):
        """Start a new sequence."""
        ops.track_reset(ctx or self.ctx, self.d_state, self.cap)

    def flush(self, ctx=None):
        """Finish the remaining active tracks (the end of track_through_ious)."""
        ops.track_flush(ctx or self.ctx, self.d_state, self.high, self.t_min)

    def track_records(self, d_records, d_counts, n_pairs, max_det, p2, image_wh, ctx=None):
        """Encode and track n_pairs record pairs (n_pairs, 2, max_det, 17), continuing the sequence."""
        ops.track_pairs(ctx or self.ctx, self.d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh,
                        self.score_threshold, self.high, self.iou, self.t_min)

    def track_encoded(self, d_track, d_ious, d_counts, n_pairs, max_rows, ctx=None):
        ops.track_encoded(ctx or self.ctx, self.d_state, d_track, d_ious, d_counts, n_pairs, max_rows, self.high,
                          self.iou, self.t_min)

    def header(self):
        h = self.d_state.offset(0, (len(_HDR),), np.int32).download()
        return dict(zip(_HDR, (int(v) for v in h)))

    def read(self):
        """Download the finished tracks (synchronous on the state's context): a list of (start_frame, max_score
        (float32), log rows (k, 28) int32 in trajectory order) -- a log row is [slot, pair, keyframe, row index,
        16-col KITTI row, offsets (7), pad] with the floats as their int32 bits.  Raises RuntimeError if the log
        overflowed."""
        h = self.header()
        if h['status'] & STATUS_OVERFLOW:
            raise RuntimeError('tracker: log capacity %d exceeded (%d log entries, %d finished tracks needed)'
                               % (self.cap, h['n_log'], h['n_fin']))
        n_fin, n_log = h['n_fin'], h['n_log']
        fin = self.d_state.offset(_FIN_OFF, (max(n_fin, 1), _FIN_WORDS), np.int32).download()[:n_fin]
        log_off = _FIN_OFF + self.cap * 4 * _FIN_WORDS
        log = self.d_state.offset(log_off, (max(n_log, 1), _LOG_WORDS), np.int32).download()[:n_log]
        order = np.argsort(log[:, 0], kind='stable')
        slots = log[order, 0]
        out = []
        for slot, start, length, score_bits in fin:
            lo, hi = np.searchsorted(slots, slot, 'left'), np.searchsorted(slots, slot, 'right')
            rows = log[order[lo:hi]]
            if len(rows) != length:
                raise RuntimeError('tracker: track %d has %d log entries, length %d' % (slot, len(rows), length))
            out.append((int(start), np.array(score_bits, np.int32).view(np.float32)[()], rows))
        return out


class TrackerLanes(object):
    """n_lanes tracker states in ONE device buffer, ops.track_lanes_stride(log_capacity) bytes apart: pair i of a step
    belongs to lane i (one video or camera each), and every lane advances in one launch triple (dodt_track_lanes).
    lane(i) is a Tracker over lane i's slice: reset / flush / header / read as on a state of its own."""

    def __init__(self, ctx=None, n_lanes=1, log_capacity=65536, high_threshold=0.5, iou_threshold=0.005, t_min=3,
                 score_threshold=0.1):
        self.ctx = ctx or device.default_context()
        self.n_lanes, self.cap = int(n_lanes), int(log_capacity)
        if self.n_lanes < 1:
            raise ValueError('n_lanes must be >= 1')
        if self.cap < 1:
            raise ValueError('log_capacity must be >= 1')
        self.high, self.iou, self.t_min = float(high_threshold), float(iou_threshold), int(t_min)
        self.score_threshold = float(score_threshold)
        self.stride = ops.track_lanes_stride(self.cap)
        nbytes = ops.track_state_bytes(self.cap)
        self.d_states = self.ctx.empty((self.n_lanes * self.stride,), np.uint8)
        self.lanes = [Tracker(self.ctx, self.cap, self.high, self.iou, self.t_min, self.score_threshold,
                              d_state=self.d_states.offset(i * self.stride, (nbytes,), np.uint8))
                      for i in range(self.n_lanes)]

    def lane(self, i):
        return self.lanes[i]

    def track_records(self, d_records, d_counts, max_det, p2s, image_whs, active=None, ctx=None):
        """Encode and track one step: d_records (n_lanes, 2, max_det, 17), d_counts (n_lanes, 2), lane i taking pair i
        under p2s[i] and image_whs[i]; active: None, or one truth value per lane -- a lane that is not active keeps
        its state (and its pair numbering) as it is."""
        ops.track_lanes(ctx or self.ctx, self.d_states, self.stride, self.n_lanes, d_records, d_counts, max_det, p2s,
                        image_whs, self.score_threshold, self.high, self.iou, self.t_min, active=active)


def _floats(rows, a, b):
    return np.ascontiguousarray(rows[:, a:b]).view(np.float32)


# ---- the Kalman-filter tracker (dodt_amd/csrc/kalman.hip) ---------------------------------------------------------------
KF_MAX_LIVE = 256               # live tracks at the start of a keyframe
KF_STATUS_LOG, KF_STATUS_LIVE, KF_STATUS_SOLVER = 1, 2, 4
# the state buffer (kalman.hip: KfHeader, KfTrack[256 + 128], the kept keyframe-1 rows, KfTrack[cap], KfLog[cap])
_KF_HDR = ('n_live', 'next_id', 'n_log', 'n_fin', 'keyframe', 'status', 'log_cap', 'n_k1')
KF_TRACK = np.dtype([('id', '<i4'), ('hits', '<i4'), ('no_losses', '<i4'), ('last_kf', '<i4'), ('x', '<f8', (8,)),
                     ('P', '<f8', (4, 2, 2)), ('det', '<f8', (12,))])
KF_LOG = np.dtype([('id', '<i4'), ('keyframe', '<i4'), ('kind', '<i4'), ('row', '<i4'), ('det', '<f8', (12,))])
_KF_LIVE_OFF = _HDR_BYTES
_KF_K1_OFF = _KF_LIVE_OFF + (KF_MAX_LIVE + MAX_ROWS) * KF_TRACK.itemsize
_KF_FIN_OFF = _KF_K1_OFF + MAX_ROWS * K1_COLS * 4
_POS = [3, 4, 5]


class KalmanTracker(object):
    """One sequence's Kalman-filter tracker state on the device (video_detection_kf.kf_pipeline's live / done lists and
    a log of every real and coasting entry of a track).  Limits: 128 detections per keyframe, 256 live tracks at the
    start of a keyframe, log_capacity log entries and finished tracks; running past one raises when the state is read.
    Every launch goes on `ctx` (default: the state's context)."""

    def __init__(self, ctx=None, sigma_l=0.0, iou_threshold=0.1, max_age=3, min_hits=3, L=10.0, R_scaler=1.0 / 16,
                 log_capacity=8192, d_state=None):
        self.ctx = ctx or device.default_context()
        self.cap = int(log_capacity)
        if self.cap < 1:
            raise ValueError('log_capacity must be >= 1')
        self.params = dict(sigma_l=float(sigma_l), iou_threshold=float(iou_threshold), max_age=int(max_age),
                           min_hits=int(min_hits), L=float(L), R_scaler=float(R_scaler))
        nbytes = ops.kf_state_bytes(self.cap)
        assert KF_TRACK.itemsize == 304 and KF_LOG.itemsize == 112
        assert nbytes == _KF_FIN_OFF + self.cap * (KF_TRACK.itemsize + KF_LOG.itemsize), 'state layout'
        if d_state is not None and d_state.nbytes < nbytes:
            raise ValueError('d_state: %d bytes, the state needs %d' % (d_state.nbytes, nbytes))
        self.d_state = self.ctx.empty((nbytes,), np.uint8) if d_state is None else d_state
        self.pending_ego = None         # (track_records: the last pair's own motion, the next keyframe's association)
        self.reset()

    def reset(self, ctx=None):
        """Start a new sequence: ids from 0."""
        ops.kf_reset(ctx or self.ctx, self.d_state, self.cap)
        self.pending_ego = None

    def flush(self, calib42, ctx=None):
        """The end of kf_pipeline: the keyframe-1 rows track_records kept are the final keyframe, then the live tracks
        with hits >= min_hits are finished."""
        ego = None if self.pending_ego is None else ops.kf_ego_rows([self.pending_ego])[0]
        ops.kf_flush(ctx or self.ctx, self.d_state, ego, calib42, self.params)
        self.pending_ego = None

    def track_keyframes(self, d_rows, d_counts, n_keyframes, max_rows, ego, calib42, ctx=None):
        """n_keyframes encoded lists, continuing the sequence: d_rows (n, max_rows, 16) float64 (boxes2d 4:8, boxes3d
        8:15, score 15), d_counts (n,); ego[k]: (trans, matrix, delta) from the keyframe before k to k, or None."""
        ops.kf_track_keyframes(ctx or self.ctx, self.d_state, d_rows, d_counts, n_keyframes, max_rows,
                               ops.kf_ego_rows(ego), calib42, self.params)

    def track_records(self, d_records, d_counts, n_pairs, max_det, p2, image_wh, ego, calib42, score_threshold=0.1,
                      ctx=None):
        """Encode n_pairs record pairs (n_pairs, 2, max_det, 17) and track them: pair j's keyframe-0 rows are the next
        keyframe of the sequence, the last pair's keyframe-1 rows wait for flush().  ego[j]: pair j's own motion
        (trans, matrix, delta) from its keyframe 0 to its keyframe 1, or None -- the association of the keyframe
        AFTER it."""
        ego = list(ego)
        if len(ego) != int(n_pairs):
            raise ValueError('track_records: one ego entry per pair')
        if n_pairs == 0:
            return
        into = [self.pending_ego] + ego[:-1]
        ops.kf_track_pairs(ctx or self.ctx, self.d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh,
                           score_threshold, ops.kf_ego_rows(into), calib42, self.params)
        self.pending_ego = ego[-1]

    def header(self):
        h = self.d_state.offset(0, (len(_KF_HDR),), np.int32).download()
        return dict(zip(_KF_HDR, (int(v) for v in h)))

    def used_bytes(self):
        """The state's bytes that mean something (header, live tracks, kept rows, finished tracks, log), downloaded:
        what two equal histories leave equal."""
        h = self.header()
        n_k1 = max(h['n_k1'], 0)
        parts = [(0, _HDR_BYTES), (_KF_LIVE_OFF, h['n_live'] * KF_TRACK.itemsize), (_KF_K1_OFF, n_k1 * K1_COLS * 4),
                 (_KF_FIN_OFF, min(h['n_fin'], self.cap) * KF_TRACK.itemsize),
                 (_KF_FIN_OFF + self.cap * KF_TRACK.itemsize, min(h['n_log'], self.cap) * KF_LOG.itemsize)]
        return [self.d_state.offset(off, (n,), np.uint8).download() for off, n in parts if n > 0]

    def read(self):
        """Download (synchronous on the state's context): (finished tracks, KF_TRACK records in finishing order; the log,
        KF_LOG records in writing order).  Raises RuntimeError if a limit was exceeded."""
        h = self.header()
        if h['status'] & KF_STATUS_LIVE:
            raise RuntimeError('kalman tracker: more than %d live tracks' % KF_MAX_LIVE)
        if h['status'] & KF_STATUS_LOG:
            raise RuntimeError('kalman tracker: log capacity %d exceeded (%d log entries, %d finished tracks needed)'
                               % (self.cap, h['n_log'], h['n_fin']))
        if h['status'] & KF_STATUS_SOLVER:
            raise RuntimeError('kalman tracker: an IoU matrix without a finite assignment (NaN boxes)')
        n_fin, n_log = h['n_fin'], h['n_log']
        fin = self.d_state.offset(_KF_FIN_OFF, (max(n_fin, 1) * KF_TRACK.itemsize,), np.uint8).download()
        log = self.d_state.offset(_KF_FIN_OFF + self.cap * KF_TRACK.itemsize, (max(n_log, 1) * KF_LOG.itemsize,),
                                  np.uint8).download()
        return fin.view(KF_TRACK)[:n_fin], log.view(KF_LOG)[:n_log]


class _KindLanes(object):
    """n_lanes states of one tracker kind in ONE device buffer, `stride` bytes apart: pair i of a step belongs to lane i
    (one video or camera each), and every lane advances by one pair in one launch triple per ops.KIND_LANES_CHUNK lanes.
    lane(i) is the kind's single tracker over lane i's slice: reset / flush / header / used_bytes / read as on a state
    of its own, and its pending_ego -- the lane's last active pair's own motion, which associates the lane's next
    keyframe.  track_records() is the only way to advance the lanes."""

    def _init_lanes(self, ctx, n_lanes, log_capacity, score_threshold, stride, nbytes, make_lane, d_states=None):
        """stride, nbytes: the kind's ops entries for them; make_lane(ctx, view): its single tracker over `view`;
        d_states: None -- the object allocates the buffer --, or n_lanes * stride bytes (or more) that hold the states."""
        self.ctx = ctx or device.default_context()
        self.n_lanes, self.cap = int(n_lanes), int(log_capacity)
        if self.n_lanes < 1:
            raise ValueError('n_lanes must be >= 1')
        if self.cap < 1:
            raise ValueError('log_capacity must be >= 1')
        self.score_threshold = float(score_threshold)
        self.stride = stride(self.cap)
        if d_states is not None and d_states.nbytes < self.n_lanes * self.stride:
            raise ValueError('d_states: %d bytes, %d lanes need %d' % (d_states.nbytes, self.n_lanes,
                                                                      self.n_lanes * self.stride))
        self.d_states = self.ctx.empty((self.n_lanes * self.stride,), np.uint8) if d_states is None else d_states
        self.lanes = [make_lane(self.ctx, self.d_states.offset(i * self.stride, (nbytes(self.cap),), np.uint8))
                      for i in range(self.n_lanes)]
        self.params = self.lanes[0].params

    def lane(self, i):
        return self.lanes[i]

    def track_records(self, d_records, d_counts, max_det, p2s, image_whs, egos, calibs, active=None, ctx=None):
        """Encode and track one step: d_records (n_lanes, 2, max_det, 17), d_counts (n_lanes, 2), lane i taking pair i
        under p2s[i], image_whs[i] and calibs[i] (42, ops.temporal_calib).  egos[i]: pair i's own motion (trans, matrix,
        delta) from its keyframe 0 to its keyframe 1, or None -- the association of lane i's NEXT keyframe; this
        keyframe is associated under the one the lane's previous active pair brought.  active: None, or one truth value
        per lane -- a lane that is not active keeps its state and its pending_ego, and its ego entry is ignored."""
        egos = list(egos)
        if len(egos) != self.n_lanes:
            raise ValueError('track_records: one ego entry per lane')
        if active is not None and len(active) != self.n_lanes:
            raise ValueError('track_records: active has %d entries for %d lanes' % (len(active), self.n_lanes))
        on = [True] * self.n_lanes if active is None else [bool(a) for a in active]
        into = [ln.pending_ego if a else None for ln, a in zip(self.lanes, on)]
        self._track_lanes(ctx or self.ctx, self.d_states, self.stride, self.n_lanes, d_records, d_counts, max_det, p2s,
                          image_whs, ops.kf_ego_rows(into), calibs, self.score_threshold, self.params, active=on)
        for ln, a, e in zip(self.lanes, on, egos):
            if a:
                ln.pending_ego = e


class KalmanTrackerLanes(_KindLanes):
    """_KindLanes of KalmanTracker states (dodt_kf_track_lanes)."""

    def __init__(self, ctx=None, n_lanes=1, sigma_l=0.0, iou_threshold=0.1, max_age=3, min_hits=3, L=10.0,
                 R_scaler=1.0 / 16, log_capacity=8192, score_threshold=0.1, d_states=None):
        self._init_lanes(ctx, n_lanes, log_capacity, score_threshold, ops.kf_lanes_stride, ops.kf_state_bytes,
                         lambda c, view: KalmanTracker(c, sigma_l, iou_threshold, max_age, min_hits, L, R_scaler,
                                                       log_capacity=log_capacity, d_state=view), d_states)

    def _track_lanes(self, *args, **kw):
        ops.kf_track_lanes(*args, **kw)


def kf_log_det(entry, stride):
    """A log entry's detection as the host's dict (the pipeline's keyframe rows carry nothing else)."""
    d = entry['det']
    return {'frame_id': int(entry['keyframe']) * stride, 'boxes3d': np.array(d[0:7], np.float64),
            'boxes2d': np.array(d[7:11], np.float64), 'scores': float(d[11])}


def kf_tracks_from_log(fin, log, stride, frame_total=None, real_det=None, L=10.0, R_scaler=1.0 / 16):
    """KalmanTracker.read() -> kf_pipeline's result: kalman_tracker.Tracker objects (id, hits, no_losses, x_state (8,1),
    P (8,8), box, dets).  dets is rebuilt from the track's log entries as the host builds it: a real entry is
    real_det(keyframe, row) (default: kf_log_det), a coasting one a copy of the entry before it at the logged position,
    one stride on (at most frame_total - 1); interpolation_detections fills the frames in between."""
    import copy

    from dodt_amd.experiments.video_detection_kf import interpolation_detections
    from dodt_amd.utils.kalman_tracker import Tracker as KfTrack
    order = np.argsort(log['id'], kind='stable')
    ids = log['id'][order]
    out = []
    for f in fin:
        trk = KfTrack()
        trk.L, trk.R_scaler = float(L), float(R_scaler)
        trk.update_R()
        trk.id, trk.hits, trk.no_losses = int(f['id']), int(f['hits']), int(f['no_losses'])
        trk.x_state = np.array(f['x'], np.float64).reshape(8, 1)
        trk.P = np.zeros((8, 8))
        for b in range(4):
            trk.P[2 * b:2 * b + 2, 2 * b:2 * b + 2] = f['P'][b]
        trk.box = [float(trk.x_state[i, 0]) for i in (0, 2, 4, 6)]
        lo, hi = np.searchsorted(ids, f['id'], 'left'), np.searchsorted(ids, f['id'], 'right')
        for e in log[order[lo:hi]]:
            if e['kind'] == 0:
                det = kf_log_det(e, stride) if real_det is None else real_det(int(e['keyframe']), int(e['row']))
            else:
                if not trk.dets:
                    raise RuntimeError('kalman tracker: track %d starts with a coasting entry' % trk.id)
                det = copy.deepcopy(trk.dets[-1])
                det['boxes3d'][_POS] = e['det'][3:6]
                det['frame_id'] = det['frame_id'] + stride
                if frame_total is not None:
                    det['frame_id'] = min(det['frame_id'], frame_total - 1)
                det['is_virtual'] = True
            if trk.dets:
                interpolation_detections(trk, det, stride)
            else:
                trk.dets.append(det)
        out.append(trk)
    return out


def _kf_check_detections(detections, stride):
    """What kf_pipeline refuses before anything reaches the device -> (rows (n, max_rows, 16) float64, counts (n,))."""
    n = len(detections)
    max_rows = max([1] + [len(f) for f in detections])
    if max_rows > MAX_ROWS:
        raise ValueError('at most %d detections per keyframe' % MAX_ROWS)
    rows = np.zeros((n, max_rows, K1_COLS), np.float64)
    counts = np.zeros((n,), np.int32)
    for k, frame in enumerate(detections):
        for i, det in enumerate(frame):
            if int(det['frame_id']) != k * stride:
                raise ValueError('kf_pipeline: detection %d of keyframe %d has frame_id %r, not %d'
                                 % (i, k, det['frame_id'], k * stride))
            rows[k, i, 4:8] = np.asarray(det['boxes2d'], np.float64).reshape(4)
            rows[k, i, 8:15] = np.asarray(det['boxes3d'], np.float64).reshape(7)
            rows[k, i, 15] = float(det['scores'])
        counts[k] = len(frame)
    return rows, counts


def kf_pipeline(ego, calib, detections, stride, frame_total, sigma_l, iou_threshold, max_age=3, min_hits=3, ctx=None):
    """video_detection_kf.kf_pipeline on the device (dodt_kf_track_keyframes): the host function's arguments, the same
    list of Tracker objects whose dets hold the caller's detection dicts.  ego(k * stride - stride, k * stride) is called
    once per keyframe k >= 1; a detection whose frame_id is not its keyframe's k * stride is a ValueError.  Boxes go
    to the device as float64."""
    rows, counts = _kf_check_detections(detections, stride)
    n = len(detections)
    if n == 0:
        return []
    ctx = ctx or device.default_context()
    egos = [None] + [ego(k * stride - stride, k * stride) for k in range(1, n)]
    calib42 = ops.temporal_calib(calib[0], calib[1])
    cap = max(1, min(n * (KF_MAX_LIVE + MAX_ROWS), int(counts.sum()) * (int(max_age) + 2)))
    tr = KalmanTracker(ctx, sigma_l, iou_threshold, max_age, min_hits, log_capacity=cap)
    tr.track_keyframes(ctx.array(rows), ctx.array(counts), n, rows.shape[1], egos, calib42)
    tr.flush(calib42)
    fin, log = tr.read()
    return kf_tracks_from_log(fin, log, stride, frame_total, real_det=lambda k, i: detections[k][i])


# ---- the velocity-extrapolating IoU tracker (dodt_amd/csrc/velocity_track.hip) -----------------------------------------
VT_STATUS_LOG, VT_STATUS_LIVE, VT_STATUS_IOU = 1, 2, 4
VT_HAS_SPEED, VT_CUT = 1, 2             # VT_TRACK['flags']
# the state buffer (velocity_track.hip: VtHeader, VtTrack[256 + 128], the kept keyframe-1 rows, VtTrack[cap], VtLog[cap]);
# the header's fields are the Kalman state's
VT_TRACK = np.dtype([('id', '<i4'), ('n_dets', '<i4'), ('extend_len', '<i4'), ('flags', '<i4'), ('max_score', '<f8'),
                     ('speed', '<f8', (3,)), ('det', '<f8', (13,))])
VT_LOG = np.dtype([('id', '<i4'), ('keyframe', '<i4'), ('kind', '<i4'), ('row', '<i4'), ('det', '<f8', (13,))])
_VT_LIVE_OFF = _HDR_BYTES
_VT_K1_OFF = _VT_LIVE_OFF + (KF_MAX_LIVE + MAX_ROWS) * VT_TRACK.itemsize
_VT_FIN_OFF = _VT_K1_OFF + MAX_ROWS * K1_COLS * 4
_XZR = [3, 5, 6]


VT_MAX_STEP = 4096              # stride and extend_len: the bound of the device's prediction loop


def _vt_check_params(stride, extend_len):
    if not 1 <= int(stride) <= VT_MAX_STEP:
        raise ValueError('stride must be 1..%d' % VT_MAX_STEP)
    if not 1 <= int(extend_len) <= VT_MAX_STEP:
        raise ValueError('extend_len must be 1..%d (the host function empties a coasting track at 0)' % VT_MAX_STEP)


class VelocityTracker(object):
    """One sequence's velocity-extrapolating IoU tracker state on the device (video_detection_iou.interpolate_by_track's
    active / finished lists and a log of every real and predicted entry of a track).  Limits: 128 detections per
    keyframe, 256 live tracks at the start of a keyframe, log_capacity log entries and finished tracks; running past
    one, or an IoU that is not finite, raises when the state is read.  Every launch goes on `ctx` (default: the state's
    context)."""

    def __init__(self, ctx=None, sigma_l=0.1, sigma_h=0.5, sigma_iou=0.1, t_min=3, extend_len=3, stride=1,
                 log_capacity=8192, d_state=None):
        _vt_check_params(stride, extend_len)
        self.cap = int(log_capacity)
        if self.cap < 1:
            raise ValueError('log_capacity must be >= 1')
        self.ctx = ctx or device.default_context()
        self.params = dict(sigma_l=float(sigma_l), sigma_h=float(sigma_h), sigma_iou=float(sigma_iou), t_min=int(t_min),
                           extend_len=int(extend_len), stride=int(stride))
        nbytes = ops.vt_state_bytes(self.cap)
        assert VT_TRACK.itemsize == 152 and VT_LOG.itemsize == 120
        assert nbytes == _VT_FIN_OFF + self.cap * (VT_TRACK.itemsize + VT_LOG.itemsize), 'state layout'
        if d_state is not None and d_state.nbytes < nbytes:
            raise ValueError('d_state: %d bytes, the state needs %d' % (d_state.nbytes, nbytes))
        self.d_state = self.ctx.empty((nbytes,), np.uint8) if d_state is None else d_state
        self.pending_ego = None         # (track_records: the last pair's own motion, the next keyframe's association)
        self.reset()

    def reset(self, ctx=None):
        """Start a new sequence: ids from 0."""
        ops.vt_reset(ctx or self.ctx, self.d_state, self.cap)
        self.pending_ego = None

    def flush(self, calib42, ctx=None):
        """The end of interpolate_by_track's loop: the keyframe-1 rows track_records kept are the final keyframe, then
        the live tracks with max_score >= sigma_h and >= t_min entries are finished."""
        ego = None if self.pending_ego is None else ops.kf_ego_rows([self.pending_ego])[0]
        ops.vt_flush(ctx or self.ctx, self.d_state, ego, calib42, self.params)
        self.pending_ego = None

    def track_keyframes(self, d_rows, d_counts, n_keyframes, max_rows, ego, calib42, ctx=None, box_f64=None,
                        score_f64=None):
        """n_keyframes encoded lists, continuing the sequence: d_rows (n, max_rows, 16) float32 or float64 (boxes2d 4:8,
        boxes3d 8:15, score 15), d_counts (n,); ego[k]: (trans, matrix, delta) from the keyframe before k to k, or
        None.  box_f64 / score_f64: the dtype the host holds boxes3d / the scores in (None: the rows')."""
        ops.vt_track_keyframes(ctx or self.ctx, self.d_state, d_rows, d_counts, n_keyframes, max_rows,
                               ops.kf_ego_rows(ego), calib42, self.params, box_f64, score_f64)

    def track_records(self, d_records, d_counts, n_pairs, max_det, p2, image_wh, ego, calib42, score_threshold=0.1,
                      ctx=None):
        """Encode n_pairs record pairs (n_pairs, 2, max_det, 17) and track them: pair j's keyframe-0 rows are the next
        keyframe of the sequence, the last pair's keyframe-1 rows wait for flush().  ego[j]: pair j's own motion
        (trans, matrix, delta) from its keyframe 0 to its keyframe 1, or None -- the association of the keyframe
        AFTER it."""
        ego = list(ego)
        if len(ego) != int(n_pairs):
            raise ValueError('track_records: one ego entry per pair')
        if n_pairs == 0:
            return
        into = [self.pending_ego] + ego[:-1]
        ops.vt_track_pairs(ctx or self.ctx, self.d_state, d_records, d_counts, n_pairs, max_det, p2, image_wh,
                           score_threshold, ops.kf_ego_rows(into), calib42, self.params)
        self.pending_ego = ego[-1]

    def header(self):
        h = self.d_state.offset(0, (len(_KF_HDR),), np.int32).download()
        return dict(zip(_KF_HDR, (int(v) for v in h)))

    def used_bytes(self):
        """The state's bytes that mean something (header, live tracks, kept rows, finished tracks, log), downloaded:
        what two equal histories leave equal."""
        h = self.header()
        n_k1 = max(h['n_k1'], 0)
        parts = [(0, _HDR_BYTES), (_VT_LIVE_OFF, h['n_live'] * VT_TRACK.itemsize), (_VT_K1_OFF, n_k1 * K1_COLS * 4),
                 (_VT_FIN_OFF, min(h['n_fin'], self.cap) * VT_TRACK.itemsize),
                 (_VT_FIN_OFF + self.cap * VT_TRACK.itemsize, min(h['n_log'], self.cap) * VT_LOG.itemsize)]
        return [self.d_state.offset(off, (n,), np.uint8).download() for off, n in parts if n > 0]

    def read(self):
        """Download (synchronous on the state's context): (finished tracks, VT_TRACK records in finishing order; the log,
        VT_LOG records in writing order).  Raises RuntimeError if a limit was exceeded or an IoU was not finite."""
        h = self.header()
        if h['status'] & VT_STATUS_LIVE:
            raise RuntimeError('velocity tracker: more than %d live tracks' % KF_MAX_LIVE)
        if h['status'] & VT_STATUS_LOG:
            raise RuntimeError('velocity tracker: log capacity %d exceeded (%d log entries, %d finished tracks needed)'
                               % (self.cap, h['n_log'], h['n_fin']))
        if h['status'] & VT_STATUS_IOU:
            raise RuntimeError('velocity tracker: an IoU that is not finite (NaN boxes)')
        n_fin, n_log = h['n_fin'], h['n_log']
        fin = self.d_state.offset(_VT_FIN_OFF, (max(n_fin, 1) * VT_TRACK.itemsize,), np.uint8).download()
        log = self.d_state.offset(_VT_FIN_OFF + self.cap * VT_TRACK.itemsize, (max(n_log, 1) * VT_LOG.itemsize,),
                                  np.uint8).download()
        return fin.view(VT_TRACK)[:n_fin], log.view(VT_LOG)[:n_log]


class VelocityTrackerLanes(_KindLanes):
    """_KindLanes of VelocityTracker states (dodt_vt_track_lanes)."""

    def __init__(self, ctx=None, n_lanes=1, sigma_l=0.1, sigma_h=0.5, sigma_iou=0.1, t_min=3, extend_len=3, stride=1,
                 log_capacity=8192, score_threshold=0.1, d_states=None):
        self._init_lanes(ctx, n_lanes, log_capacity, score_threshold, ops.vt_lanes_stride, ops.vt_state_bytes,
                         lambda c, view: VelocityTracker(c, sigma_l, sigma_h, sigma_iou, t_min, extend_len, stride,
                                                         log_capacity=log_capacity, d_state=view), d_states)

    def _track_lanes(self, *args, **kw):
        ops.vt_track_lanes(*args, **kw)


def vt_log_det(entry, stride, dtype=np.float32, classes=None):
    """A log entry's detection (det: boxes3d, boxes2d, score, class index) as the host's dict; classes: the names
    'info' is filled from (None: no 'info')."""
    d = entry['det']
    det = {'frame_id': int(entry['keyframe']) * stride, 'boxes2d': np.array(d[7:11], dtype),
           'boxes3d': np.array(d[0:7], dtype), 'score': dtype(d[11])}
    if classes is not None:
        det['info'] = np.array([classes[int(d[12])], '-1', '-1', '-10.0'])
    return det


def vt_tracks_from_log(fin, log, stride, extend_len, frame_num, real_det=None, dtype=np.float32, classes=None):
    """VelocityTracker.read() -> interpolate_by_track's result: track dicts 'dets', 'direction', 'max_score', 'speed',
    'extend_len'.  dets is rebuilt from the track's log entries with the host module's own functions: a real entry is
    real_det(keyframe, row) (default: vt_log_det in `dtype`, 'info' from `classes`), joined by interpolate_det (the frames in between); a
    predicted one a copy of the entry before it, one frame on, at the logged x, z, ry; a finished record whose
    predictions were cut loses its last extend_len entries.  max_score, speed and extend_len are the device's.  Then
    the two end extensions (extend_track_start, extend_track_end under frame_num)."""
    import copy

    from dodt_amd.experiments import video_detection_iou as host
    order = np.argsort(log['id'], kind='stable')
    ids = log['id'][order]
    out = []
    for f in fin:
        trk = {'dets': [], 'direction': [], 'max_score': None, 'speed': [0.0, 0.0, 0.0], 'extend_len': 0}
        lo, hi = np.searchsorted(ids, f['id'], 'left'), np.searchsorted(ids, f['id'], 'right')
        for e in log[order[lo:hi]]:
            if e['kind'] == 0:
                det = (vt_log_det(e, stride, dtype, classes) if real_det is None
                       else real_det(int(e['keyframe']), int(e['row'])))
                if trk['dets']:
                    host.interpolate_det(trk, det)
                else:
                    trk['direction'] = [1 if det['boxes3d'][-1] > 0 else -1]
                trk['max_score'] = np.asarray(det['score']).dtype.type(f['max_score'])
                trk['dets'].append(det)
            else:
                if not trk['dets']:
                    raise RuntimeError('velocity tracker: track %d starts with a predicted entry' % int(f['id']))
                det = copy.deepcopy(trk['dets'][-1])
                det['frame_id'] += 1
                det['boxes3d'][_XZR] = e['det'][_XZR]
                trk['dets'].append(det)
        if f['flags'] & VT_CUT:
            trk['dets'] = trk['dets'][:-int(extend_len)]
        if len(trk['dets']) != int(f['n_dets']):
            raise RuntimeError('velocity tracker: track %d has %d entries in the log, %d on the device'
                               % (int(f['id']), len(trk['dets']), int(f['n_dets'])))
        if f['flags'] & VT_HAS_SPEED:
            trk['speed'] = np.array(f['speed'], trk['dets'][-1]['boxes3d'].dtype)
        trk['extend_len'] = int(f['extend_len'])
        out.append(trk)
    out = host.extend_track_start(out, stride)
    return host.extend_track_end(out, stride, frame_num)


def _vt_check_detections(detections, stride):
    """What interpolate_by_track refuses before anything reaches the device -> (rows (n, max_rows, 16), counts (n,),
    box_f64, score_f64): the dtypes the host computes in -- boxes3d arithmetic in float32 if every boxes3d is, score
    comparisons in float32 if every score is --; the rows are float32 if both are, else float64 (which holds float32
    values exactly)."""
    n = len(detections)
    max_rows = max([1] + [len(f) for f in detections])
    if max_rows > MAX_ROWS:
        raise ValueError('at most %d detections per keyframe' % MAX_ROWS)
    dets = [d for f in detections for d in f]
    box_f64 = not all(np.asarray(d['boxes3d']).dtype == np.float32 for d in dets)
    score_f64 = not all(np.asarray(d['score']).dtype == np.float32 for d in dets)
    rows = np.zeros((n, max_rows, K1_COLS), np.float64 if box_f64 or score_f64 else np.float32)
    counts = np.zeros((n,), np.int32)
    for k, frame in enumerate(detections):
        for i, det in enumerate(frame):
            if int(det['frame_id']) != k * stride:
                raise ValueError('interpolate_by_track: detection %d of keyframe %d has frame_id %r, not %d'
                                 % (i, k, det['frame_id'], k * stride))
            rows[k, i, 4:8] = np.asarray(det['boxes2d']).reshape(4)
            rows[k, i, 8:15] = np.asarray(det['boxes3d']).reshape(7)
            rows[k, i, 15] = det['score']
        counts[k] = len(frame)
    return rows, counts, box_f64, score_f64


def interpolate_by_track(ego, calib, detections, stride, frame_num, sigma_l, sigma_h, sigma_iou, t_min, extend_len,
                         ctx=None):
    """video_detection_iou.interpolate_by_track on the device (dodt_vt_track_keyframes): the host function's arguments,
    the same list of track dicts whose real entries are the caller's detection dicts.  ego(k * stride - stride,
    k * stride) is called once per keyframe k >= 1.  A detection whose frame_id is not its keyframe's k * stride, more
    than 128 detections in a keyframe, extend_len and stride outside 1..4096 are ValueErrors.  The device computes speed
    and predictions in float32 if every boxes3d array is float32, else in float64, and compares scores in float32 if
    every score is float32, else in float64 -- as the host does on those arrays."""
    _vt_check_params(stride, extend_len)
    rows, counts, box_f64, score_f64 = _vt_check_detections(detections, stride)
    n = len(detections)
    if n == 0:
        return []
    ctx = ctx or device.default_context()
    egos = [None] + [ego(k * stride - stride, k * stride) for k in range(1, n)]
    calib42 = ops.temporal_calib(calib[0], calib[1])
    per_kf = min(int(stride), int(extend_len)) + 1
    cap = max(1, min(n * (KF_MAX_LIVE * per_kf + MAX_ROWS), int(counts.sum()) * (int(extend_len) + 2)))
    tr = VelocityTracker(ctx, sigma_l, sigma_h, sigma_iou, t_min, extend_len, stride, log_capacity=cap)
    tr.track_keyframes(ctx.array(rows), ctx.array(counts), n, rows.shape[1], egos, calib42, box_f64=box_f64,
                       score_f64=score_f64)
    tr.flush(calib42)
    fin, log = tr.read()
    return vt_tracks_from_log(fin, log, stride, extend_len, frame_num, real_det=lambda k, i: detections[k][i])


def _label_item(frame_id, row, classes, offsets=None):
    """The host's encode_tracking_dets item of one encoded row (16 float32, class index in col 0)."""
    d = {'frame_id': str(frame_id), 'info': [classes[int(row[0])], '-1', '-1', '-10.0'],
         'boxes2d': np.array(row[4:8], np.float32), 'boxes3d': np.array(row[8:15], np.float32),
         'scores': np.float32(row[15])}
    if offsets is not None:
        d['offsets'] = np.array(offsets, np.float32)
    return d


def tracks_from_log(tracks, frame_ids, classes):
    """Tracker.read() of a records-driven sequence -> the host's tracks_finished: dicts 'trajectory', 'max_score',
    'start_frame' whose detections are encode_tracking_dets' items.  frame_ids(pair, keyframe) -> the frame id."""
    out = []
    for start, score, rows in tracks:
        v, off = _floats(rows, 4, 20), _floats(rows, 20, 27)
        traj = [_label_item(frame_ids(int(r[1]), int(r[2])), v[i], classes, off[i]) for i, r in enumerate(rows)]
        out.append({'trajectory': traj, 'max_score': score, 'start_frame': start})
    return out


def _pack_records(pairs):
    """[(frame_0, frame_1, records (n,17))] -> (n_pairs, 2, max_det, 17) float32, counts (n_pairs, 2): each keyframe's
    rows (mark column 16) in order, as the host splits them."""
    split = []
    for _, _, rec in pairs:
        rec = np.asarray(rec, dtype=np.float32).reshape(-1, 17)
        split.append([rec[rec[:, -1] == 0], rec[rec[:, -1] == 1]])
    max_det = max([1] + [len(s) for sp in split for s in sp])
    if max_det > MAX_ROWS:
        raise ValueError('at most %d rows per keyframe' % MAX_ROWS)
    recs = np.zeros((len(pairs), 2, max_det, 17), np.float32)
    counts = np.zeros((len(pairs), 2), np.int32)
    for j, sp in enumerate(split):
        for f in range(2):
            recs[j, f, :len(sp[f])] = sp[f]
            counts[j, f] = len(sp[f])
    return recs, counts, max_det


def encode_tracking_dets(pairs, calib_p2, image_size, classes, threshold, ctx=None):
    """dt_evaluator_utils.encode_tracking_dets on the device (dodt_track_encode): the same (dets_for_track,
    dets_for_ious) lists of dicts."""
    ctx = ctx or device.default_context()
    dets_for_track, dets_for_ious = [], [{}]
    if len(pairs) == 0:
        return dets_for_track, dets_for_ious
    recs, counts, max_det = _pack_records(pairs)
    n = len(pairs)
    d_trk, d_k1 = ctx.empty((n, MAX_ROWS, TRK_COLS), np.float32), ctx.empty((n, MAX_ROWS, K1_COLS), np.float32)
    d_cnt = ctx.empty((n, 4), np.int32)
    ops.track_encode(ctx, ctx.array(recs), ctx.array(counts), n, max_det, calib_p2, image_size, threshold, d_trk,
                     d_k1, d_cnt)
    trk, k1, cnt = d_trk.download(), d_k1.download(), d_cnt.download()
    for j, (frame_0, frame_1, _) in enumerate(pairs):
        n_t, n_1, skip = cnt[j, :3]
        if skip:
            continue
        dets_for_track.append([_label_item(frame_0, trk[j, i, :16], classes, trk[j, i, 16:23]) for i in range(n_t)])
        dets_for_ious.append([_label_item(frame_1, k1[j, i], classes) for i in range(n_1)])
    return dets_for_track, dets_for_ious


def track_through_ious(dets_for_track, dets_for_ious, high_threshold, iou_threshold, t_min, ctx=None):
    """dt_evaluator_utils.track_through_ious on the device (dodt_track_encoded): the same finished tracks, whose
    trajectories hold the caller's detection dicts, copied as the host copies them (a merged keyframe-1 detection
    gets 'offsets' = its own box).  Boxes and scores are taken as float32."""
    ctx = ctx or device.default_context()
    n = len(dets_for_track)
    if n == 0:
        return []

    def ious_of(j):
        f = dets_for_ious[j + 1] if j + 1 < len(dets_for_ious) else []
        return f if isinstance(f, list) else []
    rows = max([1] + [len(f) for f in dets_for_track] + [len(ious_of(j)) for j in range(n)])
    if rows > MAX_ROWS:
        raise ValueError('at most %d detections per list' % MAX_ROWS)
    trk = np.zeros((n, rows, TRK_COLS), np.float32)
    k1 = np.zeros((n, rows, K1_COLS), np.float32)
    counts = np.zeros((n, 2), np.int32)
    for j in range(n):
        for i, d in enumerate(dets_for_track[j]):
            trk[j, i, 8:15] = np.asarray(d['boxes3d'], np.float32)
            trk[j, i, 15] = np.float32(d['scores'])
            trk[j, i, 16:23] = np.asarray(d['offsets'], np.float32)
        for i, d in enumerate(ious_of(j)):
            k1[j, i, 8:15] = np.asarray(d['boxes3d'], np.float32)
            k1[j, i, 15] = np.float32(d['scores'])
        counts[j] = len(dets_for_track[j]), len(ious_of(j))
    tr = Tracker(ctx, log_capacity=max(1, int(counts.sum())), high_threshold=high_threshold,
                 iou_threshold=iou_threshold, t_min=t_min)
    tr.track_encoded(ctx.array(trk), ctx.array(k1), ctx.array(counts), n, rows)
    tr.flush()
    out = []
    for start, score, log in tr.read():
        traj = []
        for _, pair, kf, i in log[:, :4]:
            if kf == 0:
                traj.append(dict(dets_for_track[pair][i]))
            else:
                d = dict(ious_of(pair)[i])
                d['offsets'] = d['boxes3d']
                traj.append(d)
        out.append({'trajectory': traj, 'max_score': score, 'start_frame': start})
    return out
