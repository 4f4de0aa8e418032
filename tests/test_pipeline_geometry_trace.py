"""The geometry belongs to the step: the real FramePairPipeline over the recording stand-ins (tests/_pipeline_trace.py,
extended in tests/_geometry_trace.py), driven with a different calibration per step (pair mode) or per sequence
(sequence mode).  Every logged launch that takes a geometry argument -- bev_slices, project_anchors_f64 / _f32,
gather_project, img_preprocess, M and the tracker -- has to carry the calibration of the step or keyframe it belongs to:
the tail enqueued one call late, the look-ahead prep enqueued one call early, the carried keyframe's second
voxelisation.  What is refused is refused with nothing logged."""
import numpy as np
import pytest

import _geometry_trace as gt
import _pipeline_trace as tr

A, B, C = gt.real_calibrations()
TAIL_OPS = ('gather_project', 'project_anchors_f32')


def _p2_wh(t):
    """(p2, image_wh) of a logged launch that takes them as arguments."""
    at = {'project_anchors_f64': 5, 'gather_project': 5, 'project_anchors_f32': 4, 'track_records': 5}[t['op']]
    return t['args'][at], t['args'][at + 1]


def _carries(t, calib):
    p2, wh = _p2_wh(t)
    return np.array_equal(p2, calib.p2) and tuple(wh) == tuple(calib.image_wh)


class _Run(object):
    """Drives a pipeline and remembers, per API call, the part of the trace it enqueued and which step's tail that part
    holds."""

    def __init__(self, pipe, trace):
        self.pipe, self.trace = pipe, trace
        # (label, start, end, step whose tail this call enqueued or None, own step or None, calibration of host frames)
        self.calls = []
        self.pending = None
        self.step_calib = {}           # step -> the calibration of each of its samples
        self.points = {}               # id(points array) -> calibration of the frame
        self.images = {}               # id(image array) -> calibration

    def inputs(self, calibs):
        """Pair mode: ([points], [n], [images]) for samples of `calibs`."""
        frames = []
        for cal in calibs:
            for _ in range(self.pipe.fps):
                fr = gt.frame(self.pipe, cal)
                self.points[id(fr[0])], self.images[id(fr[2])] = cal, cal
                frames.append(fr)
        return [list(a) for a in zip(*frames)]

    def key(self, calib):
        fr = gt.frame(self.pipe, calib)
        self.points[id(fr[0])], self.images[id(fr[2])] = calib, calib
        return fr

    def call(self, label, fn, *args, step=None, calibs=None, **kw):
        start = len(self.trace)
        ret = fn(*args, **kw)
        tail_of = self.pending
        if step is not None:
            self.step_calib[step] = calibs
            self.pending = step
        elif label.startswith('finish'):
            self.pending = None
        else:
            tail_of = None
        self.calls.append((label, start, len(self.trace), tail_of, step, getattr(self, 'host_next', None)))
        return ret

    def check(self, uploads=()):
        """Every launch with a geometry argument against the step or keyframe it belongs to.  -> counts per kind."""
        pipe, seen = self.pipe, dict(prep=0, carried=0, tail=0, temporal=0, tracker=0, late=0, rows=0)
        ring_owner = {}                # id(point ring slot) -> calibration of the keyframe copied there
        frame_of_stream = {}           # stream -> calibration of the frame whose prep chain runs there
        for label, start, end, tail_of, own, host_cal in self.calls:
            tails = []
            for t in self.trace[start:end]:
                if t.get('event'):
                    continue
                op, args = t['op'], t['args']
                if op == 'bev_slices' and args[4] is not None:               # a frame's full prep
                    cal = self.points.get(id(args[0]), ring_owner.get(id(args[0].base)))
                    assert cal is not None and gt.bp_matches(args[2], cal), (label, 'bev_slices')
                    frame_of_stream[t['stream']] = cal
                    seen['prep'] += 1
                elif op == 'bev_slices':                                     # the carried keyframe, voxelised again
                    cal = ring_owner[id(args[0].base)]
                    assert gt.bp_matches(args[2], cal) and not hasattr(args[2], 'ego_motion'), (label, 'carried')
                    seen['carried'] += 1
                elif op == 'upload_async' and args[0].base in pipe.__dict__.get('pts_ring', ()):
                    ring_owner[id(args[0].base)] = host_cal
                elif op == 'gather_rows' and args[-1].base in pipe.__dict__.get('pts_ring', ()):
                    ring_owner[id(args[-1].base)] = self.points[id(args[0])]
                elif op == 'project_anchors_f64':
                    assert _carries(t, frame_of_stream[t['stream']]), (label, op)
                elif op == 'img_preprocess':
                    cal = frame_of_stream[t['stream']]
                    w, h = cal.image_wh
                    assert tuple(args[1]) == (h, w) and args[0].shape == (h, w, 3), (label, op)
                    if id(args[0]) in self.images:
                        assert self.images[id(args[0])] is cal
                elif op in TAIL_OPS:
                    tails.append(t)
                elif op == 'interpolate_pairs':
                    cals = self.step_calib[tail_of]
                    if 'd_calibs' in t['kw']:
                        assert len({c.key() for c in cals}) > 1 and 'calib' not in t['kw']
                        slot = tail_of % len(pipe.rec2)
                        assert t['kw']['d_calibs'] is pipe.cal2[slot] and t['kw']['d_recover'] is pipe.ego2[slot]
                        # ... whose rows were uploaded with the step's recover parameters, in the call that enqueued it
                        s0, e0 = [(s, e) for _, s, e, _, o, _ in self.calls if o == tail_of][0]
                        rows = [h for at, base, h in uploads if base is pipe.cal2[slot] and s0 <= at < e0]
                        ego = [at for at, base, h in uploads if base is pipe.ego2[slot] and s0 <= at < e0]
                        assert len(rows) == 1 and len(ego) == 1
                        assert np.array_equal(rows[0], np.stack([np.full(42, c.tr_velo_to_cam[0, 3]) for c in cals]))
                        seen['rows'] += 1
                    elif t['kw'].get('calib') is not None:
                        assert len({c.key() for c in cals}) == 1
                        assert np.array_equal(t['kw']['calib'], np.full(42, cals[0].tr_velo_to_cam[0, 3])), label
                    seen['temporal'] += 1
                elif op == 'track_records':
                    assert _carries(t, self.step_calib[tail_of][0]), (label, op)
                    seen['tracker'] += 1
            if tails:
                assert tail_of is not None, label
                cals = self.step_calib[tail_of]
                per_frame = len(tails) // pipe.nf
                assert per_frame * pipe.nf == len(tails)
                streams = {}
                for t in tails:         # per stream the frames in order; frame f runs on stream f % 2
                    streams.setdefault(t['stream'], []).append(t)
                for s, ts in streams.items():
                    frames = [f for f in range(pipe.nf) if tr.STREAMS[2 + f % 2] == s]
                    for i, t in enumerate(ts):
                        f = frames[i // per_frame]
                        assert _carries(t, cals[f // pipe.fps]), (label, t['op'], f)
                        seen['tail'] += 1
                if own is not None and self.step_calib[own][0].key() != cals[0].key():
                    seen['late'] += 1   # a tail enqueued by a call whose own step has another calibration
        return seen


# ---- pair mode ---------------------------------------------------------------------------------------------------------
PAIR_CALIBS = [None, B, C, B, A, C, C, B, A]        # by step; None: the constructor's (A)


@pytest.mark.parametrize('fused', ['1', '0'])
def test_pair_mode_every_step_its_own_calibration(monkeypatch, fused):
    monkeypatch.setenv('DODT_PIPE_FUSED_TAIL', fused)
    build, uploads = gt.install(monkeypatch)
    pipe, trace, _ = build()
    run = _Run(pipe, trace)
    heads = tr._heads(pipe)
    ins = [run.inputs([c or A]) for c in PAIR_CALIBS]
    early = 0
    for k, cal in enumerate(PAIR_CALIBS):
        la = None
        if k % 3 and k + 1 < len(PAIR_CALIBS):      # the next step announced, its calibration the fifth entry
            la = tuple(ins[k + 1]) + (None, PAIR_CALIBS[k + 1])
        before = len(trace)
        was_prepped = pipe.prepped == k
        run.call('run %d' % k, pipe.run, *ins[k], heads=heads, lookahead=la, calib=cal, step=k, calibs=[cal or A])
        if was_prepped:         # prepared one call early: this call enqueued no prep of its own step
            mine = [t for t in trace[before:] if t['op'] == 'bev_slices' and id(t['args'][0]) in map(id, ins[k][0])]
            assert not mine
            early += 1
        if k == 4:
            run.call('finish %d' % k, pipe.finish)
    run.call('finish', pipe.finish)
    seen = run.check(uploads)
    assert early >= 4
    assert seen['prep'] == 2 * len(PAIR_CALIBS)
    assert seen['tail'] == 2 * len(PAIR_CALIBS) * (1 if fused == '1' else 2)
    assert seen['late'] >= 5                          # tails enqueued by a call of another calibration
    assert not tr.races(pipe, trace)


def test_two_pairs_per_step_two_calibrations_with_temporal_module(monkeypatch):
    build, uploads = gt.install(monkeypatch)
    pipe, trace, _ = build(head_params=tr.HP, pairs_per_step=2, temporal=dict(n_frames=3))
    run = _Run(pipe, trace)
    steps = [[A, B], [C, C], None, [B, A], C]
    per_sample = [[A, A] if s is None else ([s, s] if not isinstance(s, list) else s) for s in steps]
    ins = [run.inputs(cs) for cs in per_sample]
    for k, s in enumerate(steps):
        la = tuple(ins[k + 1]) + (None, steps[k + 1]) if k in (1, 2) else None
        run.call('run %d' % k, pipe.run, *ins[k], lookahead=la, calib=s, recover=tr._recover(pipe, True), step=k,
                 calibs=per_sample[k])
    run.call('finish', pipe.finish)
    seen = run.check(uploads)
    assert seen['prep'] == 4 * len(steps) and seen['tail'] == 4 * len(steps)
    assert seen['temporal'] == len(steps) and seen['rows'] == 2      # steps 0 and 3 differ within the step
    # the default path uploads no rows
    assert sum(1 for _, base, _ in uploads if any(base is c for c in pipe.cal2)) == 2


def test_tracker_takes_the_sequences_calibration(monkeypatch):
    build, uploads = gt.install(monkeypatch)
    pipe, trace, _ = build(head_params=tr.HP, temporal=dict(n_frames=3), tracker={})
    run = _Run(pipe, trace)
    k = 0
    for cal in (B, None, C):
        for j in range(3):
            ins = run.inputs([cal or A])
            run.call('run %d' % k, pipe.run, *ins, calib=cal, recover=tr._recover(pipe, j == 1), step=k,
                     calibs=[cal or A])
            k += 1
        run.call('finish %d' % k, pipe.finish)
        pipe.end_sequence()
    seen = run.check(uploads)
    assert seen['tracker'] == 9 and seen['temporal'] == 9 and seen['rows'] == 0
    # inside a sequence the calibration stays
    ins = run.inputs([B])
    pipe.run(*ins, calib=B)
    n = len(trace)
    with pytest.raises(ValueError):
        pipe.run(*run.inputs([C]), calib=C)
    with pytest.raises(ValueError):
        pipe.run(*run.inputs([A]))
    assert len(trace) == n
    pipe.finish()
    pipe.end_sequence()
    pipe.run(*run.inputs([C]), calib=C)


def test_from_host_stages_each_image_at_its_own_size(monkeypatch):
    build, _ = gt.install(monkeypatch)
    pipe, trace, _ = build(image_wh_max=(1242, 376))
    run = _Run(pipe, trace)
    heads = tr._heads(pipe)
    cals = [C, None, B]
    for k, cal in enumerate(cals):
        la = ([object(), object()], [30000, 30000], [object(), object()], None, cals[k + 1]) if k == 0 else None
        n = len(trace)
        run.call('run %d' % k, pipe.run_from_host, [object(), object()], [30000, 30000], [object(), object()],
                 heads=heads, lookahead=la, calib=cal, step=k, calibs=[cal or A])
        if k == 0:
            assert pipe.stage[0][0][1].shape == (376, 1242, 3)
        # the image launches read the head of the staging buffer as (h, w, 3)
        for t in trace[n:]:
            if t['op'] == 'img_preprocess':
                assert t['args'][0].ptr == t['args'][0].base.ptr and t['args'][0].base.shape == (376, 1242, 3)
    run.call('finish', pipe.finish)
    # (host frames carry no array to tell the frames by: the prep launches are checked by their order on the stream)
    imgs = [t for t in trace if t['op'] == 'img_preprocess']
    want = [c for cal in (C, A, B) for c in [cal] * 2]
    assert [tuple(t['args'][1]) for t in imgs] == [(c.image_wh[1], c.image_wh[0]) for c in want]
    prj = [t for t in trace if t['op'] == 'project_anchors_f64']
    assert all(_carries(t, c) for t, c in zip(prj, want)) and len(prj) == 6
    bev = [t for t in trace if t['op'] == 'bev_slices']
    assert all(gt.bp_matches(t['args'][2], c) for t, c in zip(bev, want)) and len(bev) == 6
    tails = [t for t in trace if t['op'] in TAIL_OPS]
    assert all(_carries(t, c) for t, c in zip(tails, want)) and len(tails) == 6


def test_pair_mode_refusals_log_nothing(monkeypatch):
    build, _ = gt.install(monkeypatch)
    pipe, trace, _ = build(pairs_per_step=2)
    run = _Run(pipe, trace)
    heads = tr._heads(pipe) * 2
    n = len(trace)
    with pytest.raises(ValueError):                  # a list of the wrong length
        pipe.run(*run.inputs([B, B]), heads=heads, calib=[B])
    with pytest.raises(ValueError):
        pipe.run(*run.inputs([B, B]), heads=heads, calib=[B, B, B])
    with pytest.raises(ValueError):                  # an image of another sample's size
        pipe.run(*run.inputs([B, C]), heads=heads, calib=[C, B])
    with pytest.raises(ValueError):
        pipe.run(*run.inputs([B, B]), heads=heads)
    with pytest.raises(ValueError):                  # ... in the look-ahead
        pipe.run(*run.inputs([A, A]), heads=heads, lookahead=tuple(run.inputs([B, B])) + (None, [B, C]))
    with pytest.raises(ValueError):                  # a host image larger than image_wh_max (1242 x 375: C is smaller,
        big = gt.config.Calibration(B.p2, B.r0_rect, B.tr_velo_to_cam, (1241, 376))       # this one taller)
        pipe.run_from_host([object()] * 4, [1] * 4, [object()] * 4, heads=heads, calib=big)
    with pytest.raises(ValueError):
        pipe.run_from_host([object()] * 4, [1] * 4, [object()] * 4, heads=heads,
                           lookahead=([object()] * 4, [1] * 4, [object()] * 4, None, big))
    assert len(trace) == n and pipe.step_idx == 0
    # a look-ahead calibration that the next call does not bring
    nxt = run.inputs([B, C])
    pipe.run(*run.inputs([A, A]), heads=heads, lookahead=tuple(nxt) + (None, [B, C]))
    n = len(trace)
    for wrong in (None, [C, B], B):
        with pytest.raises(ValueError):
            pipe.run(*nxt, heads=heads, calib=wrong)
    assert len(trace) == n and pipe.step_idx == 1
    pipe.run(*nxt, heads=heads, calib=[gt.config.Calibration(*B), C])       # equal by value
    assert pipe.step_idx == 2
    with pytest.raises(ValueError):
        gt.pl.FramePairPipeline(pipe.ctx, pipe.cfg, {}, {}, image_wh_max=(1200, 375),
                                reuse_streams_of=pipe, bev_input_skip=False)


# ---- sequence mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(head_params=tr.HP, temporal=dict(n_frames=3), tracker={})],
                         ids=['injected', 'computed_temporal_tracker'])
@pytest.mark.parametrize('host', [False, True], ids=['device', 'from_host'])
def test_sequence_mode_every_sequence_its_own_calibration(monkeypatch, kw, host):
    build, uploads = gt.install(monkeypatch)
    pipe, trace, _ = build(sequence=True, image_wh_max=(1242, 375), **kw)
    run = _Run(pipe, trace)
    heads = tr._heads(pipe) if pipe.rpn_head is None else None
    push = pipe.push_frame_from_host if host else pipe.push_frame
    for seq, (cal, keyframes) in enumerate(((B, 7), (C, 4), (None, 3), (B, 3))):
        real = cal or A
        keys = [run.key(real) for _ in range(keyframes)]
        args = [(object(), n, object()) for _, n, _ in keys] if host else keys
        for j in range(keyframes):
            la = None
            if j % 3 != 1 and j + 1 < keyframes:    # (the priming push announces its successor too)
                la = tuple(args[j + 1]) + (tr.EGO if j % 2 else None, cal)
            run.host_next = real
            step = pipe.step_idx if j else None
            n = len(trace)
            ret = run.call('push %d.%d' % (seq, j), push, *args[j], heads=heads if j else None,
                           ego_motion=tr.EGO if j % 4 == 1 else None, lookahead=la, calib=cal,
                           recover=tr._recover(pipe, bool(pipe.temporal) and j % 2 == 1), step=step,
                           calibs=[real] if j else None)
            assert (ret is None) == (j == 0)
            if seq == 0 and j == 4:
                run.call('finish %d.%d' % (seq, j), pipe.finish)
        run.call('finish %d' % seq, pipe.finish)
        pipe.end_sequence()
    seen = run.check(uploads)
    pairs = 6 + 3 + 2 + 2
    assert seen['carried'] == pairs and seen['prep'] == pairs + 4 and seen['tail'] == 2 * pairs
    if pipe.tracker is not None:
        assert seen['tracker'] == seen['temporal'] == pairs
    # the carried keyframe of a sequence's first pair sits in ring slots the last sequence used: it is voxelised a second
    # time under ITS calibration (B, C, A, B in turn), whichever that was
    # (with the priming push's look-ahead that launch is enqueued by the priming call itself)
    carried = [t['args'][2] for t in trace if t['op'] == 'bev_slices' and t['args'][4] is None]
    assert len(carried) == pairs
    assert all(gt.bp_matches(carried[i], c) for i, c in zip((0, 6, 9, 11), (B, C, A, B)))
    assert not tr.races(pipe, trace)


def test_sequence_mode_refusals_log_nothing(monkeypatch):
    build, _ = gt.install(monkeypatch)
    pipe, trace, _ = build(sequence=True, tracker={})
    run = _Run(pipe, trace)
    heads = tr._heads(pipe)
    n = len(trace)
    with pytest.raises(ValueError):                  # the image is not of the calibration's size
        pipe.push_frame(*run.key(A), calib=B)
    with pytest.raises(ValueError):
        pipe.push_frame(*run.key(B), calib=[B, B])
    with pytest.raises(ValueError):                  # the look-ahead frame is of the same sequence
        pipe.push_frame(*run.key(B), calib=B, lookahead=run.key(C) + (None, C))
    with pytest.raises(ValueError):
        pipe.push_frame_from_host(object(), 1, object(),
                                  calib=gt.config.Calibration(B.p2, B.r0_rect, B.tr_velo_to_cam, (1243, 375)))
    assert len(trace) == n
    assert pipe.push_frame(*run.key(B), calib=B) is None
    pipe.push_frame(*run.key(B), heads=heads, calib=B)
    n = len(trace)
    with pytest.raises(ValueError):                  # inside a sequence the calibration stays
        pipe.push_frame(*run.key(C), heads=heads, calib=C)
    with pytest.raises(ValueError):
        pipe.push_frame(*run.key(A), heads=heads)
    with pytest.raises(ValueError):
        pipe.push_frame(*run.key(B), heads=heads, calib=B, lookahead=run.key(A))
    assert len(trace) == n
    pipe.finish()
    pipe.end_sequence()
    assert pipe.push_frame(*run.key(C), calib=C) is None


def test_the_default_path_is_the_constructors_calibration(monkeypatch):
    """calib=None, the constructor's calibration given explicitly, and an equal one made from lists: the same launches."""
    texts = []
    for cal in (None, A, gt.config.Calibration(A.p2.tolist(), A.r0_rect.tolist(), A.tr_velo_to_cam.tolist(), [1242, 375])):
        build, _ = gt.install(monkeypatch)
        pipe, trace, _ = build(head_params=tr.HP, temporal=dict(n_frames=3), tracker={})
        extra = dict(inputs=[])
        for k in range(4):
            ins = [list(a) for a in zip(*[tr._frame(pipe) for _ in range(2)])]
            extra['inputs'].append(ins)
            kw = {} if cal is None else dict(calib=cal)
            pipe.run(*ins, recover=tr._recover(pipe, k % 2 == 1), **kw)
        pipe.finish()
        texts.append(tr.canonical(pipe, trace, extra))
    assert texts[0] == texts[1] == texts[2]
