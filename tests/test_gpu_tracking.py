"""The IoU tracker on the device (dodt_amd/csrc/tracking.hip) against the host module
(dodt_amd.core.dt_evaluator_utils encode_tracking_dets + track_through_ious) and the reference's goldens, and the
pipeline's opt-in stage (FramePairPipeline(tracker=...), end_sequence()) against the host module run on the
pipeline's own records."""
import os

import numpy as np
import pytest

from dodt_amd import config, device, synth
from dodt_amd import tracking as dev
from dodt_amd.core import dt_evaluator_utils as host
from dodt_amd.pipeline import MAX_DET, REC_COLS, FramePairPipeline

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
P2, WH = config.KITTI_P2, config.KITTI_IMAGE_WH
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'tracking.npz'))
REFERENCE = (0.1, 0.5, 0.005, 3)         # score, high, iou, t_min (avod_stack_tracking.config:137-140)
LOOSE = (0.1, 0.6, 0.1, 2)


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _rows(tracks):
    rows = [[t['start_frame'], float(t['max_score']), len(t['trajectory'])]
            + [d['serial'] for d in t['trajectory']] + [-1] * (16 - len(t['trajectory']))
            for t in tracks]
    return np.asarray(rows, np.float64).reshape(-1, 19)


# ---- (a) track_through_ious on the reference's goldens ------------------------------------------------------------
@pytest.mark.parametrize('case', [0, 1, 2])
def test_track_through_ious_matches_reference(ctx, case):
    table = G['ttI%d_table' % case]
    n_pairs = int(table[:, 1].max()) + 1
    dets_for_track = [[] for _ in range(n_pairs)]
    dets_for_ious = [{}] + [[] for _ in range(n_pairs)]
    for r in table:
        d = {'serial': int(r[0]), 'frame_id': str(int(r[1] + r[2])),
             'boxes3d': r[4:11].astype(np.float32), 'scores': np.float32(r[3])}
        if r[2] == 0:
            d['offsets'] = r[11:18].astype(np.float32)
            dets_for_track[int(r[1])].append(d)
        else:
            dets_for_ious[int(r[1]) + 1].append(d)
    before = [len(f) for f in dets_for_track]
    tracks = dev.track_through_ious(dets_for_track, dets_for_ious, 0.6, 0.1, 2, ctx=ctx)
    got, want = _rows(tracks), G['ttI%d_tracks' % case]
    assert got.shape == want.shape and np.array_equal(got[:, [0, 2]], want[:, [0, 2]])
    assert np.array_equal(got[:, 3:], want[:, 3:])
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=0, atol=0)
    assert all(type(t['max_score']) is np.float32 for t in tracks)
    assert [len(f) for f in dets_for_track] == before


# ---- synthetic sequences ------------------------------------------------------------------------------------------
def _sequence(rng, n_pairs, n_obj=14, special=False, empty=()):
    """Records (n,17) per pair of cars driving through the camera's view, born and dying along the sequence:
    keyframe-0 rows (mark 0) with the box shifted into keyframe 1 in cols 9:16, keyframe-1 rows (mark 1)."""
    x0, z0 = rng.uniform(-14, 14, n_obj), rng.uniform(8, 45, n_obj)
    vx, vz = rng.uniform(-0.4, 0.4, n_obj), rng.uniform(-0.6, 0.9, n_obj)
    dims = np.stack([rng.uniform(3.4, 4.6, n_obj), rng.uniform(1.5, 1.8, n_obj), rng.uniform(1.4, 1.7, n_obj)], 1)
    ry = rng.uniform(-np.pi, np.pi, n_obj)
    birth = rng.integers(0, n_pairs, n_obj)
    birth[: n_obj // 3] = 0
    death = np.minimum(birth + rng.integers(2, n_pairs, n_obj), n_pairs + 1)

    def box(o, t, sd=0.04):
        return np.concatenate([[x0[o] + vx[o] * t + rng.normal(0, sd), 1.6 + rng.normal(0, 0.02),
                                z0[o] + vz[o] * t + rng.normal(0, sd)], dims[o], [ry[o] + rng.normal(0, 0.01)]])
    pairs = []
    for j in range(n_pairs):
        r0, r1 = [], []
        if j not in empty:
            for o in range(n_obj):
                if birth[o] <= j < death[o] and rng.uniform() > 0.1:
                    r0.append(np.concatenate([box(o, j), [rng.uniform(0.02, 1.0), 0], box(o, j + 1), [0]]))
                if birth[o] <= j + 1 < death[o] and rng.uniform() > 0.1:
                    r1.append(np.concatenate([box(o, j + 1), [rng.uniform(0.02, 1.0), 0], np.zeros(7), [1]]))
        r0 = np.asarray(r0).reshape(-1, 17)
        r1 = np.asarray(r1).reshape(-1, 17)
        if special and len(r0) >= 4 and len(r1) >= 2:
            r0[0, 7] = 0.05                                  # below the threshold
            r0[1, 0:3] = [0.0, 1.6, -6.0]                    # behind the camera: outside the image
            r0[2, 3:6] = [40.0, 30.0, 20.0]                  # wider than 0.8 x the image
            r0[2, 2] = 6.0
            r0[3, 9] = 300.0                                 # the shifted box leaves the image: the zip shifts
            r1[0, 0] = -80.0                                 # keyframe 1: outside the image
            r1[1, 7] = 0.1                                   # exactly the threshold (kept)
        rec = np.concatenate([r0, r1]).astype(np.float32)
        pairs.append((2 * j, 2 * j + 2, rec[rng.permutation(len(rec))]))
    return pairs


def _same_item(g, w, what):
    assert g['frame_id'] == w['frame_id'] and g['info'] == w['info'], what
    for k in ('boxes2d', 'boxes3d', 'offsets'):
        assert (k in g) == (k in w), (what, k)
        if k in w:
            assert g[k].dtype == np.float32 and np.array_equal(g[k], w[k]), (what, k, g[k], w[k])
    assert type(g['scores']) is np.float32 and g['scores'] == w['scores'], what


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, list) == isinstance(w, list) and len(g) == len(w), (what, j, len(g), len(w))
        for i, (a, b) in enumerate(zip(g, w)):
            _same_item(a, b, '%s list %d item %d' % (what, j, i))


def _same_tracks(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        assert g['start_frame'] == w['start_frame'], (what, n)
        assert type(g['max_score']) is np.float32 and g['max_score'] == w['max_score'], (what, n)
        assert len(g['trajectory']) == len(w['trajectory']), (what, n)
        for i, (a, b) in enumerate(zip(g['trajectory'], w['trajectory'])):
            _same_item(a, b, '%s track %d det %d' % (what, n, i))


def _host_tracks(pairs, params):
    score, high, iou, t_min = params
    dft, dfi = host.encode_tracking_dets(pairs, P2, WH, ['Car'], score)
    return host.track_through_ious(dft, dfi, high, iou, t_min)


# ---- (b) encode_tracking_dets -------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_encode_matches_host(ctx, seed):
    rng = np.random.default_rng(seed)
    pairs = _sequence(rng, 24, special=True, empty=(3, 4, 11))
    # a pair whose keyframe-0 rows all fall below the threshold and whose keyframe 1 is empty: skipped as well
    low = pairs[7][2][pairs[7][2][:, 16] == 0].copy()
    low[:, 7] = 0.01
    pairs[7] = (pairs[7][0], pairs[7][1], low)
    for threshold in (0.1, 0.3):
        want = host.encode_tracking_dets(pairs, P2, WH, ['Car'], threshold)
        got = dev.encode_tracking_dets(pairs, P2, WH, ['Car'], threshold, ctx=ctx)
        assert len(want[0]) <= 24 - 4                    # the skip rule was exercised
        _same_lists(got[0], want[0], 'dets_for_track')
        _same_lists(got[1][1:], want[1][1:], 'dets_for_ious')
        assert got[1][0] == {}


# ---- (c) encode + track over synthetic sequences -------------------------------------------------------------------
@pytest.mark.parametrize('params', [REFERENCE, LOOSE])
@pytest.mark.parametrize('seed', [5, 6])
def test_sequences_match_host(ctx, seed, params):
    rng = np.random.default_rng(seed)
    pairs = _sequence(rng, 48, n_obj=20, empty=(9, 30))
    want = _host_tracks(pairs, params)
    assert len(want) >= 5 and max(len(t['trajectory']) for t in want) >= 6
    recs, counts, max_det = dev._pack_records(pairs)
    score, high, iou, t_min = params
    for batch in (48, 1, 5):           # one call (three chunks), pair by pair, and in batches that straddle them
        tr = dev.Tracker(ctx, 4096, high, iou, t_min, score)
        for p0 in range(0, len(pairs), batch):
            n = min(batch, len(pairs) - p0)
            tr.track_records(ctx.array(recs[p0:p0 + n]), ctx.array(counts[p0:p0 + n]), n, max_det, P2, WH)
        tr.flush()
        got = dev.tracks_from_log(tr.read(), lambda pair, kf: 2 * pair + 2 * kf, ['Car'])
        _same_tracks(got, want, 'batch %d' % batch)
    # the host-array form on the host's own encoding
    dft, dfi = host.encode_tracking_dets(pairs, P2, WH, ['Car'], score)
    for d in [x for f in dft for x in f] + [x for f in dfi[1:] for x in f]:
        d['serial'] = id(d)
    got = dev.track_through_ious(dft, dfi, high, iou, t_min, ctx=ctx)
    ref = host.track_through_ious(dft, dfi, high, iou, t_min)
    assert [(t['start_frame'], t['max_score'], [d['serial'] for d in t['trajectory']]) for t in got] == \
        [(t['start_frame'], t['max_score'], [d['serial'] for d in t['trajectory']]) for t in ref]
    _same_tracks(got, ref, 'host-array form')


def test_sliver_and_tied_decisions_match_host(ctx):
    """Decisions that sit on the edge: touching boxes (IoU 0 or a sliver) in the merge, duplicated columns (argmax
    ties) and IoUs around the threshold."""
    rng = np.random.default_rng(11)
    pairs = _sequence(rng, 40, n_obj=16)
    for j in range(1, 40, 3):
        rec = pairs[j][2]
        k1 = np.flatnonzero(rec[:, 16] == 1)
        k0 = np.flatnonzero(rec[:, 16] == 0)
        if len(k1) >= 3 and len(k0) >= 1:
            rec[k1[1], :7] = rec[k1[0], :7]                     # a duplicate: tied columns
            rec[k1[2], :7] = rec[k1[0], :7]
            rec[k1[2], 0] = rec[k1[0], 0] + rec[k1[0], 5]      # shifted by the IoU's (permuted) length: a sliver
            rec[k0[0], 9:16] = rec[k1[0], :7]
    for params in (REFERENCE, LOOSE, (0.1, 0.5, 0.0, 2)):
        want = _host_tracks(pairs, params)
        tr = dev.Tracker(ctx, 4096, *params[1:], score_threshold=params[0])
        recs, counts, max_det = dev._pack_records(pairs)
        tr.track_records(ctx.array(recs), ctx.array(counts), len(pairs), max_det, P2, WH)
        tr.flush()
        _same_tracks(dev.tracks_from_log(tr.read(), lambda pair, kf: 2 * pair + 2 * kf, ['Car']), want, str(params))


# ---- (f) the log's capacity ---------------------------------------------------------------------------------------
def test_log_overflow_raises(ctx):
    rng = np.random.default_rng(4)
    pairs = _sequence(rng, 20)
    recs, counts, max_det = dev._pack_records(pairs)
    tr = dev.Tracker(ctx, 8, 0.0, 0.005, 1)
    guard = ctx.zeros((4096,), np.uint8)                       # (allocated after the state)
    tr.track_records(ctx.array(recs), ctx.array(counts), len(pairs), max_det, P2, WH)
    tr.flush()
    with pytest.raises(RuntimeError, match='capacity'):
        tr.read()
    assert tr.header()['n_log'] > 8
    assert not guard.download().any()
    tr.reset()
    ctx.sync()
    assert tr.read() == []


# ---- (d), (e), (g): the pipeline ------------------------------------------------------------------------------------
def _inputs(ctx, pairs, n_batches=3):
    ins = []
    for b in range(n_batches):
        frames = [(20 + b + 10 * q, f) for q in range(pairs) for f in (0, 2)]
        pts = [synth.lidar_frame(s, f) for s, f in frames]
        ins.append(([ctx.array(p) for p in pts], [len(p) for p in pts],
                    [ctx.array(synth.image_frame(s, f)) for s, f in frames], frames))
    return ins


def _pipeline_pairs(recs, cnts, frame_ids):
    """A record ring's steps (steps, pairs, 2, max_det, 17) -> the host's [(frame_0, frame_1, records)]."""
    out = []
    for k in range(recs.shape[0]):
        for q in range(recs.shape[1]):
            rows = [recs[k, q, f, :cnts[k, q, f]] for f in range(2)]
            assert all(np.all(r[:, 16] == f) for f, r in enumerate(rows))
            j = len(out)
            out.append((frame_ids(j, 0), frame_ids(j, 1), np.concatenate(rows)))
    return out


TRACKER = dict(score_threshold=0.1, high_threshold=0.3, iou_threshold=0.005, t_min=1, classes=('Car',),
               max_sequence_dets=1 << 15)


@pytest.mark.parametrize('temporal', [False, True])
@pytest.mark.parametrize('pairs', [1, 2])
@pytest.mark.parametrize('mode', ['f32_injected', 'bf16_computed_lookahead'])
def test_free_running_pipeline_tracks_match_host(ctx, mode, pairs, temporal):
    steps = 30
    tm = dict(n_frames=3, threshold=0.1, on_conflict='next_best') if temporal else None
    if mode == 'f32_injected':
        kw = dict(rpn_nms_size=1024)
    else:
        kw = dict(rpn_nms_size=1024, head_params=synth.head_params(), conv_dtype='bf16', head_dtype='bf16')
    pipe = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), pairs_per_step=pairs, temporal=tm, tracker=TRACKER,
                             **kw)
    ins = _inputs(ctx, pairs)
    computed = 'head_params' in kw
    heads = [None if computed else
             [{k: ctx.array(v) for k, v in synth.head_outputs(s, f, pipe.n_all, pipe.P).items()} for s, f in fr]
             for _, _, _, fr in ins]
    rec_ring = ctx.zeros((steps, pairs, 2, MAX_DET, REC_COLS), np.float32)
    cnt_ring = ctx.zeros((steps, pairs, 2), np.int32)
    pipe.use_record_ring(rec_ring, cnt_ring)
    for seq in range(2):                    # (e) two sequences, separated by end_sequence()
        for k in range(steps):
            b = (k + seq) % len(ins)
            la = ins[(k + seq + 1) % len(ins)][:3] if computed and k + 1 < steps else None
            pipe.run(*ins[b][:3], heads=heads[b], lookahead=la)
        pipe.finish()
        tau = 2 if temporal else 1
        got = pipe.end_sequence()
        ctx.sync()
        host_pairs = _pipeline_pairs(rec_ring.download(), cnt_ring.download(), lambda j, f: j * tau + f * tau)
        assert sum(len(p[2]) for p in host_pairs) > 0
        want = _host_tracks(host_pairs, (0.1, 0.3, 0.005, 1))
        assert len(want) > 0
        _same_tracks(got, want, '%s pairs %d temporal %s sequence %d' % (mode, pairs, temporal, seq))
        rows = pipe.kitti_tracking_rows()
        assert np.array_equal(rows, host.convert_trajectory_to_kitti_format(want))
        assert pipe.tracks_so_far() == []   # the next sequence starts empty
    pipe.close()


def test_pipeline_without_tracker_is_unchanged(ctx):
    """(g) tracker=None: the same records and frames as a pipeline with the tracker, and nothing allocated for it."""
    pairs, tm = 2, dict(n_frames=3, threshold=0.1, on_conflict='next_best')
    pipe = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024, pairs_per_step=pairs,
                             temporal=tm, tracker=TRACKER)
    plain = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024, pairs_per_step=pairs,
                              temporal=tm, reuse_streams_of=pipe)
    assert plain.tracker is None and not hasattr(plain, 'track_state')
    with pytest.raises(ValueError):
        plain.tracks_so_far()
    ins = _inputs(ctx, pairs)
    for b in range(len(ins)):
        heads = [{k: ctx.array(v) for k, v in synth.head_outputs(s, f, pipe.n_all, pipe.P).items()}
                 for s, f in ins[b][3]]
        for p in (pipe, plain):
            p.run(*ins[b][:3], heads=heads)
            p.finish()
        ctx.sync()
        assert np.array_equal(pipe.d_records.download(), plain.d_records.download())
        assert np.array_equal(pipe.d_rec_counts.download(), plain.d_rec_counts.download())
        for a, c in zip(pipe.frames(), plain.frames()):
            for fa, fc in zip(a, c):
                assert np.array_equal(fa, fc)
    assert len(pipe.end_sequence()) >= 0
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, C, **synth.pipeline_weights(C), tracker=dict(t_min=2, stride=3))
    pipe.close()
    plain.close()
