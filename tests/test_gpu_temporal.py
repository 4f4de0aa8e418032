"""The temporal module "M" of S+T+M on the device (dodt_amd/csrc/temporal.hip): its 3-D IoU and its interpolation
against the host module (dodt_amd.core.dt_evaluator_utils) and the reference's goldens, and the pipeline's opt-in
stage (FramePairPipeline(temporal=...), frames()) against the host module run on the pipeline's own records."""
import os

import numpy as np
import pytest

from dodt_amd import config, device, synth
from dodt_amd import temporal as dev
from dodt_amd.core import dt_evaluator_utils as host
from dodt_amd.datasets.kitti import kitti_tracking_utils as ktu
from dodt_amd.pipeline import MAX_DET, REC_COLS, FramePairPipeline

pytestmark = pytest.mark.gpu
C = config.PYRAMID_DODT
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
T = np.load(os.path.join(GOLDEN, 'temporal.npz'))
E = np.load(os.path.join(GOLDEN, 'egomotion.npz'))
CASES = sorted({int(k[1:k.index('_')]) for k in T.files if k.startswith('c')})


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _random_boxes(rng, n, spread):
    return np.stack([rng.uniform(-spread, spread, n), rng.normal(1.65, 0.2, n), rng.uniform(0, 2 * spread, n),
                     rng.normal(3.9, 0.4, n), rng.normal(1.6, 0.15, n), rng.normal(1.5, 0.1, n),
                     rng.uniform(-np.pi, np.pi, n)], 1)


def _same(got, want, what=''):
    assert len(got) == len(want), what
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12, err_msg='%s frame %d' % (what, f))


# ---- 1. IoU ----------------------------------------------------------------------------------------------------
def _check_iou(ctx, a, b):
    want = host.three_d_iou_matrix(a, b)
    got = dev.three_d_iou_matrix(a, b, ctx=ctx)
    assert got.shape == want.shape
    # (atol 1e-13: the overlap of two slivers cancels in the shoelace sum, and cos/sin of the device's math library may
    #  differ from numpy's in the last bit -- the bar tests/test_temporal.py holds the batched host form to)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    # the pairs whose bounding spheres do not touch are exactly 0; elsewhere a zero-width sliver (touching boxes) may
    # come out 0 on one side and 1e-17 on the other
    da, db = np.sqrt((a[:, 3:6] ** 2).sum(1)) / 2, np.sqrt((b[:, 3:6] ** 2).sum(1)) / 2
    apart = ~(da[:, None] + db[None, :] >= np.sqrt(((b[None, :, 0:3] - a[:, None, 0:3]) ** 2).sum(2)))
    assert apart.sum() > 0 and np.all(got[apart] == 0) and np.all(want[apart] == 0)
    assert np.all(np.abs(got[want == 0]) <= 1e-13)
    return want


def test_iou_matches_host_on_golden_boxes(ctx):
    std = T['iou_boxes'][:, [4, 5, 6, 1, 3, 2, 0]]           # [ry,l,h,w,tx,ty,tz] -> [x,y,z,l,w,h,ry]
    want = _check_iou(ctx, std, std)
    assert (want > 0).sum() > len(std)
    np.testing.assert_allclose(np.diag(want), 1.0, rtol=1e-12)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_iou_matches_host_on_seeded_sets(ctx, seed):
    rng = np.random.default_rng(seed)
    a, b = _random_boxes(rng, 200, 8.0), _random_boxes(rng, 200, 8.0)
    b[:10] = a[:10]                                           # identical boxes: IoU 1
    b[10:20] = a[10:20]
    b[10:20, 0] += a[10:20, 3]                                # shared edge along the length (ry 0 below)
    a[10:20, 6] = b[10:20, 6] = 0.0
    a[20:30, 6] = np.pi / 2                                   # ry +-pi/2
    b[20:30] = a[20:30]
    b[20:30, 6] = -np.pi / 2
    b[30:40, 3] = 0.0                                         # zero-length boxes
    a[40:50, 3] = 0.0
    b[50:70, 0] += 1000.0                                     # far apart
    # sphere-test borderline: centres exactly as far apart as the two half-diagonals add up
    for i in range(70, 90):
        b[i] = a[i]
        da = np.sqrt((a[i, 3:6] ** 2).sum()) / 2
        b[i, 0] = a[i, 0] + 2 * da
    b[90:110, 3:6] = a[90:110, 3:6]
    b[90:110, 0:3] = a[90:110, 0:3] + rng.normal(0, 0.5, (20, 3))
    want = _check_iou(ctx, a, b)
    assert (want > 0).sum() > 1000 and (want == 0).sum() > 1000
    np.testing.assert_allclose(np.diag(want)[:10], 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.diag(want)[20:30], 1.0, rtol=1e-12)


# ---- 2. reference goldens --------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', CASES)
def test_device_matches_reference_goldens(ctx, cid):
    n = int(T['c%d_nframes' % cid])
    want = [T['c%d_out%d' % (cid, i)] for i in range(n)]
    got = dev.interpolate_non_keyframe_predictions(T['c%d_pred' % cid], n, 0.1, ctx=ctx)
    assert len(got) == n
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12)


# ---- 3. recovery -----------------------------------------------------------------------------------------------
def test_recovery_matches_reference(ctx):
    boxes = E['boxes']
    rec = np.zeros((len(boxes), 17))
    rec[:, :9] = boxes
    rec[:, 16] = 1
    recover = dict(r0_rect=E['r0'], tr_velo_to_cam=E['tr'], ego=[(E['trans'], E['matrix'], float(E['delta']))])
    got = dev.interpolate_non_keyframe_predictions(rec, 2, -1.0, recover=recover, ctx=ctx)
    assert got[0].shape == (0, 13) and got[1].shape == (len(boxes), 13)
    np.testing.assert_allclose(got[1][:, :9], E['recovered'], rtol=0, atol=1e-9)


# ---- 4. seeded scenes against the host module ------------------------------------------------------------------
def _scene(rng, n0, births, deaths, spread=20.0, jitter=0.3):
    """Keyframe 0: n0 detections; keyframe 1: the survivors jittered, plus births.  Scores straddle 0.1 (some are
    exactly float32(0.1)); the offset columns are a mix of the shifted box and small numbers (near / far tracks)."""
    b0 = _random_boxes(rng, n0, spread)
    keep = np.sort(rng.permutation(n0)[:max(0, n0 - deaths)])
    b1 = b0[keep].copy()
    b1[:, [0, 2]] += rng.normal(0, jitter, (len(b1), 2))
    b1[:, 6] += rng.normal(0, 0.05, len(b1))
    b1 = np.concatenate([b1, _random_boxes(rng, births, spread)])
    b1 = b1[rng.permutation(len(b1))][:MAX_DET]
    rows = []
    for f, b in enumerate((b0, b1)):
        r = np.zeros((len(b), 17))
        r[:, :7] = b
        r[:, 7] = rng.uniform(0.0, 0.5, len(b))
        r[rng.uniform(size=len(b)) < 0.1, 7] = np.float32(0.1)
        r[:, 8] = 0
        if f == 0:
            r[:, 9:16] = b + rng.normal(0, 0.3, b.shape)
            small = rng.uniform(size=len(b)) < 0.5
            r[small, 13:15] = rng.normal(0, 0.4, (small.sum(), 2))
        r[:, 16] = f
        rows.append(r)
    p = np.concatenate(rows)
    return p[rng.permutation(len(p))].astype(np.float32).astype(np.float64)     # marks mixed, as records


def _claims_scene():
    k0 = np.zeros((2, 17))
    k0[:, :7] = [[0, 1.65, 10, 4, 1.6, 1.5, 0], [1.0, 1.65, 10.2, 4, 1.6, 1.5, 0]]
    k1 = np.zeros((2, 17))
    k1[:, :7] = [[0.5, 1.65, 10.1, 4, 1.6, 1.5, 0], [3.0, 1.65, 11.5, 4, 1.6, 1.5, 0]]
    k1[:, 16] = 1
    p = np.concatenate([k0, k1])
    p[:, 7] = [0.9, 0.8, 0.7, 0.6]
    return p


def _scenes():
    rng = np.random.default_rng(2024)
    out = [_claims_scene()]
    for i in range(14):
        n0 = int(rng.integers(0, MAX_DET + 1))
        out.append(_scene(rng, n0, births=int(rng.integers(0, 20)), deaths=int(rng.integers(0, max(1, n0 // 4 + 1))),
                          spread=float(rng.choice([5.0, 20.0, 40.0])), jitter=float(rng.choice([0.1, 0.6]))))
    out.append(_scene(rng, 100, 0, 0, spread=3.0, jitter=1.0))        # crowded: many claims on one detection
    out.append(np.zeros((0, 17)))                                      # empty keyframes
    only1 = _scene(rng, 30, 5, 0)
    out.append(only1[only1[:, 16] == 1])                               # keyframe 1 only
    only0 = _scene(rng, 30, 5, 0)
    out.append(only0[only0[:, 16] == 0])                               # keyframe 0 only
    # 100 + 100 without any overlap: 200 rows per frame
    far = _scene(rng, 100, 0, 0, spread=20.0)
    far[:, 7] = 0.5
    far[:, 13:15] = 0.0                                                # every track "near": present in every frame
    far[far[:, 16] == 1, 0] += 1000.0
    out.append(far)
    return out


SCENES = _scenes()


@pytest.mark.parametrize('n_frames', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('on_conflict', ['raise', 'next_best'])
def test_seeded_scenes_match_host(ctx, n_frames, on_conflict):
    raised = 0
    for i, p in enumerate(SCENES):
        try:
            want = host.interpolate_non_keyframe_predictions(p, n_frames, 0.1, on_conflict=on_conflict)
        except ValueError:
            want = None
        if want is None:
            raised += 1
            with pytest.raises(ValueError):
                dev.interpolate_non_keyframe_predictions(p, n_frames, 0.1, on_conflict=on_conflict, ctx=ctx)
            continue
        got = dev.interpolate_non_keyframe_predictions(p, n_frames, 0.1, on_conflict=on_conflict, ctx=ctx)
        _same(got, want, 'scene %d' % i)
        if i == len(SCENES) - 1 and n_frames >= 3:
            assert all(len(g) == 200 for g in got)
    if on_conflict == 'raise' and n_frames >= 3:
        assert raised >= 1          # (the two-claims scene at least)
    else:
        assert raised == 0


# ---- 5. the pipeline, free-running -----------------------------------------------------------------------------
def _inputs(ctx, pairs, n_batches=3):
    ins = []
    for b in range(n_batches):
        frames = [(20 + b + 10 * q, f) for q in range(pairs) for f in (0, 2)]
        pts = [synth.lidar_frame(s, f) for s, f in frames]
        ins.append(([ctx.array(p) for p in pts], [len(p) for p in pts],
                    [ctx.array(synth.image_frame(s, f)) for s, f in frames], frames))
    return ins


def _host_frames(rec, cnt, n_frames, threshold, on_conflict):
    """The host module on one step's downloaded records, per pair."""
    out = []
    for pair in range(rec.shape[0]):
        p = np.concatenate([rec[pair, f, :cnt[pair, f]] for f in range(2)])
        out.append(host.interpolate_non_keyframe_predictions(p, n_frames, threshold, on_conflict=on_conflict))
    return out


@pytest.mark.parametrize('mode', ['f32_injected', 'bf16_computed_lookahead'])
def test_free_running_pipeline_frames_match_host(ctx, mode):
    pairs, R, steps, n_frames = 2, 4, 30, 3
    tm = dict(n_frames=n_frames, threshold=0.1, on_conflict='next_best')
    if mode == 'f32_injected':
        kw = dict(rpn_nms_size=1024)
    else:
        kw = dict(rpn_nms_size=1024, head_params=synth.head_params(), conv_dtype='bf16', head_dtype='bf16')
    pipe = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), pairs_per_step=pairs, temporal=tm, **kw)
    plain = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), pairs_per_step=pairs, reuse_streams_of=pipe, **kw)
    ins = _inputs(ctx, pairs)
    computed = 'head_params' in kw
    heads = [None if computed else
             [{k: ctx.array(v) for k, v in synth.head_outputs(s, f, pipe.n_all, pipe.P).items()} for s, f in fr]
             for _, _, _, fr in ins]
    rec_ring = ctx.zeros((R, pairs, 2, MAX_DET, REC_COLS), np.float32)
    cnt_ring = ctx.zeros((R, pairs, 2), np.int32)
    pipe.use_record_ring(rec_ring, cnt_ring)
    for k in range(steps):
        b = k % len(ins)
        la = ins[(k + 1) % len(ins)][:3] if computed and k + 1 < steps else None
        pipe.run(*ins[b][:3], heads=heads[b], lookahead=la)
    pipe.finish()
    ctx.sync()
    recs, cnts = rec_ring.download(), cnt_ring.download()
    got = {}
    for k in range(steps - R, steps):
        s = k % R
        got[k] = dev.unpack_frames(pipe.frames2[s].download(), pipe.fcnt2[s].download(), pipe.fst2[s].download(),
                                   'next_best')
        want = _host_frames(recs[s], cnts[s], n_frames, 0.1, 'next_best')
        assert sum(len(f) for w in want for f in w) > 0
        for pair in range(pairs):
            _same(got[k][pair], want[pair], 'step %d pair %d' % (k, pair))
    # step by step: the same frames; a pipeline without the temporal module: the same records, bit for bit
    for b in range(len(ins)):
        pipe.run(*ins[b][:3], heads=heads[b])
        pipe.finish()
        plain.run(*ins[b][:3], heads=heads[b])
        plain.finish()
        ctx.sync()
        one = pipe.frames()
        rec_plain, cnt_plain = plain.d_records.download(), plain.d_rec_counts.download()
        for k in range(steps - R, steps):
            if k % len(ins) != b:
                continue
            assert np.array_equal(recs[k % R], rec_plain), k
            assert np.array_equal(cnts[k % R], cnt_plain), k
            for pair in range(pairs):
                _same(got[k][pair], one[pair], 'step-by-step step %d pair %d' % (k, pair))
    pipe.close()
    plain.close()


# ---- 6. options ------------------------------------------------------------------------------------------------
def test_pipeline_with_recover_matches_host(ctx):
    n_frames = 3
    pipe = FramePairPipeline(ctx, C, **synth.pipeline_weights(C), rpn_nms_size=1024,
                             temporal=dict(n_frames=n_frames, threshold=0.1, on_conflict='next_best'),
                             r0_rect=E['r0'], tr_velo_to_cam=E['tr'])
    frames = [(31, 0), (31, 2)]
    pts = [synth.lidar_frame(s, f) for s, f in frames]
    d_heads = [{k: ctx.array(v) for k, v in synth.head_outputs(s, f, pipe.n_all, pipe.P).items()} for s, f in frames]
    rot = np.array([[np.cos(0.02), -np.sin(0.02), 0], [np.sin(0.02), np.cos(0.02), 0], [0, 0, 1.0]])
    ego = [(E['trans'] * 0.5, rot, 0.01), (E['trans'], E['matrix'], float(E['delta']))]
    pipe.run([ctx.array(p) for p in pts], [len(p) for p in pts], [ctx.array(synth.image_frame(s, f)) for s, f in frames],
             d_heads, recover=[ego])
    pipe.finish()
    ctx.sync()
    got = pipe.frames()[0]
    rec, cnt = pipe.d_records.download(), pipe.d_rec_counts.download()
    p = np.concatenate([rec[0, f, :cnt[0, f]] for f in range(2)])

    def recover(i, rows):
        trans, matrix, delta = ego[i - 1]
        return ktu.recovery_coordinate(rows.copy(), E['r0'], E['tr'], trans, matrix, delta)
    want = host.interpolate_non_keyframe_predictions(p, n_frames, 0.1, recover, on_conflict='next_best')
    plain = host.interpolate_non_keyframe_predictions(p, n_frames, 0.1, on_conflict='next_best')
    assert len(got) == n_frames and len(want[1]) > 0
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-9)
    assert np.abs(got[2][:, :3] - plain[2][:, :3]).max() > 0.1          # it did move them
    # the next step without recover is not recovered
    pipe.run([ctx.array(p) for p in pts], [len(p) for p in pts], [ctx.array(synth.image_frame(s, f)) for s, f in frames],
             d_heads)
    pipe.finish()
    ctx.sync()
    _same(pipe.frames()[0], plain)
    pipe.close()


def test_temporal_needs_frame_pairs(ctx):
    cfg = config.CARS_EXAMPLE
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, cfg, **synth.pipeline_weights(cfg), temporal=dict(n_frames=3))
    with pytest.raises(ValueError):
        FramePairPipeline(ctx, C, **synth.pipeline_weights(C), temporal=dict(n_frames=3, on_conflict='ignore'))


def test_raise_mode_conflict_surfaces_from_frames(ctx):
    """The status word of a 'raise'-mode conflict reaches the caller as ValueError, like the host module's raise."""
    p = _claims_scene()
    with pytest.raises(ValueError):
        dev.interpolate_non_keyframe_predictions(p, 3, 0.1, ctx=ctx)
    out = dev.interpolate_non_keyframe_predictions(p, 3, 0.1, on_conflict='next_best', ctx=ctx)
    assert [len(o) for o in out] == [2, 2, 2]
