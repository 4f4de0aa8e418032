"""Per-sample geometry on the device: one FramePairPipeline given `calib=` per step against (1) the reference's own
output for the bundled real clouds, whose samples come with three calibrations and image sizes
(tests/golden/all_frames.json), and (2) pipelines CONSTRUCTED with each calibration and fed the same step -- records,
counts and the keep lists byte-equal --, in pair mode (step by step, free-running, with look-ahead, without the BEV skip
tables, two pairs of different calibrations in one step) and in sequence mode (two sequences, temporal module with
recovery, tracker, frames from host memory smaller than the staging buffer).  Needs an MI355X."""
import numpy as np
import pytest

import _real_clouds as rc
from dodt_amd import config, device, synth
from dodt_amd.pipeline import FramePairPipeline, MAX_DET, REC_COLS
from oracle import points as opoints

pytestmark = pytest.mark.gpu
CFG = config.PYRAMID_DODT
RECORDS = rc.records_by_tag()
SEQ, N_POINTS = 47, 30000
TEMPORAL = dict(n_frames=3, threshold=0.1, on_conflict='next_best')
TRACKER = dict(score_threshold=0.1, high_threshold=0.3, iou_threshold=0.005, t_min=1, classes=('Car',),
               max_sequence_dets=1 << 15)


def _calibration(tag):
    r0, tr, p2, wh = rc.calib_of(RECORDS[tag])
    return config.Calibration(p2, r0, tr, wh)


A, B, C = (_calibration(t) for t in ('trk0001_000000', 'obj000006', 'obj000000'))   # 1242x375, 1238x374, 1224x370
CALS = dict(A=A, B=B, C=C)


def _as_ctor(cal):
    return dict(p2=cal.p2, r0_rect=cal.r0_rect, tr_velo_to_cam=cal.tr_velo_to_cam, image_wh=cal.image_wh)


def _image(frame, cal):
    """The synthetic image of `frame`, cropped to the sample's size."""
    w, h = cal.image_wh
    return np.ascontiguousarray(synth.image_frame(SEQ, frame)[:h, :w])


def _ego(deg, trans):
    a = np.deg2rad(deg)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return np.asarray(trans, np.float64), rot


def _recover(ego):
    """`recover` of one pair for n_frames = 3 from its registration: frame 1 half of it, frame 2 all of it."""
    trans, rot = ego if ego is not None else _ego(0.0, (0.0, 0.0, 0.0))
    ang = np.arctan2(rot[1, 0], rot[0, 0])
    half = _ego(np.rad2deg(ang) / 2, trans / 2)
    return [(half[0], half[1], ang / 2), (trans, rot, ang)]


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


def _snap(pipe):
    frames = []
    for f, b in enumerate(pipe.fr):
        n = pipe.last_anchor_counts[f]
        n_top, n_det = int(b['top_count'].download()[0]), int(b['det_count'].download()[0])
        frames.append(dict(A=n, keep=b['keep'].download()[:n], top_idx=b['top_idx'].download()[:n_top],
                           det_idx=b['det_idx'].download()[:n_det]))
    return dict(records=pipe.d_records.download().copy(), counts=pipe.d_rec_counts.download().copy(), frames=frames)


def _same_step(got, want, what, frames=None):
    assert np.array_equal(got['counts'], want['counts']), what
    assert got['records'].tobytes() == want['records'].tobytes(), what
    for f in range(len(want['frames'])) if frames is None else frames:
        for name in ('A', 'keep', 'top_idx', 'det_idx'):
            assert np.array_equal(got['frames'][f][name], want['frames'][f][name]), (what, f, name)


def _equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- 1. the reference's own output, every sample with its calibration -------------------------------------------------
REAL_STEPS = [   # (frame tags or (tag, pair tag), calib argument, its value)
    (('obj000003', 'obj000009'), None, A),
    (('obj000000', 'obj000000'), C, C),
    (('obj000006', 'obj000076'), B, B),
    (('trk0001_000000', 'pair_trk0001_000000_000002'), A, A),
]


def _device_outputs(pipe, f, g):
    """What check_digests takes, from frame f of the finished step.  (n_fov, the number of points inside the frustum, is
    no output of the device: counted on the host from the same rows.)"""
    b = pipe.fr[f]
    n = pipe.last_anchor_counts[f]
    words = b['occ'].download()
    nz, nx = pipe.nz, pipe.nx
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(nz, -1), axis=1, bitorder='little')
    assert not bits[:, nx:].any()
    keep = np.zeros(pipe.n_all, bool)
    keep[b['keep'].download()[:n]] = True
    assert keep.sum() == n
    out = dict(stack=pipe.d_bev_in[f].download(), occ=bits[:, :nx].T.astype(bool), keep=keep,
               bev_norm=b['bev_norm'].download()[:n][:, [1, 0, 3, 2]], img_norm=b['img_norm'].download()[:n][:, [1, 0, 3, 2]])
    imwh = (int(g['imwh'][0]), int(g['imwh'][1]))
    raw = opoints.lidar_in_camera_view(g['xyzi'], g['r0'], g['tr'], g['p2'], imwh)
    out['n_fov'] = raw.shape[1]
    if 'trans' in g:
        warped = opoints.point_cloud_transform(g['xyzi'], g['trans'], g['matrix'])
        out['n_fov'] = opoints.lidar_in_camera_view(warped, g['r0'], g['tr'], g['p2'], imwh).shape[1]
        out['n_fov_unwarped'] = raw.shape[1]
    return out


def test_real_clouds_per_step_calibration(ctx):
    pipe = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), n_points_max=50000, rpn_nms_size=1024)
    assert np.array_equal(pipe.anchors_all, rc.anchor_grid())
    heads = [{k: ctx.array(v) for k, v in synth.head_outputs(SEQ, f, pipe.n_all, pipe.P).items()} for f in range(2)]
    for k, (tags, arg, cal) in enumerate(REAL_STEPS):
        clouds = [rc.load_shipped(t) for t in tags]
        for g in clouds:        # the sample's calibration is the one its records were made with
            assert np.array_equal(g['p2'], cal.p2) and np.array_equal(g['r0'], cal.r0_rect)
            assert np.array_equal(g['tr'], cal.tr_velo_to_cam) and tuple(int(v) for v in g['imwh']) == cal.image_wh
        pts = [np.ascontiguousarray(g['xyzi'], dtype=np.float32) for g in clouds]
        ego = [(clouds[1]['trans'], clouds[1]['matrix'])] if 'trans' in clouds[1] else None
        pipe.run([ctx.array(p) for p in pts], [len(p) for p in pts], [ctx.array(_image(2 * k + f, cal)) for f in range(2)],
                 heads=heads, ego_motion=ego, calib=arg)
        pipe.finish()
        ctx.sync()
        for f, tag in enumerate(tags):
            rc.check_digests(_device_outputs(pipe, f, clouds[f]), RECORDS[tag])
    assert pipe.support.rebuilds == 3          # one per calibration, the constructor's included
    pipe.close()


# ---- 2. records against pipelines constructed with each calibration ---------------------------------------------------
STEPS = ['A', 'B', 'C', 'B', 'A', 'C']           # the calibration of step k
EGO = [None, _ego(3.0, (1.1, 0.15, 0.0)), None, _ego(-2.0, (0.9, -0.2, 0.02)), None, _ego(1.5, (0.8, 0.1, 0.0))]
KW = dict(rpn_nms_size=1024, head_params=None, t_branch_rows='proposals', temporal=TEMPORAL)


@pytest.fixture(scope='module')
def pair_case(ctx):
    """The inputs of the steps (pair k: frames 2k, 2k + 2 of one synthetic sequence, images cropped to the step's size),
    the switching pipeline, and what a pipeline constructed with each step's calibration makes of that step."""
    kw = dict(KW, head_params=synth.head_params())
    sw = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), n_points_max=N_POINTS, **kw)
    fresh = {n: FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), n_points_max=N_POINTS, reuse_streams_of=sw,
                                  **_as_ctor(c), **kw) for n, c in CALS.items()}
    assert all(np.array_equal(fresh[n].p2, CALS[n].p2) and fresh[n].image_wh == CALS[n].image_wh for n in CALS)
    ins, want = [], []
    for k, name in enumerate(STEPS):
        frames = (2 * k, 2 * k + 2)
        pts = [synth.lidar_frame(SEQ, f, N_POINTS) for f in frames]
        args = ([ctx.array(p) for p in pts], [len(p) for p in pts], [ctx.array(_image(f, CALS[name])) for f in frames])
        ins.append(dict(args=args, ego=[EGO[k]], recover=[_recover(EGO[k])], calib=CALS[name]))
        p = fresh[name]
        p.run(*args, ego_motion=[EGO[k]], recover=[_recover(EGO[k])])
        p.finish()
        ctx.sync()
        want.append(dict(_snap(p), frames_m=p.frames()))
    assert all(w['counts'].sum() > 0 for w in want)
    # the calibration matters to the records: the same step under another one gives other records
    fresh['A'].run(*ins[1]['args'][:2], [ctx.array(np.ascontiguousarray(synth.image_frame(SEQ, f))) for f in (2, 4)],
                   ego_motion=ins[1]['ego'])
    fresh['A'].finish()
    ctx.sync()
    assert _snap(fresh['A'])['records'].tobytes() != want[1]['records'].tobytes()
    yield dict(sw=sw, fresh=fresh, ins=ins, want=want)
    for p in list(fresh.values()) + [sw]:
        p.close()


def _run(pipe, step, lookahead=None, calib=True):
    pipe.run(*step['args'], ego_motion=step['ego'], recover=step['recover'], lookahead=lookahead,
             **(dict(calib=step['calib']) if calib else {}))


def test_step_by_step(ctx, pair_case):
    sw, ins, want = pair_case['sw'], pair_case['ins'], pair_case['want']
    for k, step in enumerate(ins):
        _run(sw, step, calib=STEPS[k] != 'A' or k > 0)       # (step 0: the default, no argument)
        sw.finish()
        ctx.sync()
        _same_step(_snap(sw), want[k], 'step %d' % k)
        assert _equal(sw.frames(), want[k]['frames_m']), k
    assert sw.support.rebuilds == 3
    assert 0 < sw.bev_skipped_items <= pair_case['fresh']['A'].bev_skipped_items   # the union of three supports


def test_free_running_into_a_record_ring(ctx, pair_case):
    sw, ins, want = pair_case['sw'], pair_case['ins'], pair_case['want']
    n = len(ins)
    ring = (ctx.zeros((n, 1, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((n, 1, 2), np.int32))
    sw.use_record_ring(*ring)
    k0 = sw.step_idx
    for step in ins:
        _run(sw, step)
    sw.finish()
    ctx.sync()
    recs, cnts = ring[0].download(), ring[1].download()
    for k in range(n):
        assert np.array_equal(cnts[(k0 + k) % n], want[k]['counts']), k
        assert recs[(k0 + k) % n].tobytes() == want[k]['records'].tobytes(), k
    _same_step(_snap(sw), want[-1], 'last step')
    pair_case['ring'] = ring


def test_with_lookahead(ctx, pair_case):
    sw, ins, want = pair_case['sw'], pair_case['ins'], pair_case['want']
    n = len(ins)
    ring = pair_case.get('ring') or (ctx.zeros((n, 1, 2, MAX_DET, REC_COLS), np.float32), ctx.zeros((n, 1, 2), np.int32))
    sw.use_record_ring(*ring)
    k0 = sw.step_idx
    for k, step in enumerate(ins):
        nxt = ins[k + 1] if k + 1 < n and k != 2 else None       # (step 3 comes unannounced)
        _run(sw, step, lookahead=nxt and nxt['args'] + (nxt['ego'], nxt['calib']))
    sw.finish()
    ctx.sync()
    recs, cnts = ring[0].download(), ring[1].download()
    for k in range(n):
        assert np.array_equal(cnts[(k0 + k) % n], want[k]['counts']), k
        assert recs[(k0 + k) % n].tobytes() == want[k]['records'].tobytes(), k
    _same_step(_snap(sw), want[-1], 'last step')
    pair_case['ring'] = ring


def test_without_bev_input_skip(ctx, pair_case):
    ins, want = pair_case['ins'], pair_case['want']
    kw = dict(KW, head_params=synth.head_params())
    sw = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), n_points_max=N_POINTS, bev_input_skip=False,
                           reuse_streams_of=pair_case['sw'], **kw)
    assert sw.support is None and sw.bev_skipped_items == 0
    for k, step in enumerate(ins):
        _run(sw, step)
        sw.finish()
        ctx.sync()
        _same_step(_snap(sw), want[k], 'step %d' % k)
    sw.close()


def test_two_pairs_of_different_calibrations_in_one_step(ctx, pair_case):
    ins, want = pair_case['ins'], pair_case['want']
    kw = dict(KW, head_params=synth.head_params())
    sw = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), n_points_max=N_POINTS, pairs_per_step=2,
                           reuse_streams_of=pair_case['sw'], **kw)
    for a, b in ((1, 2), (4, 3)):                 # (B, C) and (A, B)
        args = tuple(x + y for x, y in zip(ins[a]['args'], ins[b]['args']))
        sw.run(*args, ego_motion=ins[a]['ego'] + ins[b]['ego'], recover=ins[a]['recover'] + ins[b]['recover'],
               calib=[ins[a]['calib'], ins[b]['calib']])
        sw.finish()
        ctx.sync()
        got = _snap(sw)
        frames_m = sw.frames()
        for i, k in enumerate((a, b)):
            part = dict(records=got['records'][i:i + 1], counts=got['counts'][i:i + 1], frames=got['frames'][2 * i:2 * i + 2])
            _same_step(part, want[k], 'pair %d of the step = step %d' % (i, k))
            # M recovered each pair with its own calibration (one row per pair on the device)
            assert _equal(frames_m[i], want[k]['frames_m'][0]), (i, k)
    sw.close()


def test_refusals_on_the_device(ctx, pair_case):
    sw, ins = pair_case['sw'], pair_case['ins']
    k = sw.step_idx
    with pytest.raises(ValueError):
        _run(sw, dict(ins[0], calib=B))           # A-sized images with B
    with pytest.raises(ValueError):
        _run(sw, dict(ins[1], calib=[B, B]))
    assert sw.step_idx == k
    _run(sw, ins[1])
    sw.finish()
    ctx.sync()
    _same_step(_snap(sw), pair_case['want'][1], 'after the refusals')


# ---- 3. sequence mode: two sequences, two calibrations, one pipeline ---------------------------------------------------
def test_two_sequences_two_calibrations(ctx):
    kw = dict(rpn_nms_size=1024, head_params=synth.head_params(), temporal=TEMPORAL, tracker=TRACKER, sequence=True,
              n_points_max=N_POINTS)
    sq = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), **kw)
    assert sq.image_wh_max == (1242, 375)
    sequences = [(B, (0, 1, 2, 3), False), (C, (3, 4, 5), True)]     # (calibration, keyframes, from host memory)
    pts = [synth.lidar_frame(SEQ, 2 * j, N_POINTS) for j in range(6)]
    pinned = []
    for cal, ks, host in sequences:
        fresh = FramePairPipeline(ctx, CFG, **synth.pipeline_weights(CFG), reuse_streams_of=sq, **_as_ctor(cal), **kw)
        frames = [(ctx.array(pts[j]), len(pts[j]), ctx.array(_image(2 * j, cal))) for j in ks]
        want = []
        assert fresh.push_frame(*frames[0]) is None
        for i in range(1, len(ks)):
            ego = EGO[ks[i]]
            fresh.push_frame(*frames[i], ego_motion=ego, recover=[_recover(ego)])
            fresh.finish()
            ctx.sync()
            want.append((_snap(fresh), fresh.frames()))
        want_tracks = fresh.end_sequence()
        assert all(w[0]['counts'].sum() > 0 for w in want) and len(want_tracks) > 0
        fresh.close()
        if host:        # pinned arrays of the sample's own image size, smaller than the staging buffer
            args = []
            for j in ks:
                hp, hi = ctx.pinned((N_POINTS, 4), np.float32), ctx.pinned((cal.image_wh[1], cal.image_wh[0], 3), np.uint8)
                hp.a[:len(pts[j])] = pts[j]
                hi.a[...] = _image(2 * j, cal)
                args.append((hp, len(pts[j]), hi))
                pinned += [hp, hi]
            push = sq.push_frame_from_host
        else:
            args, push = frames, sq.push_frame
        assert push(*args[0], calib=cal) is None
        for i in range(1, len(ks)):
            ego = EGO[ks[i]]
            with pytest.raises(ValueError):                       # one calibration per sequence
                sq.push_frame(*frames[i], ego_motion=ego, recover=[_recover(ego)], calib=A)
            push(*args[i], ego_motion=ego, recover=[_recover(ego)], calib=cal)
            sq.finish()
            ctx.sync()
            _same_step(_snap(sq), want[i - 1][0], 'keyframes %d, %d' % (ks[i - 1], ks[i]))
            assert _equal(sq.frames(), want[i - 1][1]), ks[i]
        assert _equal(sq.end_sequence(), want_tracks)
    if sq.support is not None:
        assert sq.support.rebuilds == 3
    sq.close()
    for h in pinned:
        h.free()
