"""The Kalman-filter tracker on the device (dodt_amd/csrc/kalman.hip): the filter against the reference's vectors, the
assignment solver against scipy's optimum, the association's IoU matrix and the whole tracker against the host module
(dodt_amd.experiments.video_detection_kf), and the state carried across calls."""
import copy
import itertools
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _kalman_cases as K
from dodt_amd import config, device, ops
from dodt_amd import tracking as dev
from dodt_amd.experiments import video_detection_kf as vkf

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'kalman.npz'))
SIGMA_L, GATE = 0.3, 0.1


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


# ---- 1. the filter against the reference's vectors -------------------------------------------------------------------
def _filter_steps(ctx, cases):
    n, m = len(cases), max(len(G['c%d_ops' % c]) for c in cases)
    x0, lr = np.zeros((n, 4)), np.zeros((n, 3))
    opsv, zs, n_ops = np.zeros((n, m), np.int32), np.zeros((n, m, 4)), np.zeros((n,), np.int32)
    for i, c in enumerate(cases):
        k = len(G['c%d_ops' % c])
        x0[i], n_ops[i] = G['c%d_x0' % c], k
        lr[i] = [10.0] + list(G['c%d_LR' % c])       # (P0 is the class's, L and R_scaler are set afterwards)
        opsv[i, :k], zs[i, :k] = G['c%d_ops' % c] != 0, G['c%d_z' % c]
    d_x, d_p = ctx.zeros((n, m, 8), np.float64), ctx.zeros((n, m, 8, 8), np.float64)
    ops.kf_filter_steps(ctx, ctx.array(x0), ctx.array(opsv), ctx.array(zs), ctx.array(n_ops), ctx.array(lr), n, m,
                        d_x, d_p)
    return d_x.download(), d_p.download()


@pytest.mark.parametrize('cases', [[0], [1], [2], [3], [4], [5], [0, 1, 2, 3, 4, 5]])
def test_filter_matches_reference_vectors(ctx, cases):
    """The bar tests/test_kalman.py holds the host class to: rtol = atol = 1e-12 after every operation."""
    x, p = _filter_steps(ctx, cases)
    worst = 0.0
    for i, c in enumerate(cases):
        k = len(G['c%d_ops' % c])
        worst = max(worst, np.abs(x[i, :k] - G['c%d_x' % c]).max(), np.abs(p[i, :k] - G['c%d_P' % c]).max())
        np.testing.assert_allclose(x[i, :k], G['c%d_x' % c], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(p[i, :k], G['c%d_P' % c], rtol=1e-12, atol=1e-12)
    print('cases %s: worst absolute deviation %.3g' % (cases, worst))


# ---- 2. the solver alone ---------------------------------------------------------------------------------------------
def _assign(ctx, iou, gate):
    nt, nd = iou.shape
    k = max(min(nt, nd), 1)
    d_m, d_ud, d_ut = ctx.zeros((k, 2), np.int32), ctx.zeros((max(nd, 1),), np.int32), ctx.zeros((max(nt, 1),), np.int32)
    d_c = ctx.zeros((4,), np.int32)
    ops.kf_assign(ctx, ctx.array(np.ascontiguousarray(iou, np.float32)) if iou.size else None, nt, nd, gate, d_m,
                  d_ud, d_ut, d_c)
    c = d_c.download()
    assert c[3] == 0
    return d_m.download()[:c[0]], list(d_ud.download()[:c[1]]), list(d_ut.download()[:c[2]])


def _host_lists(iou, rows, cols, gate):
    """assign_detections_to_trackers' three results for the assignment (rows ascending, cols)."""
    nt, nd = iou.shape
    ut = [t for t in range(nt) if t not in rows]
    ud = [d for d in range(nd) if d not in cols]
    m = []
    for t, d in zip(rows, cols):
        if iou[t, d] < gate:
            ut.append(int(t))
            ud.append(int(d))
        else:
            m.append([int(t), int(d)])
    return np.asarray(m, int).reshape(-1, 2), ud, ut


def _check_assignment(ctx, iou, gate):
    nt, nd = iou.shape
    m, ud, ut = _assign(ctx, iou, gate)
    # the raw assignment: the matches and the gate-failed pairs behind the never-assigned entries of both lists
    n_gate = len(ud) - (nd - min(nt, nd))
    assert n_gate == len(ut) - (nt - min(nt, nd)) and n_gate >= 0
    pairs = [tuple(p) for p in m] + list(zip(ut[len(ut) - n_gate:], ud[len(ud) - n_gate:]))
    pairs.sort()
    rows, cols = [p[0] for p in pairs], [p[1] for p in pairs]
    assert len(pairs) == min(nt, nd) and len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
    assert all(0 <= t < nt for t in rows) and all(0 <= d < nd for d in cols)
    r, c = linear_sum_assignment(-iou)
    assert iou[rows, cols].astype(np.float64).sum() == iou[r, c].astype(np.float64).sum()     # sums of k/64: exact
    hm, hud, hut = _host_lists(iou, rows, cols, gate)
    assert np.array_equal(m, hm) and ud == hud and ut == hut
    return rows, cols, (r, c)


@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (7, 7), (3, 128), (128, 3), (64, 65), (65, 64), (128, 128),
                                   (256, 128)])
def test_solver_total_equals_scipy_optimum(ctx, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for gate in (0.5, 0.0):
        iou = (rng.integers(0, 65, size=shape) / 64.0).astype(np.float32)
        _check_assignment(ctx, iou, gate)


@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (4, 6), (6, 4), (7, 7)])
def test_solver_unique_optimum_is_scipys(ctx, shape):
    """Brute force over every assignment of the smaller side: where best - second best >= 1/64, the matching is
    scipy's."""
    rng = np.random.default_rng(7 * shape[0] + shape[1])
    nt, nd = shape
    done = 0
    for _ in range(40):
        iou = (rng.integers(0, 65, size=shape) / 64.0).astype(np.float32)
        small, large = min(nt, nd), max(nt, nd)
        m64 = iou.astype(np.float64) if nt <= nd else iou.astype(np.float64).T
        totals = sorted((m64[np.arange(small), list(p)].sum() for p in itertools.permutations(range(large), small)),
                        reverse=True)
        if len(totals) > 1 and totals[0] - totals[1] < 1.0 / 64:
            continue
        rows, cols, (r, c) = _check_assignment(ctx, iou, 0.25)
        assert rows == list(r) and cols == list(c)
        done += 1
        if done == 4:
            break
    assert done > 0


def test_solver_all_zero_and_all_below_gate(ctx):
    for shape in [(5, 5), (3, 9), (9, 3)]:
        zero = np.zeros(shape, np.float32)
        m, ud, ut = _assign(ctx, zero, 0.1)
        assert len(m) == 0 and sorted(ud) == list(range(shape[1])) and sorted(ut) == list(range(shape[0]))
        _check_assignment(ctx, zero, 0.1)
        low = (np.random.default_rng(1).integers(0, 6, size=shape) / 64.0).astype(np.float32)
        m, ud, ut = _assign(ctx, low, 0.1)
        assert len(m) == 0
        _check_assignment(ctx, low, 0.1)
    # with no tracks or no detections everything on the other side is unmatched, ascending
    m, ud, ut = _assign(ctx, np.zeros((0, 4), np.float32), 0.1)
    assert len(m) == 0 and ud == [0, 1, 2, 3] and ut == []
    m, ud, ut = _assign(ctx, np.zeros((3, 0), np.float32), 0.1)
    assert len(m) == 0 and ud == [] and ut == [0, 1, 2]


# ---- 3. the IoU matrix -----------------------------------------------------------------------------------------------
def test_iou_matrix_matches_host(ctx):
    """20 x 20 boxes under a moving ego and KITTI's calibration against cal_transformed_ious cast to float32.  The
    device's cos / sin may differ in the last bits of a double (float64 agreement <= 1e-9, test_gpu_temporal.py's bar),
    which can flip one float32 rounding and no more: at most one float32 ulp of a value <= 1 apart, 2^-24."""
    rng = np.random.default_rng(5)
    n = 20
    cx, cz = rng.uniform(-10, 10, n), rng.uniform(10, 50, n)
    last = [K.det(0, cx[i], cz[i], ry=rng.uniform(-3, 3)) for i in range(n)]
    dets = [K.det(2, cx[i] + rng.normal(0, 0.7), cz[i] + rng.normal(0, 0.7) - 0.6, ry=rng.uniform(-3, 3))
            for i in rng.permutation(n)]
    for d in last + dets:
        d['boxes3d'][0:3] *= rng.uniform(0.8, 1.2, 3)
        d['boxes3d'][4] += rng.normal(0, 0.2)
    want = np.array([[vkf.cal_transformed_ious(K.moving, K.CALIB_KITTI, a, b) for b in dets] for a in last])
    d_out = ctx.zeros((n, n), np.float32)
    ops.kf_iou_matrix(ctx, ctx.array(np.array([d['boxes3d'] for d in last])), n,
                      ctx.array(np.array([d['boxes3d'] for d in dets])), n, ops.kf_ego_rows([K.moving(0, 2)])[0],
                      ops.temporal_calib(*K.CALIB_KITTI), d_out)
    got = d_out.download()
    assert np.count_nonzero(want > 0.05) >= n // 2
    diff = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    print('IoU matrix: worst float32 difference %.3g, %d entries differ' % (diff.max(), np.count_nonzero(diff)))
    assert diff.max() <= 2.0 ** -24


# ---- 4. the whole tracker against the host ---------------------------------------------------------------------------
def _both(ctx, ego, calib, build, **kw):
    """Host and device on two builds of the same scenario; the host's own matrices decide whether the case is fair."""
    frames_h, stride, total = build()
    frames_d, _, _ = build()
    want, matrices = K.host_run(ego, calib, frames_h, stride, total, SIGMA_L, GATE, **kw)
    K.assert_fair(matrices, GATE)
    got = dev.kf_pipeline(ego, calib, frames_d, stride, total, SIGMA_L, GATE, ctx=ctx, **kw)
    K.assert_same_tracks(got, frames_d, want, frames_h)
    return want


@pytest.mark.parametrize('ego', ['parked', 'moving'])
def test_kf_pipeline_follow_scenario(ctx, ego):
    """On the CPU this scenario gives, parked: 3 tracks with 8, 7, 8 hits, the smallest gap between best and second-best
    total 0.257; moving (KITTI calibration): 3 tracks with 8, 7, 8 hits, gap 0.18, no assigned IoU within 0.08 of the
    gate."""
    want = _both(ctx, K.PARKED if ego == 'parked' else K.moving, K.CALIB_ID if ego == 'parked' else K.CALIB_KITTI,
                 K.follow_scenario)
    assert [t.hits for t in want] == [8, 7, 8]
    assert any(d.get('is_virtual') and d['frame_id'] % 2 == 0 for d in want[1].dets)    # the coasted keyframe


def _seq(objects, n_key, stride=2, extra=None):
    """objects: (x0, z0, vx, vz, ry, keyframes it is seen at)."""
    def build():
        frames = []
        for k in range(n_key):
            f = [K.det(k * stride, x0 + vx * k, z0 + vz * k, ry=ry) for (x0, z0, vx, vz, ry, seen) in objects
                 if k in seen]
            frames.append(f + [K.det(k * stride, *e) for e in (extra or {}).get(k, [])])
        return frames, stride, n_key * stride
    return build


A_ = (-5.0, 30.0, 0.1, 0.5, 1.5)
B_ = (4.0, 20.0, -0.1, 0.4, 1.5)


def test_kf_empty_first_keyframe(ctx):
    want = _both(ctx, K.PARKED, K.CALIB_ID, _seq([A_ + (range(1, 5),), B_ + (range(1, 5),)], 5), min_hits=2)
    assert len(want) == 2


def test_kf_empty_keyframe_in_the_middle(ctx):
    want = _both(ctx, K.moving, K.CALIB_KITTI, _seq([A_ + ((0, 1, 3, 4),), B_ + ((0, 1, 3, 4),)], 5), min_hits=2)
    assert len(want) == 2 and all(any(d.get('is_virtual') and d['frame_id'] == 4 for d in t.dets) for t in want)


def test_kf_one_keyframe(ctx):
    want = _both(ctx, K.PARKED, K.CALIB_ID, _seq([A_ + ((0,),), B_ + ((0,),)], 1), min_hits=0)
    assert [t.id for t in want] == [0, 1] and all(t.hits == 0 and len(t.dets) == 1 for t in want)


def test_kf_track_leaves_the_wedge_while_coasting(ctx):
    """x = 10 .. 18 at z = 20: the last detection lies outside z > 1.3 |x|, so the first coasting step ends the track
    without a virtual detection."""
    out = (10.0, 20.0, 2.0, 0.0, 0.0, range(0, 5))
    want = _both(ctx, K.PARKED, K.CALIB_ID, _seq([out, A_ + (range(0, 7),)], 7))
    gone = [t for t in want if t.no_losses == 4 and t.hits == 4]
    assert len(gone) == 1 and not gone[0].dets[-1].get('is_virtual') and gone[0].dets[-1]['frame_id'] == 8


def test_kf_track_dropped_below_min_hits(ctx):
    want = _both(ctx, K.PARKED, K.CALIB_ID, _seq([A_ + (range(0, 7),)], 7, extra={1: [(1.0, 55.0, 0.95)]}))
    assert len(want) == 1 and want[0].id == 0


def test_kf_track_coasts_max_age_times_and_is_matched_again(ctx):
    still = (2.0, 25.0, 0.0, 0.0, 1.5, (0, 1, 2, 6, 7))
    want = _both(ctx, K.PARKED, K.CALIB_ID, _seq([still, A_ + (range(0, 8),)], 8))
    back = [t for t in want if t.hits == 4]
    assert len(back) == 1 and sum(1 for d in back[0].dets if d.get('is_virtual') and d['frame_id'] % 2 == 0) == 3


def test_kf_more_tracks_than_detections_and_the_reverse(ctx):
    c = (0.0, 45.0, 0.0, 0.3, 1.5)
    d = (9.0, 35.0, 0.1, 0.2, 1.5)
    objs = [A_ + ((0, 2, 3),), B_ + ((0, 1, 2, 3),), c + ((0, 1, 2, 3),), d + ((0, 2, 3),),
            (-12.0, 50.0, 0.0, 0.0, 1.5, (2, 3)), (14.0, 60.0, 0.0, 0.0, 1.5, (2, 3))]
    want = _both(ctx, K.moving, K.CALIB_KITTI, _seq(objs, 4), min_hits=1)
    assert len(want) == 6


def _grid(k, dz=0.0):
    """128 small boxes, all inside the wedge, no two touching."""
    return [{'frame_id': k, 'boxes3d': np.array([1.0, 0.5, 0.5, -7.5 + (i % 16), 1.6, 30.0 + dz + (i // 16), 0.3]),
             'boxes2d': np.array([0., 0., 5., 5.]) + i, 'scores': 0.5 + i / 1000.0} for i in range(128)]


def test_kf_128_detections_in_one_keyframe(ctx):
    def build():
        first = _grid(0)
        second = [copy.deepcopy(first[i]) for i in (100, 3, 57)]
        for s in second:
            s['frame_id'] = 2
            s['boxes3d'][3] += 0.1
        return [first, second], 2, 4
    want = _both(ctx, K.PARKED, K.CALIB_ID, build, min_hits=1)
    assert sorted(t.id for t in want) == [3, 57, 100]


def test_kf_live_track_overflow_raises(ctx):
    rows = np.zeros((3, 128, 16))
    for k in range(3):
        for i, d in enumerate(_grid(2 * k, dz=10.0 * k)):
            rows[k, i, 8:15], rows[k, i, 4:8], rows[k, i, 15] = d['boxes3d'], d['boxes2d'], d['scores']
    counts = np.full((3,), 128, np.int32)
    cal = ops.temporal_calib(*K.CALIB_ID)
    tr = dev.KalmanTracker(ctx, SIGMA_L, GATE, log_capacity=4096)
    tr.track_keyframes(ctx.array(rows[:2]), ctx.array(counts[:2]), 2, 128, [None, None], cal)
    assert tr.header()['n_live'] == 256 and tr.header()['status'] == 0
    tr.read()
    tr.track_keyframes(ctx.array(rows[2:]), ctx.array(counts[2:]), 1, 128, [None], cal)
    with pytest.raises(RuntimeError, match='live tracks'):
        tr.read()
    small = dev.KalmanTracker(ctx, SIGMA_L, GATE, log_capacity=100)
    small.track_keyframes(ctx.array(rows[:1]), ctx.array(counts[:1]), 1, 128, [None], cal)
    with pytest.raises(RuntimeError, match='log capacity'):
        small.read()
    with pytest.raises(ValueError):
        dev.kf_pipeline(K.PARKED, K.CALIB_ID, [_grid(0) + _grid(0)[:1]], 2, 2, SIGMA_L, GATE, ctx=ctx)


# ---- 5. the state carried across calls -------------------------------------------------------------------------------
def test_state_is_the_same_however_the_keyframes_are_split(ctx):
    frames, stride, total = K.follow_scenario()
    rows, counts = dev._kf_check_detections(frames, stride)
    n = len(frames)
    egos = [None] + [K.moving(k * stride - stride, k * stride) for k in range(1, n)]
    cal = ops.temporal_calib(*K.CALIB_KITTI)
    results = []
    for split in ([n], [1] * n, [4, 5]):
        tr = dev.KalmanTracker(ctx, SIGMA_L, GATE, log_capacity=512)
        at = 0
        for m in split:
            tr.track_keyframes(ctx.array(rows[at:at + m]), ctx.array(counts[at:at + m]), m, rows.shape[1],
                               egos[at:at + m], cal)
            at += m
        before = tr.used_bytes()
        tr.flush(cal)
        fin, log = tr.read()
        results.append((before, tr.used_bytes(), fin, log))
    assert results[0][0][0].view(np.int32)[0] > 0                     # live tracks before the flush
    for other in results[1:]:
        for a, b in zip(results[0][:2], other[:2]):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        assert np.array_equal(results[0][2], other[2]) and np.array_equal(results[0][3], other[3])
    assert len(results[0][2]) == 3


def test_track_records_is_track_keyframes_on_the_encoded_rows(ctx):
    """dodt_kf_track_pairs: pair j's encoded keyframe-0 rows are keyframe j, the last pair's keyframe-1 rows the final
    one at flush() -- the same tracks as kf_pipeline on those lists, on the device and on the host."""
    rng = np.random.default_rng(11)
    n_pairs, stride = 4, 2
    objs = [(-6.0, 18.0, 0.2, 0.9), (5.0, 35.0, -0.1, -0.6), (0.5, 26.0, 0.0, 0.5)]
    recs = np.zeros((n_pairs, 2, 8, 17), np.float32)
    cnts = np.zeros((n_pairs, 2), np.int32)
    for j in range(n_pairs):
        for f in range(2):
            for (x0, z0, vx, vz) in objs:
                k = j + f
                if (k, x0) == (2, 5.0):
                    continue                                        # a missed detection
                i = cnts[j, f]
                recs[j, f, i, :9] = [x0 + vx * k + rng.normal(0, 0.02), 1.6, z0 + vz * k + rng.normal(0, 0.02), 4.0,
                                     1.6, 1.5, 1.5, 0.9, 0]
                recs[j, f, i, 9:16] = recs[j, f, i, :7]
                recs[j, f, i, 16] = f
                cnts[j, f] += 1
    # keyframe j + 1 is seen twice (pair j's keyframe 1, pair j + 1's keyframe 0): make the two the same rows
    for j in range(n_pairs - 1):
        recs[j + 1, 0], cnts[j + 1, 0] = recs[j, 1], cnts[j, 1]
        recs[j + 1, 0, :, 16] = 0
    p2, wh = config.KITTI_P2, config.KITTI_IMAGE_WH
    cal = ops.temporal_calib(*K.CALIB_KITTI)
    d_recs, d_cnts = ctx.array(recs), ctx.array(cnts)
    d_trk, d_k1 = ctx.empty((n_pairs, 128, 23), np.float32), ctx.empty((n_pairs, 128, 16), np.float32)
    d_cnt = ctx.empty((n_pairs, 4), np.int32)
    ops.track_encode(ctx, d_recs, d_cnts, n_pairs, 8, p2, wh, 0.1, d_trk, d_k1, d_cnt)
    trk, k1, cnt = d_trk.download(), d_k1.download(), d_cnt.download()
    lists = [trk[j, :cnt[j, 3], :16] for j in range(n_pairs)] + [k1[n_pairs - 1, :cnt[n_pairs - 1, 1]]]
    assert [len(x) for x in lists] == [3, 3, 2, 3, 3]

    def build():
        return [[{'frame_id': k * stride, 'boxes3d': r[8:15].astype(np.float64), 'boxes2d': r[4:8].astype(np.float64),
                  'scores': float(r[15])} for r in rows] for k, rows in enumerate(lists)], stride, None
    frames_h, frames_d = build()[0], build()[0]
    want, matrices = K.host_run(K.moving, K.CALIB_KITTI, frames_h, stride, 10 ** 6, SIGMA_L, GATE, min_hits=2)
    K.assert_fair(matrices, GATE)
    K.assert_same_tracks(dev.kf_pipeline(K.moving, K.CALIB_KITTI, frames_d, stride, 10 ** 6, SIGMA_L, GATE, min_hits=2,
                                         ctx=ctx), frames_d, want, frames_h)
    for split in ([n_pairs], [1] * n_pairs):
        tr = dev.KalmanTracker(ctx, SIGMA_L, GATE, min_hits=2, log_capacity=256)
        at = 0
        for m in split:
            sl = slice(at, at + m)
            tr.track_records(ctx.array(recs[sl]), ctx.array(cnts[sl]), m, 8, p2, wh,
                             [K.moving(2 * j, 2 * j + 2) for j in range(at, at + m)], cal, score_threshold=0.1)
            at += m
        tr.flush(cal)
        fin, log = tr.read()
        got = dev.kf_tracks_from_log(fin, log, stride, real_det=lambda k, i: frames_d[k][i])
        K.assert_same_tracks(got, frames_d, want, frames_h)
    assert len(want) == 3
