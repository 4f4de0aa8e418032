"""Shared by the tracker-lanes tests (tests/test_tracker_lanes_host.py, tests/test_gpu_tracker_lanes.py,
tests/test_gpu_tracker_lanes_pipeline.py): synthetic detection records of a sequence of keyframe pairs (the generator of
tests/test_gpu_tracking.py, here with the camera as an argument so that a lane's boxes lie in ITS image), the
calibrations the lanes use, the host module's tracks of a sequence, and the comparisons.  No GPU is needed to import
it."""
import functools
import os

import numpy as np

import _real_clouds as rc
from dodt_amd import config
from dodt_amd.core import dt_evaluator_utils as host
from dodt_amd.datasets.kitti import calib as kcalib

REFERENCE = (0.1, 0.5, 0.005, 3)         # score, high, iou, t_min (the existing tracker tests' two sets)
LOOSE = (0.1, 0.6, 0.1, 2)
CLASSES = ['Car']
RECORDS = rc.records_by_tag()


def frame_ids(pair, kf):
    """sequence()'s frame ids: pair j is frames (2j, 2j + 2)."""
    return 2 * pair + 2 * kf


def calibrations():
    """{name: config.Calibration}: the default; the two calibration files under tests/golden/ with the image sizes of
    their samples (the tracking file is video 0001, whose numbers ARE the default's: a lane may take it, a third
    geometry it is not); and object frame 000006 of tests/golden/all_frames.json, so that three differ."""
    obj, trk = RECORDS['obj000000'], RECORDS['trk0001_000000']
    r0, tr, p2, wh = rc.calib_of(RECORDS['obj000006'])
    cals = dict(default=config.KITTI_CALIBRATION,
                object_file=kcalib.read_calibration(os.path.join(rc.GOLDEN, 'calib_object_000000.txt'),
                                                    (obj['w'], obj['h'])),
                tracking_file=kcalib.read_calibration(os.path.join(rc.GOLDEN, 'calib_tracking_0001.txt'),
                                                      (trk['w'], trk['h'])),
                object_000006=config.Calibration(p2, r0, tr, wh))
    assert len({cals[n].key() for n in ('default', 'object_file', 'object_000006')}) == 3
    assert len({cals[n].image_wh for n in ('default', 'object_file', 'object_000006')}) == 3
    return cals


def sequence(seed, n_pairs, n_obj=14, special=False, empty=()):
    """Records (n,17) per pair of cars driving through the camera's view, born and dying along the sequence:
    keyframe-0 rows (mark 0) with the box shifted into keyframe 1 in cols 9:16, keyframe-1 rows (mark 1).  special:
    rows that the threshold and the truncation rules (which read the image size) drop or keep on the edge."""
    rng = np.random.default_rng(seed)
    if n_pairs == 0:
        return []
    x0, z0 = rng.uniform(-14, 14, n_obj), rng.uniform(8, 45, n_obj)
    vx, vz = rng.uniform(-0.4, 0.4, n_obj), rng.uniform(-0.6, 0.9, n_obj)
    dims = np.stack([rng.uniform(3.4, 4.6, n_obj), rng.uniform(1.5, 1.8, n_obj), rng.uniform(1.4, 1.7, n_obj)], 1)
    ry = rng.uniform(-np.pi, np.pi, n_obj)
    birth = rng.integers(0, n_pairs, n_obj)
    birth[: max(n_obj // 3, 1)] = 0
    death = np.minimum(birth + rng.integers(2, max(n_pairs, 3), n_obj), n_pairs + 1)

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


def host_tracks(pairs, cal, params, classes=CLASSES):
    """The host module's finished tracks of `pairs` under the calibration `cal`."""
    score, high, iou, t_min = params
    dft, dfi = host.encode_tracking_dets(pairs, cal.p2, cal.image_wh, list(classes), score)
    return host.track_through_ious(dft, dfi, high, iou, t_min)


def pack(pairs, max_det):
    """[(frame_0, frame_1, records (n,17))] -> (n_pairs, 2, max_det, 17) float32 and counts (n_pairs, 2) int32, each
    keyframe's rows (mark column 16) in order, as the host splits them."""
    recs = np.zeros((len(pairs), 2, max_det, 17), np.float32)
    counts = np.zeros((len(pairs), 2), np.int32)
    for j, (_, _, rec) in enumerate(pairs):
        rec = np.asarray(rec, np.float32).reshape(-1, 17)
        for f in range(2):
            rows = rec[rec[:, 16] == f]
            recs[j, f, :len(rows)] = rows
            counts[j, f] = len(rows)
    return recs, counts


def max_rows(*sequences):
    return max([1] + [int((rec[:, 16] == f).sum()) for pairs in sequences for _, _, rec in pairs for f in (0, 1)])


# ---- case (a): five lanes -------------------------------------------------------------------------------------------
# (lane: calibration, pairs, seed, n_obj, special, empty pairs).  The seeds were picked on the CPU with the host module
# alone (tests/test_tracker_lanes_host.py::test_lane_cases_are_not_trivial holds them to it).
LANES_A = (
    dict(cal='default', n_pairs=48, seed=105, n_obj=20, special=False, empty=(9, 30)),
    dict(cal='object_file', n_pairs=31, seed=106, n_obj=18, special=True, empty=(4,)),
    dict(cal='object_000006', n_pairs=17, seed=107, n_obj=20, special=False, empty=(6, 7)),
    dict(cal='tracking_file', n_pairs=1, seed=108, n_obj=12, special=False, empty=()),
    dict(cal='default', n_pairs=0, seed=109, n_obj=12, special=False, empty=()),
)


@functools.lru_cache(maxsize=None)
def lane_a(i):
    c = LANES_A[i]
    return sequence(c['seed'], c['n_pairs'], c['n_obj'], c['special'], c['empty'])


@functools.lru_cache(maxsize=None)
def lane_a_tracks(i, params):
    """The reference of lane i of case (a): computed once, shared, never changed."""
    return host_tracks(lane_a(i), calibrations()[LANES_A[i]['cal']], params)


# ---- comparisons ----------------------------------------------------------------------------------------------------
def same_item(g, w, what):
    assert g['frame_id'] == w['frame_id'] and g['info'] == w['info'], what
    for k in ('boxes2d', 'boxes3d', 'offsets'):
        assert (k in g) == (k in w), (what, k)
        if k in w:
            assert g[k].dtype == np.float32 and np.array_equal(g[k], w[k]), (what, k, g[k], w[k])
    assert type(g['scores']) is np.float32 and g['scores'] == w['scores'], what


def same_tracks(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        assert g['start_frame'] == w['start_frame'], (what, n)
        assert type(g['max_score']) is np.float32 and g['max_score'] == w['max_score'], (what, n)
        assert len(g['trajectory']) == len(w['trajectory']), (what, n)
        for i, (a, b) in enumerate(zip(g['trajectory'], w['trajectory'])):
            same_item(a, b, '%s track %d det %d' % (what, n, i))


def same_read(got, want, what):
    """Two Tracker.read() results: start frame, score bits and log rows equal."""
    assert len(got) == len(want), (what, len(got), len(want))
    for n, ((gs, gm, gr), (ws, wm, wr)) in enumerate(zip(got, want)):
        assert gs == ws and gm.tobytes() == wm.tobytes() and np.array_equal(gr, wr), (what, n)


# the state layout (dodt_amd/tracking.py): header, act (256 x 32 bytes), prev_off (256 x 7 float32), prev_k1 (128 x 16
# float32), then fin (cap x 16 bytes) and log (cap x 112 bytes)
ACT_OFF, PREV_OFF_OFF, PREV_K1_OFF, FIN_OFF = 64, 64 + 256 * 32, 64 + 256 * 32 + 256 * 28, 64 + 256 * 32 + 256 * 28 + 8192


def live_parts(state_bytes, cap):
    """The live parts of a downloaded state (uint8): header, act[0:n_active], prev_off[0:prev_nL], prev_k1[0:prev_n1],
    fin[0:n_fin], log[0:n_log] (the lists no further than the capacity), as bytes."""
    b = np.asarray(state_bytes, np.uint8)
    h = b[:64].view(np.int32)
    n_active, n_log, n_fin, has_prev, prev_nl, prev_n1 = (int(h[k]) for k in (0, 2, 3, 7, 9, 10))
    log_off = FIN_OFF + cap * 16
    return dict(header=b[:64].tobytes(),
                act=b[ACT_OFF:ACT_OFF + 32 * n_active].tobytes(),
                prev_off=b[PREV_OFF_OFF:PREV_OFF_OFF + 28 * (prev_nl if has_prev else 0)].tobytes(),
                prev_k1=b[PREV_K1_OFF:PREV_K1_OFF + 64 * (prev_n1 if has_prev else 0)].tobytes(),
                fin=b[FIN_OFF:FIN_OFF + 16 * min(n_fin, cap)].tobytes(),
                log=b[log_off:log_off + 112 * min(n_log, cap)].tobytes())
